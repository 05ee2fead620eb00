// memory_host_check.cpp — the owner type of csrc/de_memory.h (Dev<T>, Pinned<T>) on the host.  A stand-alone program: it declares stand-ins for the four
// HIP allocation calls over malloc / free — they count the live blocks and the calls, and can be told to fail the n-th allocation — includes de_memory.h
// and nothing else of the library, and asserts on its own counts and on pointer identity.  Built under the address and undefined-behaviour sanitizers
// (tests/test_memory_host.py): a double free, a leak or a use after free of the stand-in blocks is a sanitizer report, not only a wrong count.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/memory_host_check.cpp -o memory_host_check && ./memory_host_check
#include <stdio.h>
#include <stdlib.h>
#include <string>

// ---- the stand-ins
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipHostMallocDefault = 0, hipHostMallocMapped = 2, DE_ERR_NOMEM = -4 };
static int g_live = 0, g_allocs = 0, g_frees = 0;      // blocks alive, allocation calls that succeeded, free calls
static int g_fail_at = 0;                              // fail the n-th allocation call from now (1 = the next one); 0 = none
static int g_sticky = 0, g_cleared = 0;                // a failed allocation leaves a sticky error; hipGetLastError clears it
static unsigned g_last_flags = 0;
static std::string g_msg;
static hipError_t stub_alloc(void** p, size_t bytes) {
    if (g_fail_at && --g_fail_at == 0) { *p = nullptr; g_sticky = 1; return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    g_live++; g_allocs++;
    return hipSuccess;
}
static hipError_t stub_free(void* p) { free(p); g_live--; g_frees++; return hipSuccess; }
static hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes); }
static hipError_t hipFree(void* p) { return stub_free(p); }
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) { g_last_flags = flags; return stub_alloc(p, bytes); }
static hipError_t hipHostFree(void* p) { return stub_free(p); }
static hipError_t hipGetLastError() { const int e = g_sticky; g_cleared += e; g_sticky = 0; return e ? hipErrorOutOfMemory : hipSuccess; }
static int fail(int code, const std::string& msg) { g_msg = msg; return code; }

#include "../digital_earth_amd/csrc/de_memory.h"

static int g_checks = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { fprintf(stderr, "memory_host_check: line %d: %s\n", __LINE__, #cond); exit(1); } } while (0)

template <template <class> class B>
static void walk(const char* kind) {
    const int live0 = g_live;
    {   // ensure: a size already held makes no call and keeps the pointer; a larger one frees the old block exactly once
        B<float> b;
        CHECK(!b && b.bytes() == 0 && !b.borrowed());
        CHECK(b.ensure(64) == hipSuccess && b && b.bytes() == 64 && g_live == live0 + 1);
        float* p = b;
        const int a = g_allocs, f = g_frees;
        CHECK(b.ensure(64) == hipSuccess && b.ensure(16) == hipSuccess && b.get() == p && b.bytes() == 64 && g_allocs == a && g_frees == f);
        b[15] = 1.0f;                                   // the whole block is writable (the sanitizer watches)
        CHECK(b.ensure(256) == hipSuccess && b.bytes() == 256 && g_allocs == a + 1 && g_frees == f + 1 && g_live == live0 + 1);
        b[63] = 2.0f;
        // a failed ensure: empty, size 0, the old block freed, the sticky error cleared
        const int f2 = g_frees, cl = g_cleared;
        g_fail_at = 1;
        CHECK(b.ensure(1024) != hipSuccess && !b && b.bytes() == 0 && g_frees == f2 + 1 && g_live == live0 && g_sticky == 0 && g_cleared == cl + 1);
        // the noun form: DE_ERR_NOMEM and the message; then it works again
        g_fail_at = 1;
        CHECK(b.ensure(32, "pixel ring") == DE_ERR_NOMEM && g_msg == std::string("no ") + kind + " memory for the pixel ring" && !b);
        CHECK(b.ensure(32, "pixel ring") == 0 && b && g_live == live0 + 1);
        b.release();
        CHECK(!b && b.bytes() == 0 && g_live == live0);
        b.release();                                    // releasing an empty buffer is nothing
        CHECK(g_live == live0);
    }
    CHECK(g_live == live0);
    {   // borrow: releasing or destroying the view frees nothing, the owner then frees once
        B<int> owner;
        CHECK(owner.ensure(40) == hipSuccess);
        const int f = g_frees;
        {
            B<int> view;
            view.borrow(owner);
            CHECK(view.get() == owner.get() && view.bytes() == 40 && view.borrowed() && !owner.borrowed());
            view.release();
            CHECK(!view && !view.borrowed() && g_frees == f && owner);
            view.borrow(owner);
        }
        CHECK(g_frees == f && g_live == live0 + 1);
        owner[9] = 7;                                   // still alive
        owner.release();
        CHECK(g_frees == f + 1 && g_live == live0);
        B<int> none, view;                              // a view of nothing is nothing
        view.borrow(none);
        CHECK(!view && !view.borrowed());
    }
    {   // an ensure on a view allocates fresh memory — also when the view is large enough — and leaves the lender's block alive
        B<int> owner, view;
        CHECK(owner.ensure(40) == hipSuccess);
        view.borrow(owner);
        const int f = g_frees;
        CHECK(view.ensure(8) == hipSuccess && view.get() != owner.get() && !view.borrowed() && view.bytes() == 8 && g_frees == f && g_live == live0 + 2);
        owner[9] = 1; view[1] = 2;
        // a view that borrows again gives up what it owned
        view.borrow(owner);
        CHECK(g_frees == f + 1 && g_live == live0 + 1 && view.get() == owner.get());
        // a failed ensure on a view: empty, the lender untouched
        g_fail_at = 1;
        CHECK(view.ensure(8) != hipSuccess && !view && !view.borrowed() && owner && g_frees == f + 1);
    }
    CHECK(g_live == live0);
    {   // a lender destroyed after its borrower (de_destroy's order): each block freed once
        B<char> lender_a, lender_b;
        CHECK(lender_a.ensure(8) == hipSuccess && lender_b.ensure(8) == hipSuccess);
        const int f = g_frees;
        {
            B<char> borrower_a, borrower_b;
            borrower_a.borrow(lender_a); borrower_b.borrow(lender_b);
            CHECK(borrower_b.ensure(8) == hipSuccess);      // the borrower gets one of its own again
            CHECK(g_live == live0 + 3);
        }
        CHECK(g_frees == f + 1 && g_live == live0 + 2);     // the borrower's own block only
    }
    CHECK(g_live == live0);
    {   // move and swap transfer ownership: "upload into fresh, then swap / move in" (de_set_look)
        B<float> current, fresh;
        CHECK(current.ensure(12) == hipSuccess && fresh.ensure(24) == hipSuccess);
        float* pc = current; float* pf = fresh;
        const int f = g_frees;
        current.swap(fresh);
        CHECK(current.get() == pf && current.bytes() == 24 && fresh.get() == pc && fresh.bytes() == 12 && g_frees == f);
        current = std::move(fresh);                     // what `current` held goes, once; `fresh` is left empty
        CHECK(current.get() == pc && current.bytes() == 12 && !fresh && fresh.bytes() == 0 && g_frees == f + 1 && g_live == live0 + 1);
        B<float> moved(std::move(current));
        CHECK(moved.get() == pc && !current && g_frees == f + 1);
        // a move into a view makes it an owner; moving a view keeps it a view
        B<float> view;
        view.borrow(moved);
        B<float> view2(std::move(view));
        CHECK(view2.borrowed() && !view && g_frees == f + 1);
        view2 = std::move(moved);
        CHECK(!view2.borrowed() && view2.get() == pc && !moved && g_frees == f + 1 && g_live == live0 + 1);
    }
    CHECK(g_live == live0);
}

int main() {
    walk<Dev>("device");
    walk<Pinned>("pinned host");
    {   // the pinned twin hands hipHostMalloc its flags: default for staging and ring buffers, mapped for the words a kernel writes
        Pinned<unsigned> h;
        CHECK(h.ensure(64) == hipSuccess && g_last_flags == (unsigned)hipHostMallocDefault);
        h.release();
        CHECK(h.ensure(64, hipHostMallocMapped) == hipSuccess && g_last_flags == (unsigned)hipHostMallocMapped);
        h[0] = 0u;
    }
    CHECK(g_live == 0 && g_allocs == g_frees);
    printf("memory_host_check: %d checks, %d blocks allocated and freed, 0 alive at exit, no sanitizer report\n", g_checks, g_allocs);
    return 0;
}

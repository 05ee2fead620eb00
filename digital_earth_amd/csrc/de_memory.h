// de_memory.h — the one owner of device and pinned host memory: Dev<T> and Pinned<T>.  Every allocation of a context is a member or a local of one of
// them, so nothing is freed by hand: the destructor frees what the buffer owns, on every exit path and in `delete c`.
//   * ensure(bytes): "of at least `bytes`".  Holds that much already: nothing happens.  Otherwise the old block goes and a new one comes; on failure the
//     buffer is empty (size 0) and the sticky HIP error is cleared.  The caller sees to it that nothing on the GPU still uses a block that is replaced.
//   * borrow(other): a view of another buffer's block.  Releasing or destroying a view frees nothing; ensure() or a move into it makes it an owner again.
// No knowledge of the context: this header needs hipMalloc / hipFree / hipHostMalloc / hipHostFree, hipGetLastError and, for the noun form, fail() and
// DE_ERR_NOMEM, declared by whoever includes it (de_context.h; tools/memory_host_check.cpp declares stand-ins and runs it under the sanitizers).
#pragma once
#include <stddef.h>
#include <string>
#include <utility>

namespace {

struct DeviceMemory {
    static const char* kind() { return "device"; }
    static hipError_t get(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
    static void put(void* p) { (void)hipFree(p); }      // waits for the work that reads the block
};
struct PinnedMemory {
    static const char* kind() { return "pinned host"; }
    static hipError_t get(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
    static void put(void* p) { (void)hipHostFree(p); }
};

template <class T, class M>
class Buffer {
    T* p_ = nullptr;
    size_t bytes_ = 0;
    bool view_ = false;      // the block belongs to another buffer (borrow)
public:
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept { swap(o); }
    Buffer& operator=(Buffer&& o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~Buffer() { release(); }
    void swap(Buffer& o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); std::swap(view_, o.view_); }

    operator T*() const { return p_; }      // a kernel argument, a copy's end, `if (!buf)`, buf + n: as a raw pointer reads
    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    bool borrowed() const { return view_; }

    void release() {
        if (p_ && !view_) M::put(p_);
        p_ = nullptr; bytes_ = 0; view_ = false;
    }
    void borrow(const Buffer& o) {
        release();
        p_ = o.p_; bytes_ = o.bytes_; view_ = o.p_ != nullptr;
    }
    // flags: hipHostMalloc's (pinned memory only; 0 = hipHostMallocDefault)
    hipError_t ensure(size_t bytes, unsigned flags = 0) {
        if (p_ && !view_ && bytes_ >= bytes) return hipSuccess;
        release();
        void* q = nullptr;
        const hipError_t e = M::get(&q, bytes, flags);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
        p_ = static_cast<T*>(q); bytes_ = bytes;
        return hipSuccess;
    }
    // the same, answering DE_ERR_NOMEM "no device memory for the <what>" / "no pinned host memory for the <what>"
    int ensure(size_t bytes, const std::string& what, unsigned flags = 0) {
        if (ensure(bytes, flags) != hipSuccess) return fail(DE_ERR_NOMEM, std::string("no ") + M::kind() + " memory for the " + what);
        return 0;
    }
};

template <class T> using Dev = Buffer<T, DeviceMemory>;
template <class T> using Pinned = Buffer<T, PinnedMemory>;

}  // namespace

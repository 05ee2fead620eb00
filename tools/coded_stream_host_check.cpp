// coded_stream_host_check.cpp — the tail every coded output shares (csrc/coded_stream.h: the scan's three leaves, the 16-byte word, the compaction;
// DESIGN.md §22) compiled for the HOST under the address and undefined-behaviour sanitizers.  No GPU, no library.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/coded_stream_host_check.cpp -o coded_stream_host_check && ./coded_stream_host_check
// Each leaf runs for every thread of its workgroup in turn, on heap buffers of exactly the sizes asked for, under both parametrisations in use —
// JPEG's (2 bytes behind every piece, no trailer) and PNG's (none, a trailer of 28) — at 1, 2, 1023, 1024, 1025, 2049 and 3000 pieces whose lengths an
// LCG draws from [0, slot_bytes].  Checked, each against a serial statement: every offset; the word's four fields; every byte of the stream (front,
// pieces, what the caller puts behind them, trailer) and the sentinel behind its last byte; THE FAILURE RULE — with a capacity one byte short the
// status is overflow, with a status found set it is kept, and either way the length is `front` and no byte behind the front is written (the buffer
// ends there: one would be the sanitizer's to find); and saturation: five pieces of 2^30 bytes, whose slots do not exist, leave the last offset at
// 2^32 - 1 and the status at overflow.
// And the one serial leaf of the deflate coder that fills the pieces (csrc/png_deflate.h: png_code_lengths, thread 0's part), over host stand-ins for
// the four device calls the header's other functions name: the chain histograms of tests/deflate_cases.py (unlimited depth 16, 17, 21), 40 Fibonacci
// counts, 286 equal counts and 285 ones beside a million, on a heap PngLds.  Checked: every length in 1 .. 15, the Kraft sum exactly 1, no symbol's
// code longer than a rarer one's, the canonical first codes, and for the depth-16 chain the one repair step worked out by hand.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_DEV static inline
#include "../digital_earth_amd/csrc/coded_stream.h"

// the deflate coder's header as it stands; the device calls it names outside png_code_lengths, for one thread
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { const uint32_t old = *p; *p |= v; return old; }
static inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { const uint32_t old = *p; *p += v; return old; }
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { const unsigned long long old = *p; *p += v; return old; }
static inline void __syncthreads() {}
#if !defined(__clang__)
static inline uint32_t host_bitreverse32(uint32_t v) { uint32_t r = 0u; for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i); return r; }
#define __builtin_bitreverse32 host_bitreverse32
#endif
#include "../digital_earth_amd/csrc/png_tables.h"
#include "../digital_earth_amd/csrc/png_deflate.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static const uint32_t SLOT = 48, FRONT = 37, COMPACT_THREADS = 256;
static const uint8_t FILL = 0xA5, FRONT_BYTE = 0xF7, EXTRA_BYTE = 0xEE, TRAILER_BYTE = 0x7D;

static uint8_t piece_byte(uint32_t i, uint32_t k) { return (uint8_t)(i * 131u + k * 7u + 1u); }

// Both kernels of the tail as the device runs them; the caller's bytes (behind a moved piece, the trailer) are written as jpeg_compact_kernel and
// png_scan_kernel write theirs.  `out` holds the word, the front and `room` bytes more.
static void run_tail(CodedTail a, std::vector<uint8_t>& out, size_t room) {
    out.assign(CS_WORD_BYTES + FRONT + room, FILL);
    memset(out.data() + CS_WORD_BYTES, FRONT_BYTE, FRONT);
    a.out = out.data();
    std::vector<uint32_t> sums(CS_SCAN_THREADS, 0xA5A5A5A5u);
    for (int t = 0; t < CS_SCAN_THREADS; ++t) cs_scan_sum(a, sums.data(), t);
    for (int t = 0; t < CS_SCAN_THREADS; ++t) {
        const unsigned long long length = cs_scan_total(a, sums.data(), t);
        if (t == 0 && !*a.status) memset(a.out + CS_WORD_BYTES + length - a.trailer, TRAILER_BYTE, a.trailer);
        if (t != 0) CHECK(length == 0, "thread %d of the total answers a length", t);
    }
    for (int t = 0; t < CS_SCAN_THREADS; ++t) cs_scan_offsets(a, sums.data(), t);
    for (uint32_t i = 0; i < a.count + 2u; ++i)      // (two workgroups past the last piece: a grid rounded up)
        for (uint32_t t = 0; t < COMPACT_THREADS; ++t)
            if (cs_compact(a, i, (int)t, (int)COMPACT_THREADS) && t == 0) memset(a.out + CS_WORD_BYTES + a.offset[i] + a.len[i], EXTRA_BYTE, a.extra);
}

static void word_is(const std::vector<uint8_t>& out, uint64_t length, uint32_t status, uint32_t count, const char* what) {
    uint32_t w[4];
    memcpy(w, out.data(), sizeof(w));
    CHECK(w[0] == (uint32_t)length && w[1] == (uint32_t)(length >> 32) && w[2] == status && w[3] == count, "%s: the word is {%u, %u, %u, %u}, not {%llu, %u, %u}",
          what, w[0], w[1], w[2], w[3], (unsigned long long)length, status, count);
    uint64_t len; uint32_t st;
    cs_word_fields(out.data(), &len, &st);
    CHECK(len == length && st == status, "%s: the host reads another word than the device wrote", what);
}

static void failed_is(const std::vector<uint8_t>& out, uint32_t status, uint32_t count, const char* what) {
    word_is(out, FRONT, status, count, what);
    for (size_t k = 0; k < FRONT; ++k) CHECK(out[CS_WORD_BYTES + k] == FRONT_BYTE, "%s: the front was touched at %zu", what, k);
    for (size_t k = CS_WORD_BYTES + FRONT; k < out.size(); ++k) CHECK(out[k] == FILL, "%s: a byte behind the front was written at %zu", what, k);
}

static void sweep(uint32_t extra, uint32_t trailer, uint32_t count, uint32_t seed) {
    std::vector<uint32_t> len(count), offset(count, 0xA5A5A5A5u), status(1, 0u);
    std::vector<uint8_t> slots((size_t)count * SLOT), out;
    uint32_t r = seed;
    uint64_t total = FRONT;
    std::vector<uint64_t> want(count);
    for (uint32_t i = 0; i < count; ++i) {
        r = r * 1664525u + 1013904223u;
        len[i] = (r >> 8) % (SLOT + 1u);
        if (i == count / 2) len[i] = SLOT;      // both ends of the range, whatever the draw
        if (i == count / 3) len[i] = 0;
        want[i] = total;
        total += len[i] + extra;
        for (uint32_t k = 0; k < SLOT; ++k) slots[(size_t)i * SLOT + k] = piece_byte(i, k);
    }
    total += trailer;
    CodedTail a;
    a.slots = slots.data(); a.len = len.data(); a.offset = offset.data(); a.status = status.data(); a.out = nullptr;
    a.count = count; a.slot_bytes = SLOT; a.front = FRONT; a.extra = extra; a.trailer = trailer;
    char what[96];

    for (uint32_t spare = 0; spare < 2; ++spare) {      // the capacity exactly the stream (the buffer ends behind it), and one byte more (a sentinel does)
        snprintf(what, sizeof(what), "extra %u trailer %u count %u spare %u", extra, trailer, count, spare);
        a.capacity = (uint32_t)total + spare; status[0] = 0u;
        run_tail(a, out, (size_t)(total - FRONT) + spare);
        word_is(out, total, 0u, count, what);
        CHECK(status[0] == 0u, "%s: the status word was raised", what);
        const uint8_t* s = out.data() + CS_WORD_BYTES;
        for (size_t k = 0; k < FRONT; ++k) CHECK(s[k] == FRONT_BYTE, "%s: the front was touched at %zu", what, k);
        for (uint32_t i = 0; i < count; ++i) {
            CHECK(offset[i] == want[i], "%s: offset[%u] is %u, not %llu", what, i, offset[i], (unsigned long long)want[i]);
            for (uint32_t k = 0; k < len[i]; ++k) CHECK(s[want[i] + k] == piece_byte(i, k), "%s: byte %u of piece %u", what, k, i);
            for (uint32_t k = 0; k < extra; ++k) CHECK(s[want[i] + len[i] + k] == EXTRA_BYTE, "%s: the caller's byte %u behind piece %u", what, k, i);
        }
        for (uint32_t k = 0; k < trailer; ++k) CHECK(s[total - trailer + k] == TRAILER_BYTE, "%s: byte %u of the trailer", what, k);
        if (spare) CHECK(s[total] == FILL, "%s: the sentinel behind the stream was written", what);
    }

    // the failure rule.  The buffer ends behind the front.
    snprintf(what, sizeof(what), "extra %u trailer %u count %u, one byte short", extra, trailer, count);
    a.capacity = (uint32_t)total - 1u; status[0] = 0u;
    run_tail(a, out, 0);
    failed_is(out, CS_STATUS_OVERFLOW, count, what);
    CHECK(status[0] == CS_STATUS_OVERFLOW, "%s: the status word is %u", what, status[0]);
    for (uint32_t found : {CS_STATUS_RANGE, CS_STATUS_OVERFLOW, CS_STATUS_RANGE | CS_STATUS_OVERFLOW}) {
        snprintf(what, sizeof(what), "extra %u trailer %u count %u, status %u found set", extra, trailer, count, found);
        a.capacity = (uint32_t)total; status[0] = found;
        run_tail(a, out, 0);
        failed_is(out, found, count, what);
        CHECK(status[0] == found, "%s: the status word is %u", what, status[0]);
    }
}

static void saturation(uint32_t extra, uint32_t trailer) {
    const uint32_t count = 5;
    std::vector<uint32_t> len(count, 1u << 30), offset(count, 0xA5A5A5A5u), status(1, 0u);
    std::vector<uint8_t> out;
    CodedTail a;
    a.slots = nullptr; a.len = len.data(); a.offset = offset.data(); a.status = status.data(); a.out = nullptr;      // no slot is read: the compaction refuses
    a.count = count; a.slot_bytes = 1u << 30; a.front = FRONT; a.extra = extra; a.trailer = trailer; a.capacity = 0xfffffff0u;
    run_tail(a, out, 0);
    failed_is(out, CS_STATUS_OVERFLOW, count, "five pieces of 2^30 bytes");
    CHECK(status[0] == CS_STATUS_OVERFLOW, "five pieces of 2^30 bytes: the status word is %u", status[0]);
    for (uint32_t i = 0; i < count; ++i) {
        const uint64_t at = FRONT + (uint64_t)i * ((1ull << 30) + extra);
        CHECK(offset[i] == (at < 0xffffffffull ? (uint32_t)at : 0xffffffffu), "five pieces of 2^30 bytes: offset[%u] is %u", i, offset[i]);
    }
    CHECK(offset[count - 1] == 0xffffffffu, "the last offset is not saturated");
}

// counts in ascending order (the rank sort's result) through png_code_lengths.  `deep`: the unlimited tree is deeper than 15, so the longest code is 15.
static void code_lengths(const std::vector<uint32_t>& counts, bool deep, const uint32_t* want_count, const char* what) {
    std::vector<PngLds> heap(1);      // on the heap: one index past the struct is the sanitizer's to find
    PngLds& s = heap[0];
    memset(&s, 0xA5, sizeof(s));
    const uint32_t n = (uint32_t)counts.size();
    CHECK(n >= 2u && n <= PNG_SYMBOLS, "%s: %u symbols", what, n);
    for (uint32_t i = 0; i < 288u; ++i) s.len[i] = 0;
    for (uint32_t i = 0; i < n; ++i) {
        CHECK(i == 0u || counts[i - 1u] <= counts[i], "%s: the counts are not sorted", what);
        s.key[i] = counts[i];
        s.sorted[i] = (uint16_t)i;      // symbol i at rank i: ties are by symbol already
    }
    s.used = n;
    png_code_lengths(s);
    uint32_t kraft = 0u, handed = 0u, longest = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = s.len[i];
        CHECK(l >= 1u && l <= 15u, "%s: symbol %u has length %u", what, i, l);
        if (l >= 1u && l <= 15u) kraft += 1u << (15u - l);
        if (i) CHECK(s.len[i - 1u] >= l, "%s: symbol %u (count %u) has a longer code than the rarer symbol %u", what, i, counts[i], i - 1u);
        if (l > longest) longest = l;
    }
    for (uint32_t i = n; i < 288u; ++i) CHECK(s.len[i] == 0, "%s: a length was handed to the unused symbol %u", what, i);
    CHECK(kraft == (1u << 15), "%s: the Kraft sum is %u / 32768", what, kraft);
    CHECK(!deep || longest == 15u, "%s: the longest code is %u, not 15", what, longest);
    uint32_t code = 0u;
    for (uint32_t l = 1; l <= 15u; ++l) {
        handed += s.count[l];
        code = (code + (l > 1u ? s.count[l - 1u] : 0u)) << 1;
        CHECK(s.next[l] == code, "%s: the first code of length %u is %u, not %u", what, l, s.next[l], code);
        if (want_count) CHECK(s.count[l] == want_count[l], "%s: %u codes of length %u, not %u", what, s.count[l], l, want_count[l]);
    }
    CHECK(handed == n, "%s: %u lengths for %u symbols", what, handed, n);
}

static std::vector<uint32_t> chain_counts(uint32_t nsym) {      // tests/deflate_cases.py: chain_counts, end-of-block's one occurrence in front
    std::vector<uint32_t> c{1u, 1u};
    uint32_t s_prev = 1u, sum = 2u;
    while (c.size() < nsym + 1u) { const uint32_t next = s_prev + 1u; c.push_back(next); s_prev = sum; sum += next; }
    return c;
}

static int code_length_runs() {
    // depth 16: the lengths 1 .. 16, 16 clamp to one code each of 1 .. 14 and three of 15, a Kraft sum of 2^15 + 1; the one repair step takes a code of
    // 15 away and splits the code of 14 into two of 15
    static const uint32_t chain16[16] = {0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 4};
    code_lengths(chain_counts(16), true, chain16, "the chain of 16 literals");
    code_lengths(chain_counts(17), true, nullptr, "the chain of 17 literals");
    code_lengths(chain_counts(21), true, nullptr, "the chain of 21 literals");
    std::vector<uint32_t> fib{1u, 1u};
    while (fib.size() < 40u) fib.push_back(fib[fib.size() - 1u] + fib[fib.size() - 2u]);
    code_lengths(fib, true, nullptr, "40 Fibonacci counts");
    code_lengths(std::vector<uint32_t>(PNG_SYMBOLS, 1u), false, nullptr, "286 equal counts");
    std::vector<uint32_t> skew(PNG_SYMBOLS, 1u);
    skew.back() = 1000000u;
    code_lengths(skew, false, nullptr, "285 ones beside a million");
    code_lengths(std::vector<uint32_t>{1u, 5u}, false, nullptr, "two symbols");
    return 7;
}

int main() {
    static const uint32_t modes[2][2] = {{2u, 0u}, {0u, 28u}}, counts[] = {1, 2, 1023, 1024, 1025, 2049, 3000};
    int runs = 0;
    for (const auto& m : modes) {
        for (uint32_t count : counts) { sweep(m[0], m[1], count, 4711u + (uint32_t)runs); ++runs; }
        saturation(m[0], m[1]);
    }
    const int histograms = code_length_runs();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("coded_stream_host_check: %d sweeps of offsets, word, stream and the failure rule, saturation at 2^32 - 1, code lengths of %d histograms "
           "within 15 bits and complete, no sanitizer report\n", runs, histograms);
    return 0;
}

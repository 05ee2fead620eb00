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
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_DEV static inline
#include "../digital_earth_amd/csrc/coded_stream.h"

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

int main() {
    static const uint32_t modes[2][2] = {{2u, 0u}, {0u, 28u}}, counts[] = {1, 2, 1023, 1024, 1025, 2049, 3000};
    int runs = 0;
    for (const auto& m : modes) {
        for (uint32_t count : counts) { sweep(m[0], m[1], count, 4711u + (uint32_t)runs); ++runs; }
        saturation(m[0], m[1]);
    }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("coded_stream_host_check: %d sweeps of offsets, word, stream and the failure rule, saturation at 2^32 - 1, no sanitizer report\n", runs);
    return 0;
}

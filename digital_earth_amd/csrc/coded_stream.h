// coded_stream.h — the tail of every coded output (the JPEG stream, the PNG file, the OpenEXR file), plain C++ behind DE_DEV with no
// HIP in it: independent PIECES (restart intervals, deflate chunks) have been coded into fixed-size slots, piece i into slots[i slot_bytes ..) with its length in len[i].  One
// workgroup of CS_SCAN_THREADS takes the exclusive sum of (len[i] + extra) from `front` on — thread t owns the pieces [t run, (t + 1) run), the 1024 sums
// are taken serially by thread 0 — and writes the 16-byte word in front of the stream; a workgroup per piece then moves each slot to offset[i].
// THE FAILURE RULE: any non-zero status — raised by a coder, or here where front + sum(len + extra) + trailer passes the capacity — means a length of
// `front` and no piece moved.  A piece may lie elsewhere than in its slot (an OpenEXR block that is written raw): alt_at[i] then says where in
// `alt`.  Every load and store is range-checked; no atomics (whoever stores to the status word stores a failure, and the scan keeps what it finds
// there), no inline assembly.  tools/coded_stream_host_check.cpp runs these leaves under the address and UB sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#define CS_WORD_BYTES 16             // in front of the stream on the device: uint64 length, uint32 status, uint32 count
#define CS_STATUS_RANGE 1u           // a value outside the range a coder's worst case assumes
#define CS_STATUS_OVERFLOW 2u        // a store past a slot or past the stream's capacity
#define CS_SCAN_THREADS 1024
#define CS_NO_ALT 0xffffffffu        // alt_at[i]: piece i lies in its slot

struct CodedTail {
    uint8_t* slots;             // [count][slot_bytes]
    uint32_t* len;              // [count]: the bytes of a piece, written by its coder
    uint32_t* offset;           // [count]: where they start in the stream
    uint32_t* status;           // one word: CS_STATUS_*; cleared by the output's first kernel
    uint8_t* out;               // the 16-byte word, then the stream
    uint32_t count, slot_bytes;
    uint32_t front;             // bytes in front of the first piece (the host's, or the scan kernel's)
    uint32_t extra;             // bytes the compaction's caller puts behind every piece (JPEG's marker: 2; PNG: 0)
    uint32_t trailer;           // bytes the scan kernel puts behind the last piece (PNG's Adler-32 IDAT and IEND: 28; JPEG: 0)
    uint32_t capacity;          // of the stream, without the 16-byte word
    const uint8_t* alt = nullptr;         // where pieces lie that are not in their slots: piece i at alt[alt_at[i] ..) unless alt_at[i] is CS_NO_ALT
    const uint32_t* alt_at = nullptr;     // [count]; null with alt (JPEG, PNG): every piece lies in its slot
    uint32_t alt_bytes = 0;               // of `alt`
};

// ---- the word, written on the device and read on the host
DE_DEV void cs_write_word(uint8_t* out, unsigned long long length, uint32_t status, uint32_t count) {
    uint32_t* head = reinterpret_cast<uint32_t*>(out);      // 16-byte aligned: the buffer is
    head[0] = (uint32_t)length; head[1] = (uint32_t)(length >> 32); head[2] = status; head[3] = count;
}
static inline void cs_word_fields(const void* word, uint64_t* length, uint32_t* status) {
    uint32_t w[4];
    memcpy(w, word, sizeof(w));
    *length = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    *status = w[2];
}

// ---- the scan, as leaves of one thread around two barriers; `sums` is the workgroup's LDS, CS_SCAN_THREADS words
DE_DEV uint32_t cs_scan_run(const CodedTail& a) { return (a.count + CS_SCAN_THREADS - 1u) / CS_SCAN_THREADS; }
DE_DEV void cs_scan_sum(const CodedTail& a, uint32_t* sums, int t) {
    const uint32_t run = cs_scan_run(a), lo = (uint32_t)t * run;
    uint32_t s = 0;
    for (uint32_t i = lo; i < lo + run && i < a.count; ++i) s += a.len[i] + a.extra;
    sums[t] = s;
}
// Thread 0: the sums become where each thread's pieces start, saturated at 2^32 - 1; the word.  Answers the length it wrote (0 on the other threads).
DE_DEV unsigned long long cs_scan_total(const CodedTail& a, uint32_t* sums, int t) {
    if (t != 0) return 0ull;
    unsigned long long at = a.front;
    for (int k = 0; k < CS_SCAN_THREADS; ++k) {
        const uint32_t s = sums[k];
        sums[k] = (uint32_t)(at < 0xffffffffull ? at : 0xffffffffull);
        at += s;
    }
    uint32_t status = *a.status;
    if (at + a.trailer > (unsigned long long)a.capacity) status |= CS_STATUS_OVERFLOW;
    const unsigned long long length = status ? a.front : at + a.trailer;
    cs_write_word(a.out, length, status, a.count);
    if (status) *a.status = status;
    return length;
}
DE_DEV void cs_scan_offsets(const CodedTail& a, const uint32_t* sums, int t) {
    const uint32_t run = cs_scan_run(a), lo = (uint32_t)t * run;
    uint32_t at = sums[t];
    for (uint32_t i = lo; i < lo + run && i < a.count; ++i) { a.offset[i] = at; at += a.len[i] + a.extra; }
}

// ---- the compaction: thread t of the `threads` of piece i's workgroup; consecutive threads move consecutive bytes.  True where the piece was moved.
DE_DEV bool cs_compact(const CodedTail& a, uint32_t i, int t, int threads) {
    if (i >= a.count || *a.status) return false;      // the failure rule
    const uint32_t n = a.len[i], at = a.offset[i];
    const uint32_t alt_at = a.alt ? a.alt_at[i] : CS_NO_ALT;
    if ((unsigned long long)at + n + a.extra + a.trailer > (unsigned long long)a.capacity) return false;      // (the scan has refused such a total already)
    if (alt_at == CS_NO_ALT ? n > a.slot_bytes : (unsigned long long)alt_at + n > (unsigned long long)a.alt_bytes) return false;
    const uint8_t* src = alt_at == CS_NO_ALT ? a.slots + (size_t)i * (size_t)a.slot_bytes : a.alt + alt_at;
    uint8_t* dst = a.out + CS_WORD_BYTES + at;
    for (uint32_t k = (uint32_t)t; k < n; k += (uint32_t)threads) dst[k] = src[k];
    return true;
}

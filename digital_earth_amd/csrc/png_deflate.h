// png_deflate.h — the coder of one deflate chunk (include/digital_earth_png.h: TOKENS, CODES, ALIGNMENT), stated once for every output
// that deflates on the device: the PNG file (png_kernels.hip, whose chunks are IDATs) and the OpenEXR file (exr_kernels.hip, whose chunks are pieces of
// a scan-line block).  Device code of one 512-thread workgroup around barriers; it knows nothing of what frames a chunk.
//   thread t owns the contiguous bytes [t seg, (t + 1) seg) of the chunk.  Run starts by comparison with the previous byte; the head of the run a
//   segment begins in and the end of the run it ends in by two workgroup scans (max of the last start before, min of the first start behind).  Tokens
//   are a function of (position - head, run length) alone, so every thread walks its segment three times with the same leaf (png_walk): histogram, bit
//   count, bit packing.  Code lengths: a rank sort (one symbol per thread), Moffat-Katajainen and the length limit serially on thread 0 — 286 symbols:
//   clarity wins — and canonical codes one symbol per thread.  Bits are packed LSB first with LDS atomic ORs into an image of the framed chunk in LDS:
//   no atomics on global memory.  The Adler-32 partials (A, B) of the chunk's bytes are left in s.adler.
// Every store into the LDS image is checked against its size; one that would pass raises s.overflow instead.
// The includer brings DE_DEV and png_tables.h.
#pragma once

#define PNG_THREADS 512              // of a workgroup that codes a chunk
#define PNG_BUF_WORDS 16392          // the LDS image of one framed chunk: 65535 + 24 bytes, rounded up
#define PNG_SYMBOLS 286
#define PNG_HEADER_BITS 1222         // of a dynamic block: 3 + 5 + 5 + 4 + 19 * 3 + 287 * 4
#define PNG_NONE 0xffffffffu

struct PngLds {
    uint32_t buf[PNG_BUF_WORDS];       // the framed chunk as it will lie in the file
    uint32_t scan[PNG_THREADS];
    uint32_t freq[288], key[288], code[288];
    uint16_t sorted[288];
    uint8_t len[288];
    uint32_t count[16], next[16];
    unsigned long long adler[2];
    uint32_t used, bits, matches, crc, overflow;
};

DE_DEV void png_put(PngLds& s, uint32_t pos, uint32_t val, uint32_t nbits) {      // nbits <= 32 at bit `pos` of the image, LSB first
    const uint32_t w = pos >> 5, sh = pos & 31u;
    if (w + 1u >= PNG_BUF_WORDS) { s.overflow = 1u; return; }
    atomicOr(&s.buf[w], val << sh);
    if (sh + nbits > 32u) atomicOr(&s.buf[w + 1u], val >> (32u - sh));
}
DE_DEV void png_put_be32(PngLds& s, uint32_t byte, uint32_t v) { png_put(s, byte * 8u, __builtin_bswap32(v), 32u); }
DE_DEV uint32_t png_byte(const PngLds& s, uint32_t i) { return (s.buf[i >> 2] >> (8u * (i & 3u))) & 0xffu; }

// inclusive scan of one value per thread; the results are left in s.scan
template <class Op>
DE_DEV void png_wg_scan(PngLds& s, uint32_t t, uint32_t v, Op op) {
    __syncthreads();
    s.scan[t] = v;
    __syncthreads();
    for (uint32_t d = 1u; d < PNG_THREADS; d <<= 1) {
        uint32_t x = s.scan[t];
        if (t >= d) x = op(s.scan[t - d], x);
        __syncthreads();
        s.scan[t] = x;
        __syncthreads();
    }
}

// The tokens of the bytes [lo, hi) of a chunk c[0 .. n).  head_before: the start of the run that c[lo] continues (used only if it continues one);
// next_after: the first run start behind hi (n if none; used only if the run goes on at hi).  emit(value, length): length 0 is the literal `value`,
// otherwise a match of that length at distance 1.  A run of 1 + r equal bytes starting at h: a literal at h; behind it, position h + 1 + k (k < r) emits
// a match of 258 where k is a multiple of 258 below 258 (r / 258), a match of r mod 258 at k = 258 (r / 258) if that is at least 3, else a literal.
template <class Emit>
DE_DEV void png_walk(const uint8_t* c, uint32_t n, uint32_t lo, uint32_t hi, uint32_t head_before, uint32_t next_after, Emit emit) {
    uint32_t i = lo;
    uint32_t h = (lo == 0u || lo >= hi || c[lo] != c[lo - 1u]) ? lo : head_before;
    while (i < hi) {
        const uint32_t b = c[i];
        uint32_t j = i;
        while (j + 1u < hi && c[j + 1u] == b) ++j;
        uint32_t e = j;
        if (j + 1u == hi && hi < n && c[hi] == b) e = next_after - 1u;
        const uint32_t r = e - h, full = r / 258u, rem = r - full * 258u;
        uint32_t p = i;
        if (p == h) { emit(b, 0u); ++p; }
        if (p <= j) {
            const uint32_t k = p - h - 1u;
            uint32_t q = k / 258u, kk = k - q * 258u;
            for (; p <= j; ++p) {
                if (q < full) { if (kk == 0u) emit(b, 258u); }
                else if (rem >= 3u) { if (kk == 0u) emit(b, rem); }
                else emit(b, 0u);
                if (++kk == 258u) { kk = 0u; ++q; }
            }
        }
        i = j + 1u;
        h = i;
    }
}

// Thread 0: s.key[0 .. m) holds the used symbols' counts in ascending order (ties by symbol), s.sorted the symbols.  Lengths by Moffat and Katajainen's
// in-place minimum-redundancy construction, limited to 15 by the Kraft repair stated in the header, then handed out: the shortest to the most frequent.
DE_DEV void png_code_lengths(PngLds& s) {
    const int n = (int)s.used;
    if (n < 2) return;      // (a chunk always uses a literal and end-of-block)
    uint32_t* A = s.key;
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
    }
    A[n - 2] = 0u;
    for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1u;
    int avbl = 1, used = 0, depth = 0;
    root = n - 2; next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == depth) { ++used; --root; }
        while (avbl > used) { A[next--] = (uint32_t)depth; --avbl; }
        avbl = 2 * used; ++depth; used = 0;
    }
    for (int l = 0; l < 16; ++l) s.count[l] = 0u;
    for (int i = 0; i < n; ++i) s.count[A[i] < 15u ? A[i] : 15u]++;
    uint32_t total = 0u;
    for (int l = 1; l <= 15; ++l) total += s.count[l] << (15 - l);
    while (total != (1u << 15)) {
        s.count[15]--;
        for (int l = 14; l >= 1; --l)
            if (s.count[l]) { s.count[l]--; s.count[l + 1] += 2u; break; }
        --total;
    }
    int j = n;
    for (int l = 1; l <= 15; ++l)
        for (uint32_t k = s.count[l]; k > 0u; --k) s.len[s.sorted[--j]] = (uint8_t)l;
    uint32_t code = 0u;
    s.next[0] = 0u;
    for (int l = 1; l <= 15; ++l) { code = (code + s.count[l - 1]) << 1; s.next[l] = code; }
}

// The chunk c[0 .. n) as deflate data into the LDS image from byte d0 on: one block — dynamic, or stored if that is not longer — with BFINAL where
// `final_chunk`, and behind every other chunk the empty stored block.  Every thread of the workgroup calls it (it holds barriers); it clears the image
// as far as the chunk and its framing can reach and the counters first, so the caller puts its framing AFTER the call and holds a barrier of its own
// before it reads the image.  Answers the first byte behind the deflate data; the chunk's Adler sums (A, B from (0, 0), not reduced) are in s.adler.
DE_DEV uint32_t png_code_chunk(PngLds& s, const PngTables& T, const uint8_t* c, uint32_t n, uint32_t t, uint32_t d0, bool final_chunk) {
    const uint32_t seg = (n + PNG_THREADS - 1u) / PNG_THREADS;
    const uint32_t lo = t * seg < n ? t * seg : n, hi = lo + seg < n ? lo + seg : n;

    // the image cleared as far as this chunk can reach, the counters
    const uint32_t reach = (n + PNG_CHUNK_OVERHEAD + 3u) / 4u + 1u;
    for (uint32_t w = t; w < reach && w < PNG_BUF_WORDS; w += PNG_THREADS) s.buf[w] = 0u;
    if (t < 288u) { s.freq[t] = 0u; s.len[t] = 0u; s.code[t] = 0u; }
    if (t == 0u) { s.adler[0] = 0ull; s.adler[1] = 0ull; s.used = 0u; s.bits = 0u; s.matches = 0u; s.crc = 0u; s.overflow = 0u; }

    // run starts of the segment, the Adler sums of its bytes
    uint32_t first = PNG_NONE, last = 0u;      // last: position + 1, 0 = none
    unsigned long long sa = 0ull, sb = 0ull;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t b = c[i];
        if (i == 0u || b != c[i - 1u]) { if (first == PNG_NONE) first = i; last = i + 1u; }
        sa += b; sb += (unsigned long long)(n - i) * b;
    }
    png_wg_scan(s, t, last, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
    const uint32_t head_before = t ? s.scan[t - 1u] - 1u : 0u;      // (read only where a run start lies in front: position 0 is one)
    png_wg_scan(s, PNG_THREADS - 1u - t, first, [](uint32_t x, uint32_t y) { return x < y ? x : y; });
    uint32_t next_after = t + 1u < PNG_THREADS ? s.scan[PNG_THREADS - 2u - t] : PNG_NONE;
    if (next_after == PNG_NONE) next_after = n;
    __syncthreads();

    // the histogram
    png_walk(c, n, lo, hi, head_before, next_after, [&](uint32_t v, uint32_t L) { atomicAdd(&s.freq[L ? 257u + T.len_code[L - 3u] : v], 1u); });
    if (t == 0u) atomicAdd(&s.freq[256], 1u);
    if (sa) { atomicAdd(&s.adler[0], sa); atomicAdd(&s.adler[1], sb); }
    __syncthreads();

    // code lengths: rank sort, the construction on thread 0, canonical codes
    if (t < PNG_SYMBOLS && s.freq[t]) {
        const uint32_t f = s.freq[t];
        uint32_t rank = 0u;
        for (uint32_t j = 0u; j < PNG_SYMBOLS; ++j) {
            const uint32_t g = s.freq[j];
            if (g && (g < f || (g == f && j < t))) ++rank;
        }
        s.sorted[rank] = (uint16_t)t; s.key[rank] = f;
        atomicAdd(&s.used, 1u);
    }
    __syncthreads();
    if (t == 0u) png_code_lengths(s);
    __syncthreads();
    if (t < PNG_SYMBOLS && s.len[t]) {
        const uint32_t l = s.len[t];
        uint32_t code = s.next[l];
        for (uint32_t j = 0u; j < t; ++j) code += s.len[j] == l ? 1u : 0u;
        s.code[t] = __builtin_bitreverse32(code) >> (32u - l);
        const uint32_t extra = t >= 257u ? (uint32_t)T.len_extra[t - 257u] + 1u : 0u;      // a match's extra bits and its one-bit distance code
        atomicAdd(&s.bits, s.freq[t] * (l + extra));
        if (t >= 257u) atomicAdd(&s.matches, s.freq[t]);
    }
    __syncthreads();

    // the block: dynamic only if that is shorter than stored
    const uint32_t dyn_bits = PNG_HEADER_BITS + s.bits;
    const bool stored = (dyn_bits + 7u) / 8u >= n + 5u;
    uint32_t end_bit;
    if (stored) {
        if (t == 0u) {
            png_put(s, d0 * 8u, final_chunk ? 1u : 0u, 8u);
            png_put(s, d0 * 8u + 8u, n | ((~n & 0xffffu) << 16), 32u);
        }
        for (uint32_t i = lo; i < hi; ++i) png_put(s, (d0 + 5u + i) * 8u, c[i], 8u);
        end_bit = (d0 + 5u + n) * 8u;
    } else {
        const uint32_t b0 = d0 * 8u;
        if (t == 0u) {
            png_put(s, b0, (final_chunk ? 1u : 0u) | (2u << 1) | (29u << 3) | (0u << 8) | (15u << 13), 17u);
            // the code-length code in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15: none for 16, 17, 18, four bits for each of 0 .. 15
            png_put(s, b0 + 17u, 0u, 9u);
            png_put(s, b0 + 26u, 0x924924u, 24u);
            png_put(s, b0 + 50u, 0x924924u, 24u);
        }
        if (t <= PNG_SYMBOLS) {      // the 286 lengths and the distance code's, each as the 4-bit code of its value, most significant bit first
            const uint32_t l = t < PNG_SYMBOLS ? s.len[t] : (s.matches ? 1u : 0u);
            png_put(s, b0 + 74u + 4u * t, __builtin_bitreverse32(l) >> 28, 4u);
        }
        uint32_t mine = 0u;
        png_walk(c, n, lo, hi, head_before, next_after, [&](uint32_t v, uint32_t L) {
            if (L) { const uint32_t x = T.len_code[L - 3u]; mine += s.len[257u + x] + T.len_extra[x] + 1u; } else mine += s.len[v];
        });
        png_wg_scan(s, t, mine, [](uint32_t x, uint32_t y) { return x + y; });
        uint32_t at = b0 + PNG_HEADER_BITS + (t ? s.scan[t - 1u] : 0u);
        png_walk(c, n, lo, hi, head_before, next_after, [&](uint32_t v, uint32_t L) {
            if (L) {
                const uint32_t x = T.len_code[L - 3u], l = s.len[257u + x], e = T.len_extra[x];
                png_put(s, at, s.code[257u + x] | ((L - T.len_base[x]) << l), l + e + 1u);
                at += l + e + 1u;
            } else { png_put(s, at, s.code[v], s.len[v]); at += s.len[v]; }
        });
        end_bit = b0 + dyn_bits;
        if (t == 0u) png_put(s, end_bit - s.len[256], s.code[256], s.len[256]);
    }
    uint32_t end = (end_bit + 7u) / 8u;
    if (!final_chunk) {      // an empty stored block: three zero bits, padding, LEN 0, NLEN 0xFFFF
        end = (end_bit + 3u + 7u) / 8u;
        if (t == 0u) png_put(s, (end + 2u) * 8u, 0xffffu, 16u);
        end += 4u;
    }
    return end;
}

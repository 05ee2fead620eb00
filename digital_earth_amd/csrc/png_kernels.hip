// png_kernels.hip — the opt-in PNG output behind the packed outputs (include/digital_earth_png.h): the bytes pixels_pack_kernel or
// hdr_pack_kernel wrote into a buffer this stage owns become one complete, lossless PNG file behind the front the host composed.  Integer arithmetic
// only; four kernels, one after the other on the context stream:
//   png_filter_kernel    one 256-thread workgroup per row: the five candidates' costs (sum of |filtered byte as int8|) by a wave reduction and an LDS
//                        add per wave, the lowest wins (ties: the lowest type), then the winning filtered row behind its type byte into S.
//   png_deflate_kernel   one 512-thread workgroup per chunk of S; thread t owns the contiguous bytes [t seg, (t + 1) seg).  Run starts by comparison with
//                        the previous byte; the head of the run a segment begins in and the end of the run it ends in by two workgroup scans (max of the
//                        last start before, min of the first start behind).  Tokens are a function of (position - head, run length) alone, so every
//                        thread walks its segment three times with the same leaf (png_walk): histogram, bit count, bit packing.  Code lengths: a rank
//                        sort (one symbol per thread), Moffat-Katajainen and the length limit serially on thread 0 — 286 symbols: clarity wins — and
//                        canonical codes one symbol per thread.  Bits are packed LSB first with LDS atomic ORs into an image of the whole IDAT chunk
//                        (length, type, data, CRC) in LDS: no atomics on global memory.  The CRC-32 of the IDAT: a piece per thread through the byte
//                        table, shifted behind the end by the host's shift-by-2^k-bytes operators, XORed together.  The Adler-32 partials (A, B) of the
//                        chunk's bytes go to adler[2 k], adler[2 k + 1].  The image leaves LDS for the chunk's slot as whole words.
//   png_scan_kernel      one workgroup: the coded tail's scan (coded_stream.h, DESIGN.md §22: the exclusive sum of the slots' lengths, the offsets, the
//                        16-byte word) with nothing behind a piece and a trailer of 28 bytes, and what is PNG's alone: the front, the Adler partials
//                        joined along the same split (png_adler_join), the trailer (the IDAT that holds the Adler-32, IEND).
//   png_compact_kernel   one workgroup per chunk: the shared compaction of its slot to its final place.
// THE WORST CASE of a slot (png_tables.h: PNG_CHUNK_OVERHEAD).  A chunk of n filtered bytes is written as a dynamic block only if that takes FEWER than
// n + 5 bytes — the stored block's size — so its deflate data is at most 2 (CMF / FLG) + n + 5 + 5 (the empty stored block behind a non-final chunk:
// 3 bits, padding, LEN, NLEN) and the IDAT around it 12 more: n + 24.  Every store into the LDS image and into a slot is checked against that; one that
// would pass raises the status word instead, and the conversion ends with DE_ERR_INTERNAL.
// Included into de_api.hip's translation unit behind jpeg_kernels.hip; it touches no other kernel.
#include "de_kernels.h"
#include "png_tables.h"
#include "coded_stream.h"

#define PNG_FILTER_THREADS 256
#define PNG_THREADS 512              // of the deflate kernel
#define PNG_BUF_WORDS 16392          // the LDS image of one IDAT: 65535 + 24 bytes, rounded up
#define PNG_SYMBOLS 286
#define PNG_HEADER_BITS 1222         // of a dynamic block: 3 + 5 + 5 + 4 + 19 * 3 + 287 * 4
#define PNG_FILTER_ADAPTIVE 5
#define PNG_NONE 0xffffffffu

struct PngArgs : CodedTail {    // the pieces are the chunks' IDATs: count of them; front: the bytes of front_bytes; trailer: PNG_TRAILER_BYTES
    const uint8_t* pixels;      // [H][row_bytes], rows top-down; 16-bit samples little-endian (swap16: PNG wants them big-endian)
    const PngTables* tab;
    uint8_t* filtered;          // S: [H][1 + row_bytes]
    uint32_t* adler;            // [count][2]: A and B of the chunk's own bytes, from (0, 0)
    int H, bpp, swap16, filter, chunk_bytes;
    uint32_t row_bytes, total;  // total: N
    uint8_t front_bytes[PNG_FRONT_MAX];
};

// ---- the filter
DE_DEV uint32_t png_sample(const PngArgs& a, size_t row, uint32_t i) { return a.pixels[row * a.row_bytes + (a.swap16 ? (i ^ 1u) : i)]; }
DE_DEV uint32_t png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}
DE_DEV uint32_t png_filtered(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t pred = type == 0 ? 0u : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : png_paeth((int)a, (int)b, (int)c);
    return (x - pred) & 0xffu;
}
DE_DEV void png_neighbours(const PngArgs& a, uint32_t y, uint32_t i, uint32_t* x, uint32_t* l, uint32_t* u, uint32_t* ul) {
    const bool left = i >= (uint32_t)a.bpp, up = y > 0u;
    *x = png_sample(a, y, i);
    *l = left ? png_sample(a, y, i - (uint32_t)a.bpp) : 0u;
    *u = up ? png_sample(a, y - 1u, i) : 0u;
    *ul = (left && up) ? png_sample(a, y - 1u, i - (uint32_t)a.bpp) : 0u;
}

__global__ void __launch_bounds__(PNG_FILTER_THREADS) png_filter_kernel(PngArgs a) {
    __shared__ uint32_t cost[5];
    const uint32_t y = blockIdx.x, t = threadIdx.x;
    if (y == 0u && t == 0u) *a.status = 0u;
    if (y >= (uint32_t)a.H) return;
    if (t < 5u) cost[t] = 0u;
    __syncthreads();
    int type = a.filter;
    if (type == PNG_FILTER_ADAPTIVE) {
        uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
        for (uint32_t i = t; i < a.row_bytes; i += PNG_FILTER_THREADS) {
            uint32_t x, l, u, ul;
            png_neighbours(a, y, i, &x, &l, &u, &ul);
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                const uint32_t v = png_filtered(f, x, l, u, ul);
                c[f] += v < 128u ? v : 256u - v;
            }
        }
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            uint32_t v = c[f];
            for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
            if ((t & 63u) == 0u) atomicAdd(&cost[f], v);
        }
        __syncthreads();
        type = 0;
        for (int f = 1; f < 5; ++f)
            if (cost[f] < cost[type]) type = f;
    }
    uint8_t* dst = a.filtered + (size_t)y * (1u + (size_t)a.row_bytes);
    if (t == 0u) dst[0] = (uint8_t)type;
    for (uint32_t i = t; i < a.row_bytes; i += PNG_FILTER_THREADS) {
        uint32_t x, l, u, ul;
        png_neighbours(a, y, i, &x, &l, &u, &ul);
        dst[1u + i] = (uint8_t)png_filtered(type, x, l, u, ul);
    }
}

// ---- the coder of one chunk
struct PngLds {
    uint32_t buf[PNG_BUF_WORDS];       // the IDAT chunk as it will lie in the file
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

__global__ void __launch_bounds__(PNG_THREADS) png_deflate_kernel(PngArgs a) {
    __shared__ PngLds s;
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    if (k >= a.count) return;
    const uint32_t base = k * (uint32_t)a.chunk_bytes;
    const uint32_t n = a.total - base < (uint32_t)a.chunk_bytes ? a.total - base : (uint32_t)a.chunk_bytes;
    const bool final_chunk = k + 1u == a.count;
    const uint8_t* c = a.filtered + base;
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
    const PngTables& T = *a.tab;
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
    const uint32_t d0 = 8u + (k == 0u ? 2u : 0u);      // the block's first byte in the image
    const uint32_t dyn_bits = PNG_HEADER_BITS + s.bits;
    const bool stored = (dyn_bits + 7u) / 8u >= n + 5u;
    uint32_t end_bit;
    if (t == 0u) {
        png_put(s, 32u, 0x54414449u, 32u);      // "IDAT"
        if (k == 0u) png_put(s, 64u, 0x0178u, 16u);
    }
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
    if (t == 0u) png_put_be32(s, 0u, end - 8u);
    __syncthreads();

    // the CRC-32 of type and data: a piece per thread, shifted behind the end, XORed together
    const uint32_t crc_bytes = end - 4u, piece = (crc_bytes + PNG_THREADS - 1u) / PNG_THREADS;
    const uint32_t p0 = 4u + t * piece, p1 = p0 + piece < end ? p0 + piece : end;
    if (p0 < end && end <= PNG_BUF_WORDS * 4u) {
        uint32_t r = t == 0u ? 0xffffffffu : 0u;
        for (uint32_t i = p0; i < p1; ++i) r = T.crc[(r ^ png_byte(s, i)) & 0xffu] ^ (r >> 8);
        const uint32_t rest = end - p1;
        for (int m = 0; m < PNG_SHIFT_OPS; ++m)
            if ((rest >> m) & 1u) r = png_gf2_times(T.shift[m], r);
        atomicXor(&s.crc, r);
    }
    __syncthreads();
    if (t == 0u) png_put_be32(s, end, s.crc ^ 0xffffffffu);
    __syncthreads();

    const uint32_t bytes = end + 4u;
    const bool fits = !s.overflow && bytes <= a.slot_bytes && bytes <= PNG_BUF_WORDS * 4u;
    if (fits) {
        uint32_t* slot = reinterpret_cast<uint32_t*>(a.slots + (size_t)k * (size_t)a.slot_bytes);      // 16-byte aligned; slot_bytes is a multiple of 16
        for (uint32_t w = t; w < (bytes + 3u) / 4u; w += PNG_THREADS) slot[w] = s.buf[w];
    }
    if (t == 0u) {
        a.len[k] = fits ? bytes : 0u;
        a.adler[2u * k] = (uint32_t)(s.adler[0] % PNG_ADLER);
        a.adler[2u * k + 1u] = (uint32_t)(s.adler[1] % PNG_ADLER);
        if (!fits) *a.status = CS_STATUS_OVERFLOW;
    }
}

// ---- the scan: thread t owns chunks [t run, (t + 1) run)
__global__ void __launch_bounds__(CS_SCAN_THREADS) png_scan_kernel(PngArgs a) {
    __shared__ uint32_t sums[CS_SCAN_THREADS];
    __shared__ uint32_t ad_a[CS_SCAN_THREADS], ad_b[CS_SCAN_THREADS], ad_n[CS_SCAN_THREADS];
    const uint32_t t = threadIdx.x;
    const uint32_t run = cs_scan_run(a), lo = t * run;
    cs_scan_sum(a, sums, (int)t);
    unsigned long long A = 0ull, B = 0ull, count = 0ull;      // the Adler state behind this thread's chunks, from (0, 0), and their filtered bytes
    for (uint32_t i = lo; i < lo + run && i < a.count; ++i) {
        const uint32_t n = a.total - i * (uint32_t)a.chunk_bytes < (uint32_t)a.chunk_bytes ? a.total - i * (uint32_t)a.chunk_bytes : (uint32_t)a.chunk_bytes;
        png_adler_join(&A, &B, n, a.adler[2u * i], a.adler[2u * i + 1u]);
        count += n;
    }
    ad_a[t] = (uint32_t)A; ad_b[t] = (uint32_t)B; ad_n[t] = (uint32_t)count;
    if (t < a.front) a.out[CS_WORD_BYTES + t] = a.front_bytes[t];
    __syncthreads();
    const unsigned long long length = cs_scan_total(a, sums, (int)t);
    if (t == 0u && !*a.status) {      // the trailer, behind the last piece: the threads' Adler states joined from (1, 0)
        A = 1ull; B = 0ull;
        for (uint32_t j = 0u; j < CS_SCAN_THREADS; ++j) png_adler_join(&A, &B, ad_n[j], ad_a[j], ad_b[j]);
        const uint32_t adler = (uint32_t)((B << 16) | A);
        uint8_t tr[PNG_TRAILER_BYTES] = {0, 0, 0, 4, 'I', 'D', 'A', 'T', (uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8), (uint8_t)adler, 0, 0, 0, 0,
                                         0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
        uint32_t r = 0xffffffffu;
        for (int i = 4; i < 12; ++i) r = a.tab->crc[(r ^ tr[i]) & 0xffu] ^ (r >> 8);
        r ^= 0xffffffffu;
        tr[12] = (uint8_t)(r >> 24); tr[13] = (uint8_t)(r >> 16); tr[14] = (uint8_t)(r >> 8); tr[15] = (uint8_t)r;
        for (int i = 0; i < PNG_TRAILER_BYTES; ++i) a.out[CS_WORD_BYTES + length - PNG_TRAILER_BYTES + (unsigned long long)i] = tr[i];
    }
    __syncthreads();
    cs_scan_offsets(a, sums, (int)t);
}

// ---- the compaction: the workgroup of chunk k
__global__ void __launch_bounds__(256) png_compact_kernel(PngArgs a) { cs_compact(a, blockIdx.x, (int)threadIdx.x, 256); }

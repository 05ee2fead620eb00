// png_kernels.hip — the opt-in PNG output behind the packed outputs (include/digital_earth_png.h): the bytes pixels_pack_kernel or
// hdr_pack_kernel wrote into a buffer this stage owns become one complete, lossless PNG file behind the front the host composed.  Integer arithmetic
// only; four kernels, one after the other on the context stream:
//   png_filter_kernel    one 256-thread workgroup per row: the five candidates' costs (sum of |filtered byte as int8|) by a wave reduction and an LDS
//                        add per wave, the lowest wins (ties: the lowest type), then the winning filtered row behind its type byte into S.
//   png_deflate_kernel   one 512-thread workgroup per chunk of S.  The chunk's deflate data is the shared coder's (png_deflate.h: png_code_chunk — run
//                        scan, tokens, code lengths, canonical codes, bit packing, the stored fallback, the Adler partials), packed into an image of
//                        the whole IDAT chunk (length, type, data, CRC) in LDS: no atomics on global memory.  What is PNG's alone is here: the IDAT's
//                        length and type, CMF / FLG in the first, and the CRC-32 of the IDAT: a piece per thread through the byte
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
#include "png_deflate.h"
#include "coded_stream.h"

#define PNG_FILTER_THREADS 256
#define PNG_FILTER_ADAPTIVE 5

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

// ---- the coder of one chunk: png_deflate.h; here, the IDAT around it
__global__ void __launch_bounds__(PNG_THREADS) png_deflate_kernel(PngArgs a) {
    __shared__ PngLds s;
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    if (k >= a.count) return;
    const uint32_t base = k * (uint32_t)a.chunk_bytes;
    const uint32_t n = a.total - base < (uint32_t)a.chunk_bytes ? a.total - base : (uint32_t)a.chunk_bytes;
    const bool final_chunk = k + 1u == a.count;
    const uint8_t* c = a.filtered + base;
    // the deflate data behind the IDAT's length and type and, in the first, CMF / FLG; then the framing (the coder clears the image first)
    const uint32_t d0 = 8u + (k == 0u ? 2u : 0u);      // the block's first byte in the image
    const PngTables& T = *a.tab;
    const uint32_t end = png_code_chunk(s, T, c, n, t, d0, final_chunk);
    if (t == 0u) {
        png_put(s, 32u, 0x54414449u, 32u);      // "IDAT"
        if (k == 0u) png_put(s, 64u, 0x0178u, 16u);
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

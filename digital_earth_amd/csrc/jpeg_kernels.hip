// jpeg_kernels.hip — the opt-in JPEG output behind the display transform (include/digital_earth_jpeg.h): the planes that
// videoframe_pack_kernel wrote for {I420, BT.601, full range, centre siting, rounding} — JFIF's Y'CbCr, bit for bit — become the entropy-coded data of one
// baseline JPEG behind the framing the host wrote once.  Integer arithmetic only; four kernels, one after the other on the context stream:
//   jpeg_transform_kernel   one 256-thread workgroup = 32 blocks of 8 x 8 samples, 8 lanes per block, in scan order (MCU-major: Y0 Y1 Y2 Y3 Cb Cr; an
//                           MCU is 16 x 16 pixels).  stage: lane l of a block reads sample l of each of its 8 rows (8 lanes read 8 consecutive bytes), a
//                           sample outside the plane repeating its last column / row, and puts s = code - 128 into LDS.  rows: lane l takes row l,
//                           T'[l][u] = (sum_x M[u][x] s[l][x] + 2^9) >> 10, into LDS.  columns: lane l takes column u = l (the transposed read),
//                           F[v][l] = sum_y M[v][y] T'[y][l], the quantiser q = sign(F) ((|F| + D / 2) / D), D = Q << 18, computed as
//                           ((|F| + (Q << 17)) >> 18) / Q — the same quotient: floor(floor(a / m) / n) = floor(a / (m n)) — and the int16 into LDS at its
//                           zigzag position.  store: lane l writes coefficients 8 l .. 8 l + 7 as one 16-byte word; lane 0 writes the block's mask of
//                           non-zero coefficients (bit k = zigzag position k).  LDS rows are 9 words: the lanes of a block that read along a column
//                           touch different banks.  |T| <= 5 932 032, |T'| <= 5793, |F| + D / 2 < 2^29: int32 throughout.
//   jpeg_entropy_kernel     one THREAD per restart interval — intervals are independent by construction: the DC predictors start at 0 — walking its
//                           blocks' masks, so that only non-zero coefficients are loaded.  Bits are gathered MSB first in a 64-bit accumulator (at most
//                           7 left over + 27 new), bytes leave it with a 0x00 behind every 0xFF, gathered again into 32-bit words and stored into the
//                           interval's SLOT, whose start is 16-byte aligned; the last byte is padded with 1-bits.  The slot's length goes to len[i].
//   jpeg_scan_kernel        one workgroup: the exclusive sum of (len[i] + 2) over the intervals, the offsets and the 16-byte word in front of the stream —
//                           the coded tail every coded output shares (coded_stream.h), with 2 bytes behind every piece and no trailer.
//   jpeg_compact_kernel     one workgroup per interval: the shared compaction of its slot to its final place behind the framing, then RSTm
//                           (m = i mod 8) behind it, or EOI behind the last.
// THE WORST CASE of a slot (jpeg_tables.h: JP_BLOCK_BITS, jp_geometry).  One block: its DC costs at most 11 bits of code (the longest of K.3 / K.4) + 11 of
// magnitude (|difference| <= 2047) = 22.  Each of the 63 AC positions is paid for by exactly one symbol: a non-zero coefficient pays for itself and for the
// run in front of it with at most 16 bits of code (the longest of K.5 / K.6) + 10 of magnitude (|q| <= 1023) = 26; a ZRL pays 11 bits for 16 positions;
// EOB pays 4 for at least one.  So a block has at most 22 + 63 * 26 = 1660 bits, an interval of R MCUs ceil(6 R 1660 / 8) bytes including the padded last
// one, and twice that with a 0x00 behind every byte: slot_bytes, rounded up to 16.  A coefficient outside those ranges (the DCT's bounds say there is
// none) is not coded: the thread raises the status word instead, as does a store that would leave its slot, and the conversion ends with DE_ERR_INTERNAL.
// Every load and store is range-checked; no atomics (the status word is only ever set to the same value), no scratch, no inline assembly.
// Included into de_api.hip's translation unit behind videoframe_kernels.hip, which it reads the planes of and is otherwise untouched by.
#ifndef DE_JPEG_STANDALONE      // a host build of this file alone brings its own DE_DEV (the host check under tools/)
#include "de_kernels.h"
#endif
#include "jpeg_tables.h"
#include "coded_stream.h"

#define JP_WG_BLOCKS 32          // blocks per workgroup of the transform
#define JP_LDS_STRIDE 9          // words per staged row of 8

struct JpegArgs : CodedTail {    // the pieces are the restart intervals: count of them; front: the host's framing; extra: the marker behind each
    const uint8_t* planes;      // Y [H][W], Cb [H / 2][W / 2], Cr: rows top-down
    const JpegTables* tab;
    int16_t* coef;              // [blocks][64], zigzag order
    unsigned long long* mask;   // [blocks]
    int W, H, mcus_x, restart;
    uint32_t blocks, mcus;
};

struct JpegTile {               // the transform's LDS: 2 x 9216 + 4096 + 256 = 22 784 bytes
    int s[JP_WG_BLOCKS][8][JP_LDS_STRIDE];
    int t[JP_WG_BLOCKS][8][JP_LDS_STRIDE];
    alignas(16) int16_t q[JP_WG_BLOCKS][64];
    uint8_t nz[JP_WG_BLOCKS][8];
};

// ---- the transform, as leaves of (thread, workgroup) around three barriers
DE_DEV void jp_stage(const JpegArgs& a, JpegTile& tile, int t, uint32_t wg) {
    const int g = t >> 3, l = t & 7;
    const uint32_t blk = wg * JP_WG_BLOCKS + (uint32_t)g;
    if (wg == 0 && t == 0) *a.status = 0u;
    if (blk >= a.blocks) return;
    const uint32_t mcu = blk / 6u;
    const int b = (int)(blk - mcu * 6u);
    const int mx = (int)(mcu % (uint32_t)a.mcus_x), my = (int)(mcu / (uint32_t)a.mcus_x);
    const int CW = a.W >> 1, CH = a.H >> 1;
    const uint8_t* plane = a.planes;
    int pw = a.W, ph = a.H, x0 = mx * 16 + (b & 1) * 8, y0 = my * 16 + (b >> 1) * 8;
    if (b >= 4) {
        plane += (size_t)a.W * (size_t)a.H + (b == 5 ? (size_t)CW * (size_t)CH : 0);
        pw = CW; ph = CH; x0 = mx * 8; y0 = my * 8;
    }
    const int x = x0 + l < pw ? x0 + l : pw - 1;
    for (int j = 0; j < 8; ++j) {
        const int y = y0 + j < ph ? y0 + j : ph - 1;
        tile.s[g][j][l] = (int)plane[(size_t)y * (size_t)pw + (size_t)x] - 128;
    }
}
DE_DEV void jp_rows(const JpegArgs& a, JpegTile& tile, int t, uint32_t wg) {
    const int g = t >> 3, l = t & 7;
    if (wg * JP_WG_BLOCKS + (uint32_t)g >= a.blocks) return;
    const int32_t* M = a.tab->M;
    int s[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) s[x] = tile.s[g][l][x];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int T = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) T += M[u * 8 + x] * s[x];
        tile.t[g][l][u] = (T + 512) >> 10;
    }
}
DE_DEV void jp_columns(const JpegArgs& a, JpegTile& tile, int t, uint32_t wg) {
    const int g = t >> 3, l = t & 7;
    const uint32_t blk = wg * JP_WG_BLOCKS + (uint32_t)g;
    if (blk >= a.blocks) return;
    const int32_t* M = a.tab->M;
    const int c = (blk % 6u) >= 4u ? 1 : 0;
    int tp[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) tp[y] = tile.t[g][y][l];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        int F = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) F += M[v * 8 + y] * tp[y];
        const uint32_t Q = a.tab->Q[c][v * 8 + l];
        const uint32_t mag = (((uint32_t)(F < 0 ? -F : F) + (Q << 17)) >> 18) / Q;
        tile.q[g][a.tab->zzpos[v * 8 + l]] = (int16_t)(F < 0 ? -(int)mag : (int)mag);
    }
}
DE_DEV void jp_store(const JpegArgs& a, JpegTile& tile, int t, uint32_t wg) {
    const int g = t >> 3, l = t & 7;
    const uint32_t blk = wg * JP_WG_BLOCKS + (uint32_t)g;
    if (blk >= a.blocks) return;
    uint32_t w[4], nz = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t lo = (uint16_t)tile.q[g][8 * l + 2 * k], hi = (uint16_t)tile.q[g][8 * l + 2 * k + 1];
        w[k] = lo | (hi << 16);
        nz |= (lo ? 1u : 0u) << (2 * k) | (hi ? 1u : 0u) << (2 * k + 1);
    }
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.coef + (size_t)blk * 64 + (size_t)(8 * l));      // 16-byte aligned: the buffer is, a block is 128 bytes
    dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2]; dst[3] = w[3];
    tile.nz[g][l] = (uint8_t)nz;
}
DE_DEV void jp_mask(const JpegArgs& a, JpegTile& tile, int t, uint32_t wg) {
    const int g = t >> 3, l = t & 7;
    const uint32_t blk = wg * JP_WG_BLOCKS + (uint32_t)g;
    if (blk >= a.blocks || l != 0) return;
    unsigned long long m = 0;
    for (int k = 0; k < 8; ++k) m |= (unsigned long long)tile.nz[g][k] << (8 * k);
    a.mask[blk] = m;
}

// ---- the entropy coder of one interval
struct JpegBits {
    uint32_t* slot;             // the interval's slot, as words
    uint32_t words, at;         // its capacity in words; bytes written so far
    uint32_t word;              // the bytes of word at / 4 gathered so far
    unsigned long long acc;     // the bits not yet written, in its low `n` bits
    int n;
    uint32_t status;
};
DE_DEV void jp_byte(JpegBits& w, uint32_t byte) {
    w.word |= byte << (8 * (w.at & 3u));
    if ((w.at & 3u) == 3u) {
        if ((w.at >> 2) < w.words) w.slot[w.at >> 2] = w.word; else w.status |= CS_STATUS_OVERFLOW;
        w.word = 0;
    }
    w.at++;
}
DE_DEV void jp_put(JpegBits& w, uint32_t bits, int n) {      // n <= 27 new bits behind at most 7 old ones
    w.acc = (w.acc << n) | (unsigned long long)bits;
    w.n += n;
    while (w.n >= 8) {
        const uint32_t byte = (uint32_t)(w.acc >> (w.n - 8)) & 0xffu;
        w.n -= 8;
        jp_byte(w, byte);
        if (byte == 0xffu) jp_byte(w, 0u);
    }
    w.acc &= (1ull << w.n) - 1ull;      // what is left: fewer than 8 bits
}
DE_DEV int jp_category(int v) {      // the number of bits of |v|
    const uint32_t m = (uint32_t)(v < 0 ? -v : v);
    return m ? 32 - __builtin_clz(m) : 0;
}
// value v of category n behind the symbol's code (length << 16 | code): a negative value is coded as v - 1 in n bits
DE_DEV void jp_symbol(JpegBits& w, uint32_t entry, int v, int n) {
    const uint32_t len = entry >> 16, code = entry & 0xffffu;
    const uint32_t mag = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
    jp_put(w, (code << n) | mag, (int)len + n);
}
DE_DEV void jp_encode_interval(const JpegArgs& a, uint32_t i) {
    if (i >= a.count) return;
    JpegBits w;
    w.slot = reinterpret_cast<uint32_t*>(a.slots + (size_t)i * (size_t)a.slot_bytes);
    w.words = a.slot_bytes >> 2; w.at = 0; w.word = 0; w.acc = 0; w.n = 0; w.status = 0;
    const uint32_t first = i * (uint32_t)a.restart;
    const uint32_t last = first + (uint32_t)a.restart < a.mcus ? first + (uint32_t)a.restart : a.mcus;
    int pred_y = 0, pred_cb = 0, pred_cr = 0;
    for (uint32_t mcu = first; mcu < last; ++mcu)
        for (int b = 0; b < 6; ++b) {
            const size_t blk = (size_t)mcu * 6 + (size_t)b;
            const int c = b >= 4 ? 1 : 0;
            const unsigned long long mask = a.mask[blk];
            const int16_t* q = a.coef + blk * 64;
            const int dc = (mask & 1ull) ? (int)q[0] : 0;
            const int pred = b < 4 ? pred_y : (b == 4 ? pred_cb : pred_cr);
            const int diff = dc - pred;
            if (b < 4) pred_y = dc; else if (b == 4) pred_cb = dc; else pred_cr = dc;
            const int n = jp_category(diff);
            if (n > 11) { w.status |= CS_STATUS_RANGE; continue; }
            jp_symbol(w, a.tab->dc[c][n], diff, n);
            unsigned long long m = mask >> 1;      // bit k - 1 = zigzag position k
            int prev = 0;
            while (m) {
                const int k = __builtin_ctzll(m) + 1;
                m &= m - 1;
                int run = k - prev - 1;
                prev = k;
                const int v = (int)q[k];
                const int na = jp_category(v);
                if (na > 10 || na == 0) { w.status |= CS_STATUS_RANGE; continue; }
                for (; run >= 16; run -= 16) { const uint32_t zrl = a.tab->ac[c][0xF0]; jp_put(w, zrl & 0xffffu, (int)(zrl >> 16)); }
                jp_symbol(w, a.tab->ac[c][(run << 4) | na], v, na);
            }
            if (prev != 63) { const uint32_t eob = a.tab->ac[c][0x00]; jp_put(w, eob & 0xffffu, (int)(eob >> 16)); }
        }
    if (w.n) jp_put(w, (1u << (8 - w.n)) - 1u, 8 - w.n);      // pad with 1-bits
    const uint32_t bytes = w.at;
    while (w.at & 3u) jp_byte(w, 0u);                         // flush the last word
    if (bytes > a.slot_bytes) w.status |= CS_STATUS_OVERFLOW;
    a.len[i] = bytes <= a.slot_bytes ? bytes : 0u;
    if (w.status) *a.status = w.status;
}

// ---- the marker behind interval i, by thread 0 of the workgroup that moved it
DE_DEV void jp_marker(const JpegArgs& a, uint32_t i) {
    uint8_t* dst = a.out + CS_WORD_BYTES + a.offset[i] + a.len[i];
    dst[0] = 0xff; dst[1] = i + 1u < a.count ? (uint8_t)(0xd0u + (i & 7u)) : (uint8_t)0xd9u;
}
#ifndef DE_JPEG_STANDALONE
__global__ void __launch_bounds__(256) jpeg_transform_kernel(JpegArgs a) {
    __shared__ JpegTile tile;
    const int t = (int)threadIdx.x;
    jp_stage(a, tile, t, blockIdx.x);
    __syncthreads();
    jp_rows(a, tile, t, blockIdx.x);
    __syncthreads();
    jp_columns(a, tile, t, blockIdx.x);
    __syncthreads();
    jp_store(a, tile, t, blockIdx.x);
    __syncthreads();
    jp_mask(a, tile, t, blockIdx.x);
}
__global__ void __launch_bounds__(64) jpeg_entropy_kernel(JpegArgs a) { jp_encode_interval(a, blockIdx.x * 64u + threadIdx.x); }
__global__ void __launch_bounds__(CS_SCAN_THREADS) jpeg_scan_kernel(JpegArgs a) {
    __shared__ uint32_t sums[CS_SCAN_THREADS];
    const int t = (int)threadIdx.x;
    cs_scan_sum(a, sums, t);
    __syncthreads();
    cs_scan_total(a, sums, t);
    __syncthreads();
    cs_scan_offsets(a, sums, t);
}
__global__ void __launch_bounds__(256) jpeg_compact_kernel(JpegArgs a) {
    if (cs_compact(a, blockIdx.x, (int)threadIdx.x, 256) && threadIdx.x == 0) jp_marker(a, blockIdx.x);
}
#endif

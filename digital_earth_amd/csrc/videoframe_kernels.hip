// videoframe_kernels.hip — the opt-in video frame output behind the display transform (include/digital_earth_video.h): the displayed
// image, (W, H, 3) f32 with the pixels of a COLUMN contiguous and row 0 at the bottom, becomes the planes of one Y'CbCr 4:2:0 frame — NV12, I420,
// P010 or I010 — rows top-down, the samples of a ROW contiguous (r = H - 1 - v, x = u), planes tightly packed in one buffer.  W and H are even.
//   videoframe_pack_kernel    one 256-thread workgroup = one 32 x 32 luma tile = one 16 x 16 chroma block, in three steps around two barriers.
//     1. stage   33 x 33 cells: the tile, the column to its left and the row above it (v + 1), which the [1 2 1] taps of the LEFT and TOPLEFT sitings
//                reach; a cell outside the image reads the edge pixel (only u = -1 and v = H can occur: W and H are even, a tile starts at even u, v).
//                Cell p = t + 256 k is (column p / 33, row p % 33): a wave reads runs of 12-byte pixels along the image's contiguous columns.  Each
//                cell computes R'G'B' -> Y, Cb, Cr once; Cb and Cr go to LDS as f32, and a cell inside the tile quantises its Y code into LDS too.
//                Rows are 33 words: the column-wise writes of a 32-lane group (consecutive rows of one column, word 33 row + column) touch 32
//                different banks.  The filter's row-wise reads step two columns per lane, so a 32-lane group (two chroma rows of 16 samples) reads
//                even banks only, two lanes per bank; splitting even and odd columns would cure it and is not worth a second layout at 18 reads per thread.
//     2. filter  thread t owns chroma sample (t & 15, t >> 4) of the block: the siting's fixed dyadic filter over the staged differences, the code,
//                the clip and the quantiser, both planes, into LDS.
//     3. store   whole row segments as 32-bit words wherever the geometry proves them aligned, otherwise by sample (below).
// Alignment of the 32-bit stores (derived, not tested at run time; the buffer comes from hipMalloc, a tile starts at x0 = 32 bx, its chroma block at
// i0 = 16 bx, CW = W / 2, CH = H / 2, all offsets in bytes):
//   NV12  Y row r at r W + x0, CbCr row j at W H + j W + 2 i0: multiples of 4 for every r, j exactly when W = 0 mod 4.  Then a ragged tile holds a
//         multiple of 4 pixels: whole words of 4 Y codes, whole words of 2 CbCr pairs.  W = 2 mod 4: Y by bytes, CbCr by 16-bit pairs (every offset is even).
//   I420  Y as NV12.  Cb row j at W H + j CW + i0, Cr a further CW CH: multiples of 4 for every j exactly when CW = 0 mod 4, W = 0 mod 8; a ragged
//         tile then holds a multiple of 8 pixels, whole words of 4 chroma codes.  Otherwise the chroma planes go by bytes.
//   P010  Y row r at 2 (r W + x0): W is even, always a multiple of 4; a ragged tile holds an even number of pixels, whole words of 2 codes.  CbCr row
//         j at 2 W H + 2 (j W + 2 i0), one word per (Cb, Cr) pair: always aligned.  No narrow path.
//   I010  Y as P010.  Cb row j at 2 (W H + j CW + i0), Cr a further 2 CW CH: multiples of 4 for every j exactly when CW is even, W = 0 mod 4; a ragged
//         tile then holds an even number of chroma samples.  W = 2 mod 4 (an odd chroma stride): the chroma planes go by 16-bit words.
// A context's W is a multiple of 16 and so is every output size of the scaling stage: they always take the wide paths; de_debug_video admits any even size.
// All float work is f32 in the order the header states (no contraction: -ffp-contract=off), so the numpy restatement under tests/ gives the
// same bytes.  No atomics, no scratch; every index is range-checked before its load or store.
// Included into de_api.hip's translation unit; display_kernel and pixels_pack_kernel are untouched.
#ifndef DE_VIDEO_STANDALONE      // a host build of this file alone brings its own DE_DEV (the host check under tools/)
#include "de_kernels.h"
#endif
#include "pack.h"             // the hash, the quantiser, the clamp and the tile (PACK_TILE, PACK_LDS_STRIDE): what this pack shares with the pixel packs

#define VD_CELLS 33           // staged cells per axis: the tile, one column to its left (cell column 0 is u0 - 1), one row above it (cell row 32 is v0 + 32)
#define VD_CTILE 16
#define VD_C_STRIDE 17

struct VideoConsts {          // of the matrix, the range and the bit depth: vd_make_consts below, once per de_set_video
    float kr, kg, kb, sb, sr;
    float ys, yo, ylo, yhi;   // y = Y ys + yo, clipped to [ylo, yhi]
    float cs, co, clo, chi;   // c = C cs + co, clipped to [clo, chi]
};

struct VideoArgs {
    const float* image;     // (W, H, 3): index (u H + v) 3 + c, v = 0 at the bottom
    uint8_t* out;           // the frame: W H 3 / 2 samples of 1 or 2 bytes
    int W, H;               // both even
    int format;             // DE_VIDEO_NV12, _I420, _P010, _I010
    int siting;             // DE_VIDEO_SITING_LEFT, _CENTER, _TOPLEFT
    int mode;               // DE_PIXELS_*
    uint32_t seed, phase;   // of the dither's hash
    VideoConsts k;
};

// The constants of a setting, on the host in double, rounded to f32 (the header's list).  kg alone is two f32 operations: (kr + kb) + kg == 1.0f.
static inline VideoConsts vd_make_consts(int format, int matrix, int range) {
    static const double KR[3] = {0.2126, 0.299, 0.2627}, KB[3] = {0.0722, 0.114, 0.0593};
    const double Kr = KR[matrix], Kb = KB[matrix];
    const double k = format >= 2 ? 4.0 : 1.0, M = format >= 2 ? 1023.0 : 255.0;
    VideoConsts c;
    c.kr = (float)Kr; c.kb = (float)Kb;
    const float krb = c.kr + c.kb;
    c.kg = 1.0f - krb;
    c.sb = (float)(0.5 / (1.0 - Kb)); c.sr = (float)(0.5 / (1.0 - Kr));
    if (range == 0) {
        c.ys = (float)(219.0 * k); c.yo = (float)(16.0 * k); c.ylo = (float)(16.0 * k); c.yhi = (float)(235.0 * k);
        c.cs = (float)(224.0 * k); c.co = (float)(128.0 * k); c.clo = (float)(16.0 * k); c.chi = (float)(240.0 * k);
    } else {
        c.ys = (float)M; c.yo = 0.0f; c.ylo = 0.0f; c.yhi = (float)M;
        c.cs = (float)M; c.co = (float)(128.0 * k); c.clo = 0.0f; c.chi = (float)M;
    }
    return c;
}

struct VideoTile {       // the workgroup's LDS: 2 x 4356 + 4224 + 2176 = 15112 bytes
    float cb[VD_CELLS][PACK_LDS_STRIDE];
    float cr[VD_CELLS][PACK_LDS_STRIDE];
    uint32_t y[PACK_TILE][PACK_LDS_STRIDE];
    uint32_t c[2][VD_CTILE][VD_C_STRIDE];
};

// The codes come from pack_quantise(s, lo, hi, ...) on a clipped s; `idx` = 4 (sample index in its plane) + plane: 0 for Y, 1 for Cb, 2 for Cr.
DE_DEV float vd_clip(float v, float lo, float hi) { return v > lo ? (v < hi ? v : hi) : lo; }

// Step 1: thread t computes cells p = t + 256 k (cell column cl = p / 33 is image column u0 - 1 + cl, cell row rl = p % 33 is image row v0 + rl).
DE_DEV void vd_stage_tile(const VideoArgs& a, VideoTile& tile, int t, int bx, int by) {
    const uint32_t key = pack_key(a.seed, a.phase);
    const int u0 = bx * PACK_TILE, v0 = by * PACK_TILE;
    for (int k = 0; k < 5; ++k) {
        const int p = t + 256 * k;
        if (p >= VD_CELLS * VD_CELLS) break;
        const int cl = p / VD_CELLS, rl = p - cl * VD_CELLS;
        const int u = u0 - 1 + cl, v = v0 + rl;
        if (u < a.W && v <= a.H) {                                   // u >= -1; the cells the filter of a sample inside the image can reach
            const int us = u < 0 ? 0 : u, vs = v < a.H ? v : a.H - 1;      // the edge pixel repeated
            const float* px = pack_pixel(a.image, a.H, us, vs);
            const float R = pack_clamp01(px[0]), G = pack_clamp01(px[1]), B = pack_clamp01(px[2]);
            const float Y = ((a.k.kr * R) + (a.k.kb * B)) + (a.k.kg * G);
            tile.cb[rl][cl] = (B - Y) * a.k.sb;
            tile.cr[rl][cl] = (R - Y) * a.k.sr;
            if (cl >= 1 && rl < PACK_TILE && v < a.H) {                // inside the tile and the image: its Y code
                tile.y[rl][cl - 1] = pack_quantise(vd_clip(Y * a.k.ys + a.k.yo, a.k.ylo, a.k.yhi), a.k.ylo, a.k.yhi, a.mode, key, pack_idx(a.W, a.H, u, v));
            }
        }
    }
}

// The siting's filter of one staged difference around cell column c0 = 2 i (image column x - 1) and cell row r0 = 2 ml (the pair's bottom row; the
// top row of the pair, output row 2 j, is r0 + 1 and the row above it, output row 2 j - 1, is r0 + 2).
DE_DEV float vd_filter(const float (*c)[PACK_LDS_STRIDE], int siting, int c0, int r0) {
    if (siting == 1) {                                               // CENTER
        const float ht = c[r0 + 1][c0 + 1] + c[r0 + 1][c0 + 2], hb = c[r0][c0 + 1] + c[r0][c0 + 2];
        return (ht + hb) * 0.25f;
    }
    const float ht = (c[r0 + 1][c0] + c[r0 + 1][c0 + 2]) + 2.0f * c[r0 + 1][c0 + 1];
    const float hb = (c[r0][c0] + c[r0][c0 + 2]) + 2.0f * c[r0][c0 + 1];
    if (siting == 0) return (ht + hb) * 0.125f;                      // LEFT
    const float ha = (c[r0 + 2][c0] + c[r0 + 2][c0 + 2]) + 2.0f * c[r0 + 2][c0 + 1];
    return ((ha + hb) + 2.0f * ht) * 0.0625f;                        // TOPLEFT
}

// Step 2: thread t filters and quantises chroma sample (i = t & 15, ml = t >> 4) of the block into tile.c[plane][ml][i].
DE_DEV void vd_chroma_tile(const VideoArgs& a, VideoTile& tile, int t, int bx, int by) {
    const uint32_t key = pack_key(a.seed, a.phase);
    const int i = t & 15, ml = t >> 4;
    const int x = bx * PACK_TILE + 2 * i, vb = by * PACK_TILE + 2 * ml;
    if (x < a.W && vb < a.H) {                                       // then x + 1 < W and vb + 2 <= H: every cell read below was staged
        const uint32_t idx = pack_idx(a.W >> 1, a.H >> 1, x >> 1, vb >> 1);      // the chroma plane is (W / 2, H / 2), rows top-down like Y
        const float fb = vd_filter(tile.cb, a.siting, 2 * i, 2 * ml), fr = vd_filter(tile.cr, a.siting, 2 * i, 2 * ml);
        tile.c[0][ml][i] = pack_quantise(vd_clip(fb * a.k.cs + a.k.co, a.k.clo, a.k.chi), a.k.clo, a.k.chi, a.mode, key, idx + 1u);
        tile.c[1][ml][i] = pack_quantise(vd_clip(fr * a.k.cs + a.k.co, a.k.clo, a.k.chi), a.k.clo, a.k.chi, a.mode, key, idx + 2u);
    }
}

// Step 3: the tile's rows into the planes (the alignment of every 32-bit store: the head of this file).
DE_DEV void vd_store_tile(const VideoArgs& a, const VideoTile& tile, int t, int bx, int by) {
    const int W = a.W, H = a.H, CW = W >> 1, CH = H >> 1;
    const int u0 = bx * PACK_TILE, v0 = by * PACK_TILE;
    const bool wide16 = a.format >= 2;                               // P010, I010: two bytes per sample
    const int shift = a.format == 2 ? 6 : 0;                         // P010: the code in the high bits
    const size_t npx = (size_t)W * (size_t)H;
    // ---- Y
    if (!wide16) {
        if ((W & 3) == 0) {
            const int vl = t >> 3, d = t & 7;                        // 32 rows x 8 words of 4 codes
            const int v = v0 + vl, x = u0 + 4 * d;
            if (v < H && x + 3 < W) {
                uint32_t* row = reinterpret_cast<uint32_t*>(a.out + (size_t)(H - 1 - v) * (size_t)W);
                row[x >> 2] = tile.y[vl][4 * d] | (tile.y[vl][4 * d + 1] << 8) | (tile.y[vl][4 * d + 2] << 16) | (tile.y[vl][4 * d + 3] << 24);
            }
        } else {
            for (int k = 0; k < 4; ++k) {
                const int p = t + 256 * k;
                const int vl = p >> 5, ul = p & 31;
                const int v = v0 + vl, x = u0 + ul;
                if (v < H && x < W) a.out[(size_t)(H - 1 - v) * (size_t)W + (size_t)x] = (uint8_t)tile.y[vl][ul];
            }
        }
    } else {
        for (int k = 0; k < 2; ++k) {
            const int p = t + 256 * k;                               // 32 rows x 16 words of 2 codes
            const int vl = p >> 4, d = p & 15;
            const int v = v0 + vl, x = u0 + 2 * d;
            if (v < H && x + 1 < W) {
                uint32_t* row = reinterpret_cast<uint32_t*>(a.out + (size_t)(H - 1 - v) * (size_t)W * 2);
                row[x >> 1] = (tile.y[vl][2 * d] << shift) | ((tile.y[vl][2 * d + 1] << shift) << 16);
            }
        }
    }
    // ---- Cb, Cr
    if (a.format == 0) {                                             // NV12: [CH][CW][2] bytes behind Y
        uint8_t* base = a.out + npx;
        if ((W & 3) == 0) {
            const int ml = t >> 3, d = t & 7;                        // 16 rows x 8 words of 2 pairs
            const int vb = v0 + 2 * ml, x = u0 + 4 * d;
            if (t < 128 && vb < H && x + 3 < W) {
                const size_t j = (size_t)(CH - 1 - (vb >> 1));
                reinterpret_cast<uint32_t*>(base)[(j * (size_t)W + (size_t)x) >> 2] =
                    tile.c[0][ml][2 * d] | (tile.c[1][ml][2 * d] << 8) | (tile.c[0][ml][2 * d + 1] << 16) | (tile.c[1][ml][2 * d + 1] << 24);
            }
        } else {
            const int ml = t >> 4, i = t & 15;
            const int vb = v0 + 2 * ml, x = u0 + 2 * i;
            if (vb < H && x < W) {
                const size_t j = (size_t)(CH - 1 - (vb >> 1));
                reinterpret_cast<uint16_t*>(base)[(j * (size_t)W + (size_t)x) >> 1] = (uint16_t)(tile.c[0][ml][i] | (tile.c[1][ml][i] << 8));
            }
        }
    } else if (a.format == 1) {                                      // I420: Cb [CH][CW], then Cr, bytes behind Y
        uint8_t* base = a.out + npx;
        if ((W & 7) == 0) {
            const int plane = t >> 6, q = t & 63;                    // 2 planes x 16 rows x 4 words of 4 codes
            const int ml = q >> 2, d = q & 3;
            const int vb = v0 + 2 * ml, x = u0 + 8 * d;
            if (t < 128 && vb < H && x + 7 < W) {
                const size_t j = (size_t)(CH - 1 - (vb >> 1));
                reinterpret_cast<uint32_t*>(base)[((size_t)plane * (size_t)CW * (size_t)CH + j * (size_t)CW + (size_t)(x >> 1)) >> 2] =
                    tile.c[plane][ml][4 * d] | (tile.c[plane][ml][4 * d + 1] << 8) | (tile.c[plane][ml][4 * d + 2] << 16) | (tile.c[plane][ml][4 * d + 3] << 24);
            }
        } else {
            const int ml = t >> 4, i = t & 15;
            const int vb = v0 + 2 * ml, x = u0 + 2 * i;
            if (vb < H && x < W) {
                const size_t at = (size_t)(CH - 1 - (vb >> 1)) * (size_t)CW + (size_t)(x >> 1);
                base[at] = (uint8_t)tile.c[0][ml][i];
                base[(size_t)CW * (size_t)CH + at] = (uint8_t)tile.c[1][ml][i];
            }
        }
    } else if (a.format == 2) {                                      // P010: [CH][CW][2] 16-bit words behind Y, one 32-bit word per pair
        const int ml = t >> 4, i = t & 15;
        const int vb = v0 + 2 * ml, x = u0 + 2 * i;
        if (vb < H && x < W) {
            const size_t j = (size_t)(CH - 1 - (vb >> 1));
            reinterpret_cast<uint32_t*>(a.out + npx * 2)[(j * (size_t)W + (size_t)x) >> 1] = (tile.c[0][ml][i] << 6) | ((tile.c[1][ml][i] << 6) << 16);
        }
    } else {                                                         // I010: Cb [CH][CW], then Cr, 16-bit words behind Y
        uint8_t* base = a.out + npx * 2;
        if ((W & 3) == 0) {
            const int plane = t >> 7, q = t & 127;                   // 2 planes x 16 rows x 8 words of 2 codes
            const int ml = q >> 3, d = q & 7;
            const int vb = v0 + 2 * ml, x = u0 + 4 * d;
            if (vb < H && x + 3 < W) {
                const size_t j = (size_t)(CH - 1 - (vb >> 1));
                reinterpret_cast<uint32_t*>(base)[((size_t)plane * (size_t)CW * (size_t)CH + j * (size_t)CW + (size_t)(x >> 1)) >> 1] =
                    tile.c[plane][ml][2 * d] | (tile.c[plane][ml][2 * d + 1] << 16);
            }
        } else {
            const int ml = t >> 4, i = t & 15;
            const int vb = v0 + 2 * ml, x = u0 + 2 * i;
            if (vb < H && x < W) {
                const size_t at = (size_t)(CH - 1 - (vb >> 1)) * (size_t)CW + (size_t)(x >> 1);
                reinterpret_cast<uint16_t*>(base)[at] = (uint16_t)tile.c[0][ml][i];
                reinterpret_cast<uint16_t*>(base)[(size_t)CW * (size_t)CH + at] = (uint16_t)tile.c[1][ml][i];
            }
        }
    }
}

#ifndef DE_VIDEO_STANDALONE
__global__ void __launch_bounds__(256) videoframe_pack_kernel(VideoArgs a) {
    __shared__ VideoTile tile;
    vd_stage_tile(a, tile, (int)threadIdx.x, (int)blockIdx.x, (int)blockIdx.y);
    __syncthreads();
    vd_chroma_tile(a, tile, (int)threadIdx.x, (int)blockIdx.x, (int)blockIdx.y);
    __syncthreads();
    vd_store_tile(a, tile, (int)threadIdx.x, (int)blockIdx.x, (int)blockIdx.y);
}
#endif

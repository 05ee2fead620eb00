// hdr_pack.h — the two halves of hdr_pack_kernel (hdr_output_kernels.hip) and its arguments, apart from the transform above the kernel,
// so that a host build (tools/pixels_host_check.cpp) runs them one workgroup at a time under the sanitizers.  The noise, the quantiser, the tile walk and
// the dword-per-pixel store are pack.h's; this file owns the 10 / 16-bit staging and the RGB16 store.  The includer brings DE_DEV.
// Alignment of the dword stores (derived, not tested at run time, as in pixels_kernels.hip): W is a multiple of 16 (de_create, de_set_output_scale), a tile starts at
// x0 = 32 bx: a row starts at byte r W 4 or r W 6 and a tile's segment 128 bx or 192 bx further, all multiples of 4; the buffer comes from hipMalloc.
// W = 16 mod 32 leaves half a tile: 16 pixels = 16 or 24 whole dwords.
// No atomics, no scratch; every index is range-checked before its load or store.
#pragma once
#include "pack.h"

struct HdrPackArgs {
    const float* image;     // (W, H, 3): index (u H + v) 3 + c, v = 0 at the bottom
    void* out;              // RGB10A2: uint32 [H][W]; RGB16: uint16 [H][W][3]; row 0 at the top
    int W, H;
    int format;             // DE_HDR_PIXELS_*
    int mode;               // DE_PIXELS_*
    uint32_t seed, phase;   // of the dither's hash
};

#define HPX_PLANES 3      // the workgroup's LDS, uint32 [3][32][33].  RGB10A2: [0] holds the packed dword; RGB16: one plane per channel

// First half: thread t quantises its four cells (pack.h: column ul, row vl) of tile (bx, by) to 0 ... maxcode (1023 or 65535; s + 0.5 and maxcode - s
// are exact-or-rounded f32 as at 255).  `idx` = (r W + x) 4 + c.
DE_DEV void hdr_stage_tile(const HdrPackArgs& a, uint32_t (*tile)[PACK_TILE][PACK_LDS_STRIDE], int t, int bx, int by) {
    const uint32_t key = pack_key(a.seed, a.phase);
    const bool wide = a.format == 1;
    const float maxcode = wide ? 65535.0f : 1023.0f;
    for (int k = 0; k < 4; ++k) {
        const PackCell c = pack_cell(t + 256 * k, bx, by);
        if (c.u < a.W && c.v < a.H) {
            const float* px = pack_pixel(a.image, a.H, c.u, c.v);
            const uint32_t idx = pack_idx(a.W, a.H, c.u, c.v);
            const uint32_t r = pack_quantise01(px[0], maxcode, a.mode, key, idx), g = pack_quantise01(px[1], maxcode, a.mode, key, idx + 1u),
                           b = pack_quantise01(px[2], maxcode, a.mode, key, idx + 2u);
            if (wide) {
                tile[0][c.vl][c.ul] = r; tile[1][c.vl][c.ul] = g; tile[2][c.vl][c.ul] = b;
            } else {
                tile[0][c.vl][c.ul] = r | (g << 10) | (b << 20) | 0xc0000000u;
            }
        }
    }
}

// Second half: the tile's rows as 32-bit words.  RGB10A2: word d of staged row vl is pixel d (pack.h's store).  RGB16: dword d of a tile's row segment
// holds halfwords 2 d and 2 d + 1: channel (2 d) % 3 of pixel (2 d) / 3 and the halfword after it, which belongs to pixel (2 d + 1) / 3 — so a word
// whose second pixel is inside the row is inside the row.
DE_DEV void hdr_store_tile(const HdrPackArgs& a, const uint32_t (*tile)[PACK_TILE][PACK_LDS_STRIDE], int t, int bx, int by) {
    if (a.format != 1) {
        pack_store_dwords(static_cast<uint32_t*>(a.out), a.W, a.H, tile[0], 0u, t, bx, by);
    } else {
        const int u0 = bx * PACK_TILE;
        const size_t stride = (size_t)a.W * 3 / 2;                       // dwords per row of the output
        for (int k = 0; k < 6; ++k) {
            const int p = t + 256 * k;                                   // 0 ... 1535 = 32 rows x 48 words
            const int vl = p / 48, d = p % 48;
            const int v = by * PACK_TILE + vl, x1 = u0 + (2 * d + 1) / 3;
            if (v < a.H && x1 < a.W) {
                uint32_t* row = static_cast<uint32_t*>(a.out) + (size_t)(a.H - 1 - v) * stride;
                const int h0 = 2 * d, h1 = 2 * d + 1;
                row[(u0 * 3) / 2 + d] = tile[h0 % 3][vl][h0 / 3] | (tile[h1 % 3][vl][h1 / 3] << 16);
            }
        }
    }
}

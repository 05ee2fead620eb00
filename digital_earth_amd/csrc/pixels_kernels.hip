// pixels_kernels.hip — the opt-in 8-bit pixel output behind the display transform (include/digital_earth_pixels.h): the displayed
// image, (W, H, 3) f32 with the pixels of a COLUMN contiguous and row 0 at the bottom, becomes packed bytes out[r][x][ch] with the pixels of a ROW
// contiguous and row 0 at the top (r = H - 1 - v, x = u), 3 or 4 bytes per pixel, truncated, rounded or dithered.
//   pixels_pack_kernel   one 256-thread workgroup = one 32 x 32 pixel tile.  Each thread quantises 4 pixels read along the image's contiguous
//                        columns (a wave reads two runs of 384 contiguous bytes) and stages each as ONE dword (r | g << 8 | b << 16) in LDS,
//                        rows padded to 33 dwords: the column-wise writes and the RGBA8 store's row-wise reads touch 32 different banks per 32-lane
//                        group.  (The RGB8 store does not: a 32-lane group spans two staged rows of 24 words and reads columns 4 g + j and 4 g + j + 1,
//                        so some lanes share a bank; not worth a second layout in a kernel of about ten microseconds.)
//                        The tile is then written as whole row segments of 32-bit words: RGBA8 one dword per pixel (128 contiguous bytes per
//                        row), RGB8 24 dwords per row (96 bytes), each assembled from two neighbouring staged pixels.
// Alignment of the dword stores (derived, not tested at run time): a context's W is a multiple of 16 and its H of 8 (de_create), a tile starts at
// x0 = 32 bx, so a row starts at byte r W channels = a multiple of 16 channels and a tile's row segment 32 bx channels further — both multiples of 4
// for 3 and for 4 channels; the buffer comes from hipMalloc.  W = 16 mod 32 leaves half a tile: 16 pixels = 12 whole dwords of RGB8.
// All float work is f32 in the order the header states (no contraction: -ffp-contract=off), so a numpy restatement (tests/pixels_ref.py) gives the
// same bytes.  No atomics, no scratch; every index is range-checked before its load or store.
// Included into de_api.hip's translation unit; display_kernel is untouched.
#ifndef DE_PIXELS_STANDALONE      // a host build of this file alone brings its own DE_DEV (tools/pixels_host_check.cpp)
#include "de_kernels.h"
#endif
#include "pack.h"             // the hash, the quantiser, the tile and its walk: what this pack shares with the HDR and video packs

struct PixelsArgs {
    const float* image;     // (W, H, 3): index (u H + v) 3 + c, v = 0 at the bottom
    uint8_t* out;           // [H][W][channels], row 0 at the top
    int W, H;
    int channels;           // 3 or 4
    int mode;               // DE_PIXELS_*
    uint32_t seed, phase;   // of the dither's hash
};

// First half: thread t quantises its four cells (pack.h: column ul, row vl) of tile (bx, by) into tile[vl][ul].  `idx` = (r W + x) 4 + c.
DE_DEV void pixels_stage_tile(const PixelsArgs& a, uint32_t (*tile)[PACK_LDS_STRIDE], int t, int bx, int by) {
    const uint32_t key = pack_key(a.seed, a.phase);
    for (int k = 0; k < 4; ++k) {
        const PackCell c = pack_cell(t + 256 * k, bx, by);
        if (c.u < a.W && c.v < a.H) {
            const float* px = pack_pixel(a.image, a.H, c.u, c.v);
            const uint32_t idx = pack_idx(a.W, a.H, c.u, c.v);
            const uint32_t r = pack_quantise01(px[0], 255.0f, a.mode, key, idx), g = pack_quantise01(px[1], 255.0f, a.mode, key, idx + 1u), b = pack_quantise01(px[2], 255.0f, a.mode, key, idx + 2u);
            tile[c.vl][c.ul] = r | (g << 8) | (b << 16);
        }
    }
}

// Second half: the tile's rows as 32-bit words.  RGBA8: word d of staged row vl is pixel d (pack.h's store, alpha or-ed in).  RGB8: word d = 3 g + j
// holds bytes 4 d ... 4 d + 3 of the row segment, the upper 3 - j bytes of pixel 4 g + j and the lower j + 1 bytes of pixel 4 g + j + 1; its last byte,
// 3 u0 + 4 d + 3, is at or below the last byte of that second pixel, 3 (u0 + 4 g + j + 1) + 2, so a word whose second pixel is inside the row is inside the row.
DE_DEV void pixels_store_tile(const PixelsArgs& a, const uint32_t (*tile)[PACK_LDS_STRIDE], int t, int bx, int by) {
    if (a.channels == 4) {
        pack_store_dwords(reinterpret_cast<uint32_t*>(a.out), a.W, a.H, tile, 0xff000000u, t, bx, by);
    } else {
        const int u0 = bx * PACK_TILE;
        for (int k = 0; k < 3; ++k) {
            const int p = t + 256 * k;                                   // 0 ... 767 = 32 rows x 24 words
            const int vl = p / 24, d = p % 24;
            const int g = d / 3, j = d % 3;
            const int v = by * PACK_TILE + vl, x1 = u0 + 4 * g + j + 1;   // the word's second pixel; 4 g + j + 1 <= 31
            if (v < a.H && x1 < a.W) {
                uint32_t* row = reinterpret_cast<uint32_t*>(a.out + (size_t)(a.H - 1 - v) * (size_t)a.W * 3);
                const uint32_t lo = tile[vl][4 * g + j], hi = tile[vl][4 * g + j + 1];
                row[(u0 / 4) * 3 + d] = (lo >> (8 * j)) | (hi << (24 - 8 * j));
            }
        }
    }
}

#ifndef DE_PIXELS_STANDALONE
__global__ void __launch_bounds__(256) pixels_pack_kernel(PixelsArgs a) {
    __shared__ uint32_t tile[PACK_TILE][PACK_LDS_STRIDE];
    pixels_stage_tile(a, tile, (int)threadIdx.x, (int)blockIdx.x, (int)blockIdx.y);
    __syncthreads();
    pixels_store_tile(a, tile, (int)threadIdx.x, (int)blockIdx.x, (int)blockIdx.y);
}
#endif

// pack.h — what the packed outputs share (pixels_kernels.hip; hdr_pack.h, §17; videoframe_kernels.hip, §18): the dither's hash and key,
// the clamp, the quantiser, the 32 x 32 tile with its 33-word LDS rows, the walk that stages it along the image's contiguous columns, and the store of a
// tile whose rows are one dword per pixel.  The dither is a contract (include/digital_earth_pixels.h, include/digital_earth_video.h): it
// is stated here and nowhere else under csrc/ (tests/test_pack_shared.py).  Everything is a DE_DEV leaf of (thread, workgroup), so a kernel reads
// "half, __syncthreads(), half" and a host build (the packs' host checks under tools/) runs the halves one workgroup at a time under
// the sanitizers.  The includer brings DE_DEV; nothing else is needed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define PACK_TILE 32
#define PACK_LDS_STRIDE 33      // words per staged row: one word of padding, so that column-wise writes and row-wise reads of a 32-lane group touch 32 banks

// ---- the noise
DE_DEV uint32_t pack_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// Once per conversion: of the settings' seed and the conversion's phase.
DE_DEV uint32_t pack_key(uint32_t seed, uint32_t phase) { return pack_mix(seed + 0x9E3779B9u * phase); }
// Triangular on (-1, 1), the difference of the hash's two halves; both terms and the difference are exact.
DE_DEV float pack_tri(uint32_t key, uint32_t idx) {
    const uint32_t h = pack_mix(key ^ idx);
    return (float)(h >> 16) * 0x1p-16f - (float)(h & 0xffffu) * 0x1p-16f;
}
// A sample's index under the hash: 4 (its index in its plane of width W, row-major, rows top-down: row H - 1 - v) + channel or plane.
DE_DEV uint32_t pack_idx(int W, int H, int u, int v) { return ((uint32_t)(H - 1 - v) * (uint32_t)W + (uint32_t)u) * 4u; }

// ---- the quantiser
DE_DEV float pack_clamp01(float t) { return t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f; }      // NaN and -0.0 fail the first test
// One value s in [lo, hi] to its code: truncated, rounded, or dithered with the noise's amplitude limited by the distance to either end of the range.
// (With lo = 0, s - lo is s bit for bit: s = pack_clamp01(t) * hi is never -0.0.)
DE_DEV uint32_t pack_quantise(float s, float lo, float hi, int mode, uint32_t key, uint32_t idx) {
    if (mode == 0) return (uint32_t)(int)s;
    if (mode == 1) return (uint32_t)(int)(s + 0.5f);
    const float tri = pack_tri(key, idx);
    const float d = s - lo, e = hi - s;
    const float m = d < e ? d : e;
    const float amp = m < 1.0f ? m : 1.0f;
    return (uint32_t)(int)((s + 0.5f) + amp * tri);                  // amp <= s - lo, amp <= hi - s, |tri| < 1: within lo ... hi
}
// A value t of the displayed image to its code in 0 ... maxcode (255, 1023, 65535): the 8-bit and the HDR pack.
DE_DEV uint32_t pack_quantise01(float t, float maxcode, int mode, uint32_t key, uint32_t idx) {
    return pack_quantise(pack_clamp01(t) * maxcode, 0.0f, maxcode, mode, key, idx);
}

// ---- the tile walk
// Stage: thread t takes cells p = t + 256 k, k = 0 ... 3, of tile (bx, by): column ul = p >> 5, row vl = p & 31 — consecutive threads read consecutive
// v of one column u, along the image's contiguous columns.  The image is (W, H, 3) f32: pixel (u, v) at (u H + v) 3, v = 0 at the bottom.
struct PackCell { int ul, vl, u, v; };
DE_DEV PackCell pack_cell(int p, int bx, int by) { return PackCell{p >> 5, p & 31, bx * PACK_TILE + (p >> 5), by * PACK_TILE + (p & 31)}; }
DE_DEV const float* pack_pixel(const float* image, int H, int u, int v) { return image + ((size_t)u * (size_t)H + (size_t)v) * 3; }

// Store: a staged tile whose word [vl][d] is pixel d of its row vl, as whole row segments of one dword per pixel (128 contiguous bytes per row) into
// out[H][W], rows top-down; `or_bits` is or-ed into every word.  Thread t takes words p = t + 256 k: row vl = p >> 5, word d = p & 31.
DE_DEV void pack_store_dwords(uint32_t* out, int W, int H, const uint32_t (*tile)[PACK_LDS_STRIDE], uint32_t or_bits, int t, int bx, int by) {
    for (int k = 0; k < 4; ++k) {
        const int p = t + 256 * k;
        const int vl = p >> 5, d = p & 31;
        const int v = by * PACK_TILE + vl, x = bx * PACK_TILE + d;
        if (v < H && x < W) out[(size_t)(H - 1 - v) * (size_t)W + (size_t)x] = tile[vl][d] | or_bits;
    }
}

#ifdef __HIPCC__
// The launch grid of every pack: one 256-thread workgroup per tile.  Host code.
static inline dim3 pack_grid(int W, int H) { return dim3((unsigned)((W + PACK_TILE - 1) / PACK_TILE), (unsigned)((H + PACK_TILE - 1) / PACK_TILE)); }
#endif

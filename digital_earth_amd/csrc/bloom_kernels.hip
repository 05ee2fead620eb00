// bloom_kernels.hip — the opt-in bloom of the display path (include/digital_earth_bloom.h): energy-conserving lens glare ahead of the
// unchanged display transform.  A fraction of the light above a threshold is taken from every pixel and given back through a wide, normalised
// point-spread function built as an image pyramid.
//   bloom_down0_kernel      source pixel -> mean -> bright part -> level 1, fused: a workgroup makes 16 x 16 outputs from a 34 x 34 source tile; every
//                           source pixel is prefiltered once as it is staged into LDS
//   bloom_down_kernel       level l -> level l + 1 over float4 levels (rgb + pad), the same tiling
//   bloom_up_kernel         U_l = (1 - spread) D_l + spread up(U_{l+1})
//   bloom_composite_kernel  full resolution: out = m + intensity (up(U_1) - b), m and b recomputed (a pure function: the same bits), written [H][W][3]
// All arithmetic is f32 with + - * / min max and compares in the order DESIGN.md §12 states (no contraction: -ffp-contract=off), so a numpy float32
// restatement (tests/bloom_ref.py) is bit-exact.  No global atomics, nothing to clear between displays.  The two passes of a level down are the
// shared pyramid's (pyramid.h), the source is read as every stage reads it (display_source.h).  Included into de_api.hip's translation unit;
// display_kernel is untouched.
#include "de_kernels.h"
#include "display_source.h"
#include "pyramid.h"

#include <float.h>

#define BL_MAX_LEVELS PYR_MAX_LEVELS

// What the display launch is about to read, and the settings of the bright part.
struct BloomSrc : DisplaySrc {
    float threshold, knee, clamp;
};

// Steps 1 and 2: the mean m (display_pixel's own division) and its bright part b.  A pixel whose luminance is not in (0, FLT_MAX] — zero, negative,
// NaN, Inf — gives nothing and cannot spread.  With threshold = 0, w == 1 exactly and b == m bit for bit.
DE_DEV void bloom_bright(const BloomSrc& s, const float* px, float samples, float* m, float* b) {
    m[0] = px[0] / samples; m[1] = px[1] / samples; m[2] = px[2] / samples;
    const float Y = src_luminance(m[0], m[1], m[2]);
    if (!(Y > 0.0f && Y <= FLT_MAX)) { b[0] = 0.0f; b[1] = 0.0f; b[2] = 0.0f; return; }
    const float t = s.threshold, tk = t * s.knee;
    const float q = de_min(de_max((Y - t) + tk, 0.0f), 2.0f * tk);
    const float soft = (q * q) / (4.0f * tk + 1e-5f);
    float Yb = de_max(soft, Y - t);
    if (s.clamp > 0.0f) Yb = de_min(Yb, s.clamp);
    const float w = Yb / Y;
    b[0] = m[0] * w; b[1] = m[1] * w; b[2] = m[2] * w;
}

// Source -> the staged tile of level 0: every source pixel's bright part.  W is a multiple of 16, so a group of 4 source pixels is inside the image
// or outside it.
template <bool VEC>
DE_DEV void bloom_stage0(const BloomSrc& s, float (*src)[34][PYR_SRC_STRIDE], int t, int bx, int by) {
    const int c0 = bx * 32 - 4, r0 = by * 32 - 1;
    for (int it = t; it < 34 * (PYR_SRC_COLS / 4); it += 256) {
        const int row = it / (PYR_SRC_COLS / 4), g = it - row * (PYR_SRC_COLS / 4);
        const int j = r0 + row, i0 = c0 + 4 * g;
        if (j < 0 || j >= s.H || i0 < 0 || i0 >= s.W) continue;
        float px[12];
        src_load4<VEC>(s.hdr + ((size_t)j * s.W + i0) * 3, px);
        const float samples = src_samples(s, i0, j);
        for (int k = 0; k < 4; ++k) {
            float m[3], b[3];
            bloom_bright(s, px + 3 * k, samples, m, b);
            src[0][row][4 * g + k] = b[0]; src[1][row][4 * g + k] = b[1]; src[2][row][4 * g + k] = b[2];
        }
    }
}

// Source -> level 1.  Grid: 16 x 16 output tiles of level 1.
template <bool VEC>
__global__ void __launch_bounds__(256) bloom_down0_kernel(BloomSrc s, float4* out, int Wd, int Hd) {
    __shared__ float src[3][34][PYR_SRC_STRIDE];
    __shared__ float hb[3][34][PYR_H_STRIDE];
    const int t = (int)threadIdx.x, bx = (int)blockIdx.x, by = (int)blockIdx.y;
    bloom_stage0<VEC>(s, src, t, bx, by);
    __syncthreads();
    pyr_row_pass<3, PYR_SRC_STRIDE>(src, hb, t, bx, by, bx * 32 - 4, s.W, s.H, Wd);
    __syncthreads();
    pyr_col_pass<3>(hb, t, bx, by, s.H, Wd, Hd, out);
}

// Level l -> level l + 1.  Grid: 16 x 16 output tiles.
__global__ void __launch_bounds__(256) bloom_down_kernel(const float4* in, int Ws, int Hs, float4* out, int Wd, int Hd) {
    __shared__ float src[3][34][PYR_LVL_STRIDE];
    __shared__ float hb[3][34][PYR_H_STRIDE];
    const int t = (int)threadIdx.x, bx = (int)blockIdx.x, by = (int)blockIdx.y;
    pyr_stage_level<3>(in, Ws, Hs, src, t, bx, by);
    __syncthreads();
    pyr_row_pass<3, PYR_LVL_STRIDE>(src, hb, t, bx, by, bx * 32 - 1, Ws, Hs, Wd);
    __syncthreads();
    pyr_col_pass<3>(hb, t, bx, by, Hs, Wd, Hd, out);
}

// U_l = (1 - spread) D_l + spread up(U_{l+1}).  Grid: 16 x 16 tiles of level l (Wf, Hf); a tile needs a 10 x 10 tile of the coarse level (Wc, Hc).
struct BloomUpArgs {
    const float4* coarse;   // U_{l+1}
    const float4* fine;     // D_l
    float4* out;            // U_l
    int Wc, Hc, Wf, Hf;
    float keep, spread;     // keep = 1.0f - spread, taken in f32 on the host
};
__global__ void __launch_bounds__(256) bloom_up_kernel(BloomUpArgs a) {
    __shared__ float cs[3][10][11];
    __shared__ float hb[3][10][16];      // the next coarse row is 16 banks on: the 32 lanes of two fine rows read one row (a broadcast) or two that do not collide
    const int X0 = (int)blockIdx.x * 16, Y0 = (int)blockIdx.y * 16;
    const int c0 = (X0 >> 1) - 1, r0 = (Y0 >> 1) - 1;
    if (threadIdx.x < 100u) {
        const int row = (int)threadIdx.x / 10, col = (int)threadIdx.x - row * 10;
        const int j = r0 + row, i = c0 + col;
        if (j >= 0 && j < a.Hc && i >= 0 && i < a.Wc) {
            const float4 v = a.coarse[(size_t)j * a.Wc + i];
            cs[0][row][col] = v.x; cs[1][row][col] = v.y; cs[2][row][col] = v.z;
        }
    }
    __syncthreads();
    if (threadIdx.x < 160u) {
        const int row = (int)threadIdx.x >> 4, x = (int)threadIdx.x & 15, X = X0 + x, j = r0 + row;
        if (j >= 0 && j < a.Hc && X < a.Wf) {
            const int kn = (X >> 1) - c0, kf = pyr_far(X, a.Wc) - c0;
            for (int c = 0; c < 3; ++c) hb[c][row][x] = 0.75f * cs[c][row][kn] + 0.25f * cs[c][row][kf];
        }
    }
    __syncthreads();
    const int x = (int)threadIdx.x & 15, y = (int)threadIdx.x >> 4, X = X0 + x, Y = Y0 + y;
    if (X >= a.Wf || Y >= a.Hf) return;
    const int qn = (Y >> 1) - r0, qf = pyr_far(Y, a.Hc) - r0;
    const float4 d = a.fine[(size_t)Y * a.Wf + X];
    float4 o;
    o.x = a.keep * d.x + a.spread * (0.75f * hb[0][qn][x] + 0.25f * hb[0][qf][x]);
    o.y = a.keep * d.y + a.spread * (0.75f * hb[1][qn][x] + 0.25f * hb[1][qf][x]);
    o.z = a.keep * d.z + a.spread * (0.75f * hb[2][qn][x] + 0.25f * hb[2][qf][x]);
    o.w = 0.0f;
    a.out[(size_t)Y * a.Wf + X] = o;
}

// out = m + intensity (G - b) at full resolution, G = up(U_1).  One thread = a group of 4 pixels of a row: its glow needs 4 columns of 2 rows of U_1
// (eight 16-byte loads that neighbouring groups share through L2), its output is three float4 stores (the output buffer is the context's own).
template <bool VEC>
__global__ void __launch_bounds__(256) bloom_composite_kernel(BloomSrc s, const float4* u1, int W1, int H1, float intensity, float* out) {
    const uint32_t item = blockIdx.x * 256u + threadIdx.x, gw = (uint32_t)s.W >> 2;
    if (item >= gw * (uint32_t)s.H) return;
    const int j = (int)(item / gw), i0 = (int)(item - (uint32_t)j * gw) * 4;
    float px[12];
    src_load4<VEC>(s.hdr + ((size_t)j * s.W + i0) * 3, px);
    const float samples = src_samples(s, i0, j);
    const int cx = i0 >> 1, rn = j >> 1, rf = pyr_far(j, H1);
    float4 un[4], uf[4];      // columns cx - 1 .. cx + 2, clamped, of the near and the far row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int col = pyr_clampi(cx - 1 + k, 0, W1 - 1);
        un[k] = u1[(size_t)rn * W1 + col];
        uf[k] = u1[(size_t)rf * W1 + col];
    }
    float o[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float m[3], b[3];
        bloom_bright(s, px + 3 * k, samples, m, b);
        const int kn = (k >> 1) + 1, kf = (k & 1) ? kn + 1 : kn - 1;      // pixel i0 + k: near = cx + (k >> 1), far one to its left (even) or right (odd)
        const float gx = 0.75f * (0.75f * un[kn].x + 0.25f * un[kf].x) + 0.25f * (0.75f * uf[kn].x + 0.25f * uf[kf].x);      // horizontal first
        const float gy = 0.75f * (0.75f * un[kn].y + 0.25f * un[kf].y) + 0.25f * (0.75f * uf[kn].y + 0.25f * uf[kf].y);
        const float gz = 0.75f * (0.75f * un[kn].z + 0.25f * un[kf].z) + 0.25f * (0.75f * uf[kn].z + 0.25f * uf[kf].z);
        o[3 * k] = m[0] + intensity * (gx - b[0]);
        o[3 * k + 1] = m[1] + intensity * (gy - b[1]);
        o[3 * k + 2] = m[2] + intensity * (gz - b[2]);
    }
    float4* q = reinterpret_cast<float4*>(out + ((size_t)j * s.W + i0) * 3);
    q[0] = make_float4(o[0], o[1], o[2], o[3]); q[1] = make_float4(o[4], o[5], o[6], o[7]); q[2] = make_float4(o[8], o[9], o[10], o[11]);
}

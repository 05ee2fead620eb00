// local_exposure_kernels.hip — the opt-in local exposure of the display path (include/digital_earth_local_exposure.h): an edge-aware
// dodge and burn ahead of the unchanged display transform.  Every pixel's luminance is multiplied by a gain that depends on a smooth, edge-stopping
// BASE of log2 luminance only, so bright regions are pulled down and dark ones lifted towards the anchor while the detail inside them keeps its contrast.
//   lx_down0_kernel   source pixel -> mean -> (l w, w) -> level 1, fused: a workgroup makes 16 x 16 outputs from a 34 x 34 source tile; every source
//                     pixel's logarithm is taken once as it is staged into LDS
//   lx_down_kernel    level l -> level l + 1 over float2 levels (l w, w), the same tiling
//   lx_up_kernel      B_l from B_{l+1} by joint-bilateral upsampling: four taps of the coarser level, range weights between the levels' guides
//   lx_apply_kernel   full resolution: m, Y, l recomputed (a pure function: the same bits), B_0 from B_1 / D_1, the gain, written [H][W][3]
// All arithmetic is f32 with + - * / min max, compares and de_log / de_pow (de_math.h) in the order DESIGN.md §15 states (no contraction:
// -ffp-contract=off), so a numpy float32 restatement (tests/local_exposure_ref.py) with the same two functions injected is bit-exact.  No global
// atomics, nothing to clear between displays.  Every kernel is its phases around its barriers, each a function of (thread, workgroup): a host build
// of this file alone (tools/local_exposure_host_check.cpp) runs them one workgroup at a time under the sanitizers.  Included into de_api.hip's
// translation unit; display_kernel is untouched.
#ifndef DE_LX_STANDALONE      // a host build of this file alone brings its own DE_DEV, vector types, de_math.h and FrameConsts
#include "de_kernels.h"
#endif

#include "display_source.h"
#include "pyramid.h"

#include <float.h>

#define LX_MAX_LEVELS PYR_MAX_LEVELS

// Step 1: the mean m (display_pixel's own division), its luminance and l = log2 Y.  Valid: 2^-24 <= Y <= FLT_MAX (the meter's lower bound); black
// space, negatives, NaN and Inf are not, weigh nothing anywhere and leave the stage as m.
DE_DEV bool lx_pixel(const float* px, float samples, float* m, float* l) {
    m[0] = px[0] / samples; m[1] = px[1] / samples; m[2] = px[2] / samples;
    const float Y = src_luminance(m[0], m[1], m[2]);
    if (!(Y >= 0x1p-24f && Y <= FLT_MAX)) { *l = 0.0f; return false; }
    *l = de_log(Y) * DE_LOG2E;
    return true;
}

// Source -> the staged tile of level 0: (l, 1) for a valid pixel, (0, 0) otherwise.  W is a multiple of 16, so a group of 4 source pixels is inside
// the image or outside it.
template <bool VEC>
DE_DEV void lx_stage0(const DisplaySrc& s, float (*src)[34][PYR_SRC_STRIDE], int t, int bx, int by) {
    const int c0 = bx * 32 - 4, r0 = by * 32 - 1;
    for (int it = t; it < 34 * (PYR_SRC_COLS / 4); it += 256) {
        const int row = it / (PYR_SRC_COLS / 4), g = it - row * (PYR_SRC_COLS / 4);
        const int j = r0 + row, i0 = c0 + 4 * g;
        if (j < 0 || j >= s.H || i0 < 0 || i0 >= s.W) continue;
        float px[12];
        src_load4<VEC>(s.hdr + ((size_t)j * s.W + i0) * 3, px);
        const float samples = src_samples(s, i0, j);
        for (int k = 0; k < 4; ++k) {
            float m[3], l;
            const bool valid = lx_pixel(px + 3 * k, samples, m, &l);
            src[0][row][4 * g + k] = l; src[1][row][4 * g + k] = valid ? 1.0f : 0.0f;
        }
    }
}

// ---- the base, coarse to fine (one level down is the shared pyramid's, pyramid.h: §12's "Down" on both components)
// One entry of the coarser level as a tap: does it count (its weight is positive), its guide D.x / D.y and its base (the guide itself on the top level,
// whose bases are not stored: b == null).  An entry that does not count is not divided and its base is not read.
struct LxTap { float g, b; bool on; };
DE_DEV LxTap lx_read_tap(const float2* d, const float* b, size_t idx) {
    LxTap tp;
    const float2 v = d[idx];
    tp.on = v.y > 0.0f; tp.g = 0.0f; tp.b = 0.0f;
    if (tp.on) { tp.g = v.x / v.y; tp.b = b ? b[idx] : tp.g; }
    return tp;
}
DE_DEV void lx_add_tap(float k, const LxTap& tp, float guide, float inv_sigma, float* num, float* den) {
    if (!tp.on) return;
    const float a = (guide - tp.g) * inv_sigma;
    const float r = 1.0f / (1.0f + a * a);
    const float w = k * r;
    *num = *num + w * tp.b; *den = *den + w;
}
// B(p) from the four taps in the order (near, near), (far, near), (near, far), (far, far), x first.  A pixel with a positive weight always has a
// counting (near, near) tap: the pixel itself lies inside that entry's 4 x 4 footprint with the weight 0.375 x 0.375, and no weight is negative.  So
// den >= 0.5625 / (1 + a^2) > 0.
DE_DEV float lx_blend(const LxTap& nn, const LxTap& fn, const LxTap& nf, const LxTap& ff, float guide, float inv_sigma) {
    float num = 0.0f, den = 0.0f;
    lx_add_tap(0.75f * 0.75f, nn, guide, inv_sigma, &num, &den);
    lx_add_tap(0.25f * 0.75f, fn, guide, inv_sigma, &num, &den);
    lx_add_tap(0.75f * 0.25f, nf, guide, inv_sigma, &num, &den);
    lx_add_tap(0.25f * 0.25f, ff, guide, inv_sigma, &num, &den);
    return num / den;
}

struct LxUpArgs {
    const float2* fine;       // D_l
    const float2* coarse;     // D_{l+1}
    const float* coarse_b;    // B_{l+1}, or null on the top level: B_L is the level's guide
    float* out;               // B_l
    int Wc, Hc, Wf, Hf;
    float inv_sigma;          // 1.0f / sigma, taken in f32 on the host
};
// One entry of level l.  The levels below the first are a few thousand entries: plain loads through L2, no staging.
DE_DEV void lx_up_item(const LxUpArgs& a, uint32_t item) {
    if (item >= (uint32_t)a.Wf * (uint32_t)a.Hf) return;
    const int Y = (int)(item / (uint32_t)a.Wf), X = (int)(item - (uint32_t)Y * (uint32_t)a.Wf);
    const float2 d = a.fine[item];
    if (!(d.y > 0.0f)) { a.out[item] = 0.0f; return; }      // never read: every reader tests the weight first
    const float guide = d.x / d.y;
    const int xn = X >> 1, xf = pyr_far(X, a.Wc), yn = Y >> 1, yf = pyr_far(Y, a.Hc);
    const LxTap nn = lx_read_tap(a.coarse, a.coarse_b, (size_t)yn * a.Wc + xn), fn = lx_read_tap(a.coarse, a.coarse_b, (size_t)yn * a.Wc + xf);
    const LxTap nf = lx_read_tap(a.coarse, a.coarse_b, (size_t)yf * a.Wc + xn), ff = lx_read_tap(a.coarse, a.coarse_b, (size_t)yf * a.Wc + xf);
    a.out[item] = lx_blend(nn, fn, nf, ff, guide, a.inv_sigma);
}

struct LxApplyArgs {
    DisplaySrc s;
    const float2* d1;         // D_1
    const float* b1;          // B_1, or null when the pyramid has one level
    int W1, H1;
    const FrameConsts* fc;    // what the display about to run reads: its exposure_scale sets the anchor
    float highlights, shadows, inv_sigma, max_ev, key;
    float* out;               // [H][W][3], the context's own: 16-byte aligned
};
// One group of 4 pixels of a row: its base needs 4 columns of 2 rows of level 1 (eight taps that neighbouring groups share through L2), its output is
// three float4 stores.
template <bool VEC>
DE_DEV void lx_apply_item(const LxApplyArgs& a, uint32_t item) {
    const DisplaySrc& s = a.s;
    const uint32_t gw = (uint32_t)s.W >> 2;
    if (item >= gw * (uint32_t)s.H) return;
    const int j = (int)(item / gw), i0 = (int)(item - (uint32_t)j * gw) * 4;
    float px[12];
    src_load4<VEC>(s.hdr + ((size_t)j * s.W + i0) * 3, px);
    const float samples = src_samples(s, i0, j);
    const int cx = i0 >> 1, rn = j >> 1, rf = pyr_far(j, a.H1);
    LxTap tn[4], tf[4];      // columns cx - 1 .. cx + 2, clamped, of the near and the far row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int col = pyr_clampi(cx - 1 + k, 0, a.W1 - 1);
        tn[k] = lx_read_tap(a.d1, a.b1, (size_t)rn * a.W1 + col);
        tf[k] = lx_read_tap(a.d1, a.b1, (size_t)rf * a.W1 + col);
    }
    const float mid = de_log(a.key / a.fc->exposure_scale) * DE_LOG2E;      // the scene luminance the display maps to the key, in stops
    float o[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float m[3], l;
        const bool valid = lx_pixel(px + 3 * k, samples, m, &l);
        float g = 1.0f;
        if (valid) {
            const int kn = (k >> 1) + 1, kf = (k & 1) ? kn + 1 : kn - 1;      // pixel i0 + k: near = cx + (k >> 1), far one to its left (even) or right (odd)
            const float base = lx_blend(tn[kn], tn[kf], tf[kn], tf[kf], l, a.inv_sigma);
            const float strength = base > mid ? a.highlights : a.shadows;
            const float ev = de_min(de_max(-(strength * (base - mid)), -a.max_ev), a.max_ev);
            if (ev != 0.0f) g = de_pow(2.0f, ev);
            o[3 * k] = m[0] * g; o[3 * k + 1] = m[1] * g; o[3 * k + 2] = m[2] * g;
        } else {
            o[3 * k] = m[0]; o[3 * k + 1] = m[1]; o[3 * k + 2] = m[2];
        }
    }
    float4* q = reinterpret_cast<float4*>(a.out + ((size_t)j * s.W + i0) * 3);
    q[0] = make_float4(o[0], o[1], o[2], o[3]); q[1] = make_float4(o[4], o[5], o[6], o[7]); q[2] = make_float4(o[8], o[9], o[10], o[11]);
}

#ifndef DE_LX_STANDALONE
// Source -> level 1.  Grid: 16 x 16 output tiles of level 1.
template <bool VEC>
__global__ void __launch_bounds__(256) lx_down0_kernel(DisplaySrc s, float2* out, int Wd, int Hd) {
    __shared__ float src[2][34][PYR_SRC_STRIDE];
    __shared__ float hb[2][34][PYR_H_STRIDE];
    const int t = (int)threadIdx.x, bx = (int)blockIdx.x, by = (int)blockIdx.y;
    lx_stage0<VEC>(s, src, t, bx, by);
    __syncthreads();
    pyr_row_pass<2, PYR_SRC_STRIDE>(src, hb, t, bx, by, bx * 32 - 4, s.W, s.H, Wd);
    __syncthreads();
    pyr_col_pass<2>(hb, t, bx, by, s.H, Wd, Hd, out);
}

// Level l -> level l + 1.  Grid: 16 x 16 output tiles.
__global__ void __launch_bounds__(256) lx_down_kernel(const float2* in, int Ws, int Hs, float2* out, int Wd, int Hd) {
    __shared__ float src[2][34][PYR_LVL_STRIDE];
    __shared__ float hb[2][34][PYR_H_STRIDE];
    const int t = (int)threadIdx.x, bx = (int)blockIdx.x, by = (int)blockIdx.y;
    pyr_stage_level<2>(in, Ws, Hs, src, t, bx, by);
    __syncthreads();
    pyr_row_pass<2, PYR_LVL_STRIDE>(src, hb, t, bx, by, bx * 32 - 1, Ws, Hs, Wd);
    __syncthreads();
    pyr_col_pass<2>(hb, t, bx, by, Hs, Wd, Hd, out);
}

// B_l.  Grid: one thread per entry of level l.
__global__ void __launch_bounds__(256) lx_up_kernel(LxUpArgs a) { lx_up_item(a, blockIdx.x * 256u + threadIdx.x); }

// Full resolution.  Grid: one thread per group of 4 pixels.
template <bool VEC>
__global__ void __launch_bounds__(256) lx_apply_kernel(LxApplyArgs a) { lx_apply_item<VEC>(a, blockIdx.x * 256u + threadIdx.x); }
#endif

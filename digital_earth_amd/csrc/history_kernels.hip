// history_kernels.hip — the opt-in history reprojection of the display path (include/digital_earth_history.h): the picture survives a
// camera move.  Ahead of the unchanged display transform, every pixel of the frame's mean finds where its world point was in the previously
// displayed picture (the history: HDR mean + weight in samples, first-hit land distance, camera) and is blended with it by sample count.
//   history_camera_kernel   the camera basis of a de_params, setup_kernel's IEEE expression (de_debug_history: no FrameConsts of its own)
//   history_blend_kernel    one thread per pixel, 16 x 16 pixels per workgroup: mean, world point, projection into the history's camera, four
//                           unclamped bilinear taps (a float4 + an f32 each) with the surface test, blend; writes the mean the display reads
//                           ([H][W][3]) and the next history candidate (float4 + f32 per pixel, the camera by one thread)
// All arithmetic is f32 with + - * / sqrt floor and compares in the order DESIGN.md §13 states (no contraction: -ffp-contract=off; the IEEE
// normalisation, not the contract-2 one), so a numpy float32 restatement (tests/history_ref.py) is bit-exact.  No atomics, no LDS, nothing to clear
// between displays.  Neighbouring pixels reproject to neighbouring taps: a wave's 4 x 16 pixels gather from a few rows of the history.
// Included into de_api.hip's translation unit; display_kernel and the render kernels are untouched.
#ifndef DE_HISTORY_STANDALONE      // a host build of this file alone brings its own vec3 / FrameConsts / DE_DEV (tools/history_host_check.cpp)
#include "de_kernels.h"
#endif

#include "display_source.h"

#include <float.h>

// The camera of a displayed picture: what FrameConsts holds of it.
struct HistoryCam {
    vec3 cam_pos, d, du, dv;
    float fov, aspect_ratio, aspect_scale;
};

struct HistoryArgs {
    DisplaySrc s;                 // what the display launch is about to read; (s.W, s.H) is the size of every array here
    const int32_t* n_tile;        // the pixel's sample count n: its tile's [H/8][W/8] (an adaptive frame), ...
    const int32_t* n_pixel;       // ... its own [H][W] (de_debug_history), ...
    int n_frame;                  // ... or the frame's
    const float* dist;            // [H][W] DenoiseGuides::dist of the current camera
    const FrameConsts* fc;        // the current camera
    const float4* hist_c;         // [H][W] (rgb of the displayed mean, weight in samples); null: no history yet
    const float* hist_d;          // [H][W] its land distance, 0 where no ray hit land
    const HistoryCam* hist_cam;
    float* out;                   // [H][W][3]: what the display reads with samples = 1
    float4* cand_c;               // [H][W] (out, Wout): the next history
    float* cand_d;                // [H][W] a copy of dist (the guides are recomputed after the move)
    HistoryCam* cand_cam;
    float max_history, depth_tolerance;
};

DE_DEV bool history_finite3(float x, float y, float z) { return __builtin_fabsf(x) <= FLT_MAX && __builtin_fabsf(y) <= FLT_MAX && __builtin_fabsf(z) <= FLT_MAX; }

// One bilinear tap (step 5): its weight b and its weighted history weight and colour, or zeros when it is not valid.  The taps are not clamped.
struct HistoryTap { float b, w, c0, c1, c2; };
DE_DEV HistoryTap history_tap(const HistoryArgs& a, int xi, int yi, float b, bool land, float r, float tol) {
    HistoryTap t = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (xi < 0 || xi >= a.s.W || yi < 0 || yi >= a.s.H) return t;
    const size_t tp = (size_t)yi * a.s.W + xi;
    const float4 c = a.hist_c[tp];
    const float hd = a.hist_d[tp];
    const bool surface = land ? (hd > 0.0f && __builtin_fabsf(hd - r) <= tol) : hd == 0.0f;
    if (!(c.w > 0.0f && history_finite3(c.x, c.y, c.z) && surface)) return t;
    t.b = b; t.w = b * c.w;
    t.c0 = b * c.x; t.c1 = b * c.y; t.c2 = b * c.z;
    return t;
}

// Steps 2 - 6 of DESIGN.md §13 for pixel (u, v) whose distance guide is t: the reprojected history h and its weight w.  false: no history.
DE_DEV bool history_reproject(const HistoryArgs& a, int u, int v, float t, float* h, float* w) {
    const FrameConsts& fc = *a.fc;
    const HistoryCam& hc = *a.hist_cam;
    const float Hf = (float)a.s.H;
    // guide_kernel's expression at the pixel centre
    const float fu = (2.0f * fc.fov * ((float)u + 0.5f) / Hf - fc.fov * fc.aspect_ratio - 1e-5f) * fc.aspect_scale;
    const float fv = 2.0f * fc.fov * ((float)v + 0.5f) / Hf - fc.fov - 1e-5f;
    const vec3 dir = normalized_ieee(fc.d + fu * fc.du + fv * fc.dv);
    const bool land = t > 0.0f;
    // the camera's step first: it is small and near-exact, and dir * t is rounded relative to itself.  (cam + dir * t) - cam_h would round the world
    // point at planet scale (0.25 - 0.5 m) and leave that absolute error in q however short the ray is.
    const vec3 step = fc.cam_pos - hc.cam_pos;
    vec3 q;
    if (land) {
        q = step + dir * t;
    } else {
        const float s = -dot(fc.cam_pos, dir);            // the planet is centred at the origin: the tangent point, where the limb's glow sits
        q = s > 0.0f ? step + dir * s : dir;              // behind the camera: the pixel is at infinity, only its direction reprojects
    }
    const float z = dot(q, hc.d);
    if (!(z > 0.0f)) return false;
    const float gu = dot(q, hc.du) / z, gv = dot(q, hc.dv) / z;
    // guide_kernel's pixel -> (fu, fv) inverted with the history's camera, centre convention: pixel i has its centre at xo = i
    const float xo = ((gu / hc.aspect_scale + 1e-5f) + hc.fov * hc.aspect_ratio) * Hf / (2.0f * hc.fov) - 0.5f;
    const float yo = ((gv + 1e-5f) + hc.fov) * Hf / (2.0f * hc.fov) - 0.5f;
    // no tap of (floor, floor + 1) inside the image (or a NaN): nothing to read, and nothing to convert to an integer
    if (!(xo >= -1.0f && xo < (float)a.s.W && yo >= -1.0f && yo < Hf)) return false;
    const float fx = __builtin_floorf(xo), fy = __builtin_floorf(yo);
    const float bx = xo - fx, by = yo - fy;
    const int x0 = (int)fx, y0 = (int)fy;
    const float r = de_sqrt(dot(q, q));
    const float tol = a.depth_tolerance * r;
    // an invalid tap gives +0 to every sum; the two taps of a row first, then the two rows
    const float ax = 1.0f - bx, ay = 1.0f - by;
    const HistoryTap t00 = history_tap(a, x0, y0, ax * ay, land, r, tol), t10 = history_tap(a, x0 + 1, y0, bx * ay, land, r, tol);
    const HistoryTap t01 = history_tap(a, x0, y0 + 1, ax * by, land, r, tol), t11 = history_tap(a, x0 + 1, y0 + 1, bx * by, land, r, tol);
    const float B = (t00.b + t10.b) + (t01.b + t11.b), Ws = (t00.w + t10.w) + (t01.w + t11.w);
    const float h0 = (t00.c0 + t10.c0) + (t01.c0 + t11.c0), h1 = (t00.c1 + t10.c1) + (t01.c1 + t11.c1), h2 = (t00.c2 + t10.c2) + (t01.c2 + t11.c2);
    if (!(B > 0.0f)) return false;
    h[0] = h0 / B; h[1] = h1 / B; h[2] = h2 / B;
    const float wm = Ws / B;
    *w = (wm < a.max_history ? wm : a.max_history) * B;      // a pixel that lost taps at a depth edge trusts its history less
    return true;
}

// Steps 1 and 7, the display's mean and the next history candidate.
DE_DEV void history_pixel(const HistoryArgs& a, int u, int v) {
    const size_t p = (size_t)v * a.s.W + u;
    const int tile = (v >> 3) * (a.s.W >> 3) + (u >> 3);
    const float samples = src_samples(a.s, u, v);      // display_pixel's own sample count and division
    const float* px = a.s.hdr + p * 3;
    const float m0 = px[0] / samples, m1 = px[1] / samples, m2 = px[2] / samples;
    const int n = a.n_pixel ? a.n_pixel[p] : (a.n_tile ? a.n_tile[tile] : a.n_frame);
    const float nf = (float)n;
    const float t = a.dist[p];
    float h[3] = {0.0f, 0.0f, 0.0f}, w = 0.0f;
    const bool have = a.hist_c != nullptr && history_reproject(a, u, v, t, h, &w);
    float o0 = m0, o1 = m1, o2 = m2, wout = nf;
    if (have) {
        if (n == 0) {                // the reprojected old picture is on screen before the first new sample
            o0 = h[0]; o1 = h[1]; o2 = h[2]; wout = w;
        } else {
            wout = nf + w;
            o0 = (m0 * nf + h[0] * w) / wout; o1 = (m1 * nf + h[1] * w) / wout; o2 = (m2 * nf + h[2] * w) / wout;
        }
    }
    float* o = a.out + p * 3;
    o[0] = o0; o[1] = o1; o[2] = o2;
    a.cand_c[p] = make_float4(o0, o1, o2, wout);
    a.cand_d[p] = t;
}

// Grid: 16 x 16 pixel tiles.
__global__ void __launch_bounds__(256) history_blend_kernel(HistoryArgs a) {
    const int u = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), v = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (blockIdx.x == 0u && blockIdx.y == 0u && threadIdx.x == 0u) {
        const FrameConsts& fc = *a.fc;
        HistoryCam* k = a.cand_cam;
        k->cam_pos = fc.cam_pos; k->d = fc.d; k->du = fc.du; k->dv = fc.dv;
        k->fov = fc.fov; k->aspect_ratio = fc.aspect_ratio; k->aspect_scale = fc.aspect_scale;
    }
    if (u >= a.s.W || v >= a.s.H) return;
    history_pixel(a, u, v);
}

// The camera fields of FrameConsts from a de_params, in setup_kernel's expression; either output may be null.  One thread.
__global__ void history_camera_kernel(de_params p, int W, int H, FrameConsts* fc, HistoryCam* hc) {
    HistoryCam k;
    k.cam_pos = v3(p.camera_pos[0], p.camera_pos[1], p.camera_pos[2]);
    const vec3 look_at = v3(p.look_at[0], p.look_at[1], p.look_at[2]);
    const vec3 up = v3(p.up[0], p.up[1], p.up[2]);
    k.d = normalized_ieee(look_at - k.cam_pos);
    k.du = normalized_ieee(cross(k.d, up));
    k.dv = normalized_ieee(cross(k.du, k.d));
    k.fov = p.fov;
    k.aspect_ratio = (float)((double)W / (double)H);
    k.aspect_scale = p.aspect_scale;
    if (hc) *hc = k;
    if (fc) {
        fc->cam_pos = k.cam_pos; fc->d = k.d; fc->du = k.du; fc->dv = k.dv;
        fc->fov = k.fov; fc->aspect_ratio = k.aspect_ratio; fc->aspect_scale = k.aspect_scale;
    }
}

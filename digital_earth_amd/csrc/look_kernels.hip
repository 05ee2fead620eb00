// look_kernels.hip — the opt-in look LUTs behind the display transform (include/digital_earth_look.h): every pixel of the displayed
// image, n x 3 f32, goes through a 1D table, a 3D table or both, is mixed with itself by `strength` and clamped to [0, 1], in place.  The stage is
// pointwise: no pixel reads what another wrote, so the image is its own output.
//   look_apply_kernel    thread j < n / 4 owns pixels 4 j ... 4 j + 3: three 16-byte loads (the 48 bytes of a thread are contiguous, the 3 KB of a wave
//                        too), four pixels, three 16-byte stores.  The image comes from hipMalloc and a context's W is a multiple of 16, so the
//                        float4 view is aligned and a context's image has no tail.  The n % 4 pixels left over (de_debug_look's arbitrary n) are
//                        taken one each, by floats, by the threads n / 4 ... n / 4 + n % 4 - 1: at most three lanes of the last wave.
// The 3D table lies on the device as one float4 per lattice point (w = 0): a gather is one 16-byte load, four of them per pixel for the
// tetrahedral split and eight for the trilinear mix.  A 33^3 table is 0.6 MB and a 65^3 table 4.4 MB: resident in L2 beside the 24 B / pixel image
// stream.  No LDS copy: profiles/look.md has the figures behind that.  The 1D table is read as it was given, [N][3] floats, two 4-byte loads per channel.
// All float work is f32 in the order the header states (no contraction: -ffp-contract=off), so the numpy restatement under tests/ gives the same
// bits.  No atomics, no LDS, no scratch; every index is clamped into its table before the load (lk_coord) and every thread is range-checked.
// Included into de_api.hip's translation unit; display_kernel, the scaler and the pack kernels are untouched.
#ifndef DE_LOOK_STANDALONE      // a host build of this file alone brings its own DE_DEV and float4 (the host check under tools/)
#include "de_kernels.h"
#endif

struct LookAxis { float lo, k; };      // of one channel of one table: t = (x - lo) * k

struct LookArgs {
    float* image;             // n x 3 f32, in place
    uint64_t n;               // pixels
    const float* t1;          // [n1][3], or null
    const float4* t3;         // [n3][n3][n3] (b, g, r: red fastest), or null
    int n1, n3;               // 0: no such table
    int tetrahedral;
    float strength;
    LookAxis a1[3], a3[3];
};

// The header's k, on the host in double from the f32 ends, rounded once.
static inline float lk_scale(int N, float lo, float hi) { return (float)((double)(N - 1) / ((double)hi - (double)lo)); }

// The cell and the fraction of x along one axis of a table of edge N: 0 <= *i <= N - 2, 0 <= *f <= 1.
DE_DEV void lk_coord(float x, LookAxis a, int N, int* i, float* f) {
    const float top = (float)(N - 1);
    float t = (x - a.lo) * a.k;
    t = t > 0.0f ? (t < top ? t : top) : 0.0f;      // NaN fails the first test
    const int c = (int)t;
    *i = c < N - 2 ? c : N - 2;
    *f = t - (float)*i;
}

DE_DEV float lk_mix(float a, float b, float f) {
    const float p = a * (1.0f - f), q = b * f;
    return p + q;
}

DE_DEV void lk_table_1d(const LookArgs& a, float* v) {
    for (int c = 0; c < 3; ++c) {
        int i; float f;
        lk_coord(v[c], a.a1[c], a.n1, &i, &f);
        v[c] = lk_mix(a.t1[(size_t)i * 3 + c], a.t1[(size_t)(i + 1) * 3 + c], f);
    }
}

DE_DEV void lk_table_3d(const LookArgs& a, float* v) {
    const int N = a.n3;
    int ir, ig, ib; float fr, fg, fb;
    lk_coord(v[0], a.a3[0], N, &ir, &fr);
    lk_coord(v[1], a.a3[1], N, &ig, &fg);
    lk_coord(v[2], a.a3[2], N, &ib, &fb);
    const float4* p = a.t3 + ((size_t)ib * N + ig) * N + ir;      // c000; ir, ig, ib <= N - 2: every neighbour below is inside the table
    const int sr = 1, sg = N, sb = N * N;
    if (a.tetrahedral) {
        // The six-way branch of the header as selects: `hi`, `mid`, `lo` are the fractions in the branch's order, s1 the step to its second vertex and
        // s1 + s2 the step to its third.
        float hi, mid, lo; int s1, s2;
        if (fr >= fg) {
            if (fg >= fb)      { hi = fr; mid = fg; lo = fb; s1 = sr; s2 = sg; }
            else if (fr >= fb) { hi = fr; mid = fb; lo = fg; s1 = sr; s2 = sb; }
            else               { hi = fb; mid = fr; lo = fg; s1 = sb; s2 = sr; }
        } else {
            if (fb >= fg)      { hi = fb; mid = fg; lo = fr; s1 = sb; s2 = sg; }
            else if (fb >= fr) { hi = fg; mid = fb; lo = fr; s1 = sg; s2 = sb; }
            else               { hi = fg; mid = fr; lo = fb; s1 = sg; s2 = sr; }
        }
        const float4 c0 = p[0], c1 = p[s1], c2 = p[s1 + s2], c3 = p[sr + sg + sb];
        const float w0 = 1.0f - hi, w1 = hi - mid, w2 = mid - lo, w3 = lo;
        v[0] = ((w0 * c0.x + w1 * c1.x) + w2 * c2.x) + w3 * c3.x;
        v[1] = ((w0 * c0.y + w1 * c1.y) + w2 * c2.y) + w3 * c3.y;
        v[2] = ((w0 * c0.z + w1 * c1.z) + w2 * c2.z) + w3 * c3.z;
    } else {
        const float4 c000 = p[0], c100 = p[sr], c010 = p[sg], c110 = p[sg + sr];
        const float4 c001 = p[sb], c101 = p[sb + sr], c011 = p[sb + sg], c111 = p[sb + sg + sr];
        v[0] = lk_mix(lk_mix(lk_mix(c000.x, c100.x, fr), lk_mix(c010.x, c110.x, fr), fg), lk_mix(lk_mix(c001.x, c101.x, fr), lk_mix(c011.x, c111.x, fr), fg), fb);
        v[1] = lk_mix(lk_mix(lk_mix(c000.y, c100.y, fr), lk_mix(c010.y, c110.y, fr), fg), lk_mix(lk_mix(c001.y, c101.y, fr), lk_mix(c011.y, c111.y, fr), fg), fb);
        v[2] = lk_mix(lk_mix(lk_mix(c000.z, c100.z, fr), lk_mix(c010.z, c110.z, fr), fg), lk_mix(lk_mix(c001.z, c101.z, fr), lk_mix(c011.z, c111.z, fr), fg), fb);
    }
}

// One pixel, in place: the 1D table, the 3D table on its result, the mix with the original by `strength`, the display's clamp.
DE_DEV void lk_pixel(const LookArgs& a, float* px) {
    float y[3] = {px[0], px[1], px[2]};
    if (a.n1) lk_table_1d(a, y);
    if (a.n3) lk_table_3d(a, y);
    const float s = a.strength, keep = 1.0f - s;
    for (int c = 0; c < 3; ++c) {
        const float p = px[c] * keep, q = y[c] * s;
        const float o = p + q;
        px[c] = o > 0.0f ? (o < 1.0f ? o : 1.0f) : 0.0f;
    }
}

// Thread j of the launch: four pixels by float4, or one pixel of the tail, or nothing.
DE_DEV void lk_thread(const LookArgs& a, uint64_t j) {
    const uint64_t groups = a.n >> 2;
    if (j < groups) {
        float4* q = reinterpret_cast<float4*>(a.image) + j * 3;
        const float4 v0 = q[0], v1 = q[1], v2 = q[2];
        float px[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
        for (int k = 0; k < 4; ++k) lk_pixel(a, px + 3 * k);
        float4 o0, o1, o2;
        o0.x = px[0]; o0.y = px[1]; o0.z = px[2]; o0.w = px[3];
        o1.x = px[4]; o1.y = px[5]; o1.z = px[6]; o1.w = px[7];
        o2.x = px[8]; o2.y = px[9]; o2.z = px[10]; o2.w = px[11];
        q[0] = o0; q[1] = o1; q[2] = o2;
    } else if (j < groups + (a.n & 3u)) {
        float* q = a.image + ((groups << 2) + (j - groups)) * 3;
        float px[3] = {q[0], q[1], q[2]};
        lk_pixel(a, px);
        q[0] = px[0]; q[1] = px[1]; q[2] = px[2];
    }
}
static inline uint64_t lk_threads(uint64_t n) { return (n >> 2) + (n & 3u); }

#ifndef DE_LOOK_STANDALONE
__global__ void __launch_bounds__(256) look_apply_kernel(LookArgs a) {
    lk_thread(a, (uint64_t)blockIdx.x * 256u + threadIdx.x);
}
#endif

// denoise_kernels.hip — the opt-in denoiser of the display path (include/digital_earth_denoise.h): an SVGF-style edge-avoiding
// a-trous wavelet filter on the HDR mean, guided by noise-free first-hit features.
//   guide_kernel        four fixed sub-pixel primary rays per pixel through Tracer<CLAMP> (render_kernel.hip): land coverage, distance, normal,
//                       albedo, cloud transmittance
//   prep_mean_kernel    mean = S1 / n and the variance of the mean from S2 (temporal), or a marker that asks for the spatial estimate
//   prep_spatial_kernel the 7x7 variance of the luminance for the marked pixels
//   atrous_kernel       one level of the 5x5 B3-spline a-trous filter with edge-stopping weights; carries the variance along
// Included into de_api.hip's translation unit after render_kernel.hip (the anonymous-namespace Tracer is visible here).  The render kernels are untouched.
#include "de_kernels.h"

// Fixed constants of the edge-stopping terms (restated in tests/denoise_f64.py).  The luminance sigma and the levels are options.
#define DN_EPS_L 1e-6f            // luminance: exp(-|Y_p - Y_q| / (sigma_l sqrt(G3(v)_p) + DN_EPS_L))
#define DN_SIGMA_D 1.0f           // distance: exp(-|d_p - d_q| / (DN_SIGMA_D (|gx_p| |dx| + |gy_p| |dy|) + DN_EPS_D_REL d_p)), land on both sides only
#define DN_EPS_D_REL 1e-3f
#define DN_K_COV 16.0f            // coverage: exp(-16 |cov_p - cov_q|)
#define DN_K_ALB 10.0f            // albedo: exp(-10 L1(a_p - a_q))
#define DN_K_TR 10.0f             // cloud transmittance: exp(-10 |T_p - T_q|)
// normal: max(0, n_p . n_q)^128, land on both sides only
#define DN_MIN_TEMPORAL_N 4       // the per-pixel (temporal) variance needs n >= 4 samples and complete S2; below: the spatial estimate
#define DN_CLOUD_STEPS 64

struct DenoiseGuides {
    float4* nc;       // [H][W] (normal xyz, coverage)
    float4* at;       // [H][W] (albedo rgb, cloud transmittance)
    float* dist;      // [H][W] mean distance to the land hit of the hitting rays (0 when none hits)
};

// Four fixed sub-pixel rays (0.25 | 0.75, 0.25 | 0.75) in place of get_cast_dir's jitter; no RNG.
template <bool CLAMP>
__global__ void __launch_bounds__(256) guide_kernel(RenderArgs a, DenoiseGuides g) {
    const int u = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), v = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (u >= a.W || v >= a.H) return;
    const FrameConsts& fc = *a.fc;
    Work wk = {0, 0, 0, 0, 0};
    Tracer<CLAMP> tr(a, fc, wk);
    float hits = 0.0f, dist = 0.0f, trans = 0.0f;
    vec3 nsum = v3(0.0f, 0.0f, 0.0f), alb = v3(0.0f, 0.0f, 0.0f);
    for (int r = 0; r < 4; ++r) {
        const float ou = (r & 1) ? 0.75f : 0.25f, ov = (r & 2) ? 0.75f : 0.25f;
        const float fu = (2.0f * fc.fov * ((float)u + ou) / (float)a.H - fc.fov * fc.aspect_ratio - 1e-5f) * fc.aspect_scale;
        const float fv = 2.0f * fc.fov * ((float)v + ov) / (float)a.H - fc.fov - 1e-5f;
        const vec3 dir = normalized(fc.d + fu * fc.du + fv * fc.dv);
        const float t_land = tr.intersect_land(fc.cam_pos, dir);
        if (t_land > 0.0f) {
            const vec3 hp = fc.cam_pos + dir * t_land;
            hits += 1.0f;
            dist += t_land;
            nsum = nsum + tr.land_normal(hp);
            vec3 al; float ocean, bathy, emissive;
            tr.get_land_material(hp, &al, &ocean, &bathy, &emissive);
            alb = alb + al;
        }
        // cloud transmittance: DN_CLOUD_STEPS midpoint steps from the entry into the upper cloud sphere to the earlier of its exit and the land hit
        const vec2_ cs = rsi(fc.cam_pos, dir, DE_CLOUDS_UPPER);
        const float t0 = fmaxf(cs.x, 0.0f);
        float t1 = cs.y;
        if (t_land > 0.0f) t1 = fminf(t1, t_land);
        float tau = 0.0f;
        if (t1 > t0) {
            const float dt = (t1 - t0) / (float)DN_CLOUD_STEPS;
            float sum = 0.0f;
            for (int i = 0; i < DN_CLOUD_STEPS; ++i) sum += tr.get_clouds_density(fc.cam_pos + dir * (t0 + ((float)i + 0.5f) * dt));
            tau = DE_CLOUDS_EXTINCT * sum * dt;
        }
        trans += expf(-tau);
    }
    const float ln = sqrtf(nsum.x * nsum.x + nsum.y * nsum.y + nsum.z * nsum.z);
    const vec3 n = ln > 0.0f ? nsum * (1.0f / ln) : v3(0.0f, 0.0f, 0.0f);
    const size_t p = (size_t)v * a.W + u;
    g.nc[p] = make_float4(n.x, n.y, n.z, hits * 0.25f);
    g.at[p] = make_float4(alb.x * 0.25f, alb.y * 0.25f, alb.z * 0.25f, trans * 0.25f);
    g.dist[p] = hits > 0.0f ? dist / hits : 0.0f;
}

__device__ __forceinline__ float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

struct DenoisePrepArgs {
    const float* s1;          // [H][W][3]
    const float* s2;          // [H][W][3], or null: no temporal estimate
    const int32_t* tile_spp;  // [H/8][W/8] (adaptive frame), or null: every pixel has n = spp
    int spp, W, H;
    float4* out;              // [H][W] (mean rgb, variance of the mean; -1 = the spatial estimate is needed)
};

// Temporal: sd_c = sqrt(max(0, (S2_c - S1_c mean_c) / (n - 1))), v = (0.2126 sd_r + 0.7152 sd_g + 0.0722 sd_b)^2 / n — an upper bound on the
// variance of the luminance of the mean (the covariances are unknown).
__global__ void __launch_bounds__(256) prep_mean_kernel(DenoisePrepArgs a) {
    const int u = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), v = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (u >= a.W || v >= a.H) return;
    const size_t p = (size_t)v * a.W + u;
    const int n = a.tile_spp ? a.tile_spp[(v >> 3) * (a.W >> 3) + (u >> 3)] : a.spp;
    float m[3] = {0.0f, 0.0f, 0.0f};
    float var = -1.0f;
    if (n > 0) {
        const float nf = (float)n;
        for (int ch = 0; ch < 3; ++ch) m[ch] = a.s1[p * 3 + ch] / nf;
        if (a.s2 && n >= DN_MIN_TEMPORAL_N) {
            float sd[3];
            for (int ch = 0; ch < 3; ++ch) sd[ch] = sqrtf(fmaxf(0.0f, (a.s2[p * 3 + ch] - a.s1[p * 3 + ch] * m[ch]) / (nf - 1.0f)));
            const float y = dn_lum(sd[0], sd[1], sd[2]);
            var = y * y / nf;
        }
    } else {
        var = 0.0f;       // no samples: nothing to filter
    }
    a.out[p] = make_float4(m[0], m[1], m[2], var);
}

// Spatial: the population variance of the luminance of the means over the 7x7 neighbourhood inside the image (two passes).
__global__ void __launch_bounds__(256) prep_spatial_kernel(const float4* in, float4* out, int W, int H) {
    const int u = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), v = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (u >= W || v >= H) return;
    const size_t p = (size_t)v * W + u;
    float4 c = in[p];
    if (c.w < 0.0f) {
        const int x0 = max(u - 3, 0), x1 = min(u + 3, W - 1), y0 = max(v - 3, 0), y1 = min(v + 3, H - 1);
        float s = 0.0f;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) { const float4 q = in[(size_t)y * W + x]; s += dn_lum(q.x, q.y, q.z); }
        const float cnt = (float)((x1 - x0 + 1) * (y1 - y0 + 1));
        const float mean = s / cnt;
        float s2 = 0.0f;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) { const float4 q = in[(size_t)y * W + x]; const float d = dn_lum(q.x, q.y, q.z) - mean; s2 += d * d; }
        c.w = s2 / cnt;
    }
    out[p] = c;
}

struct AtrousArgs {
    const float4* in;         // [H][W] (colour rgb, variance)
    float4* out;              // [H][W]
    float* out3;              // [H][W][3] colour for the display (last level), or null
    DenoiseGuides g;
    int W, H, step;
    float sigma_l;
};

// One level, step h: the 5x5 B3-spline kernel (1/16, 1/4, 3/8, 1/4, 1/16)^2 at offsets h (dx, dy), taps outside the image skipped.  Weight of tap q:
// k * w, w = [max(0, n_p . n_q)^128] * exp(-(luminance + distance + coverage + albedo + transmittance terms)).  colour = sum(k w c_q) / sum(k w),
// variance = sum((k w)^2 v_q) / (sum(k w))^2.  G3(v)_p: the 3x3 kernel (1/4, 1/2, 1/4)^2 over the variances, coordinates clamped to the image.
__global__ void __launch_bounds__(256) atrous_kernel(AtrousArgs a) {
    const int u = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), v = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (u >= a.W || v >= a.H) return;
    const int W = a.W, H = a.H;
    const size_t p = (size_t)v * W + u;
    const float4 cp = a.in[p];
    const float4 ncp = a.g.nc[p], atp = a.g.at[p];
    const float dp = a.g.dist[p];
    const float k3[3] = {0.25f, 0.5f, 0.25f};
    float g3 = 0.0f;
    for (int j = -1; j <= 1; ++j)
        for (int i = -1; i <= 1; ++i) {
            const int x = min(max(u + i, 0), W - 1), y = min(max(v + j, 0), H - 1);
            g3 += (k3[i + 1] * k3[j + 1]) * a.in[(size_t)y * W + x].w;
        }
    const float denom_l = a.sigma_l * sqrtf(fmaxf(g3, 0.0f)) + DN_EPS_L;
    const float gx = 0.5f * (a.g.dist[(size_t)v * W + min(u + 1, W - 1)] - a.g.dist[(size_t)v * W + max(u - 1, 0)]);
    const float gy = 0.5f * (a.g.dist[(size_t)min(v + 1, H - 1) * W + u] - a.g.dist[(size_t)max(v - 1, 0) * W + u]);
    const float yp = dn_lum(cp.x, cp.y, cp.z);
    const float k5[5] = {1.0f / 16.0f, 0.25f, 0.375f, 0.25f, 1.0f / 16.0f};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int j = -2; j <= 2; ++j) {
        const int y = v + j * a.step;
        if (y < 0 || y >= H) continue;
        for (int i = -2; i <= 2; ++i) {
            const int x = u + i * a.step;
            if (x < 0 || x >= W) continue;
            const size_t q = (size_t)y * W + x;
            const float4 cq = a.in[q];
            const float k = k5[i + 2] * k5[j + 2];
            if (i == 0 && j == 0) {      // the centre tap: w = 1
                sw += k; sr += k * cq.x; sg += k * cq.y; sb += k * cq.z; sv += (k * k) * cq.w;
                continue;
            }
            const float4 ncq = a.g.nc[q], atq = a.g.at[q];
            const float dq = a.g.dist[q];
            float e = fabsf(yp - dn_lum(cq.x, cq.y, cq.z)) / denom_l;
            e += DN_K_COV * fabsf(ncp.w - ncq.w);
            e += DN_K_ALB * ((fabsf(atp.x - atq.x) + fabsf(atp.y - atq.y)) + fabsf(atp.z - atq.z));
            e += DN_K_TR * fabsf(atp.w - atq.w);
            float wn = 1.0f;
            if (ncp.w > 0.0f && ncq.w > 0.0f) {
                const float grad = DN_SIGMA_D * (fabsf(gx) * (float)abs(i * a.step) + fabsf(gy) * (float)abs(j * a.step)) + DN_EPS_D_REL * dp;
                e += fabsf(dp - dq) / fmaxf(grad, 1e-30f);
                float c = fmaxf(0.0f, (ncp.x * ncq.x + ncp.y * ncq.y) + ncp.z * ncq.z);
                for (int s = 0; s < 7; ++s) c = c * c;      // ^128
                wn = c;
            }
            const float w = k * (wn * expf(-e));
            sw += w;
            sr += w * cq.x; sg += w * cq.y; sb += w * cq.z;
            sv += (w * w) * cq.w;
        }
    }
    // the centre tap has w = 1: sw >= 9/64
    const float4 o = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
    a.out[p] = o;
    if (a.out3) { a.out3[p * 3 + 0] = o.x; a.out3[p * 3 + 1] = o.y; a.out3[p * 3 + 2] = o.z; }
}

// hdr_output_kernels.hip — the opt-in HDR display output (include/digital_earth_hdr_output.h): openDR_transform in its general form
// — a peak luminance, a display gamut, an inverse EOTF — in display_kernel's place, and the 10 / 16-bit pack behind it.
//   hdr_display_kernel<PER_TILE>   display_kernel's launch shape and DisplayArgs: one 256-thread block = one 32 x 32 pixel tile read along the rows of
//                                  the accumulation buffer, transformed, staged in LDS and written along the columns of the (W, H, 3) image.  Divide
//                                  by samples, vignette and exposure scale are display_pixel's; then lib/OpenDRT.py:325-485 with the constants of the
//                                  settings (HdrConsts, computed on the host in double: de_host_consts.h hdr_output_consts) BY VALUE in the kernel's
//                                  arguments — FrameConsts, which the render kernels read, is untouched.  No camera response, gamma or sRGB OETF.
//   hdr_transform_kernel           the transform alone on n colours (de_debug_hdr_transform)
//   hdr_pack_kernel                pixels_pack_kernel's shape: one block = one 32 x 32 tile of the displayed image read along its contiguous columns,
//                                  quantised to 10 or 16 bits (truncate / round / dither: the shared quantiser and noise of pack.h with maxcode in
//                                  255's place), staged in LDS as dwords (one per pixel, or one plane per channel; rows padded to 33) and
//                                  written as whole row segments of 32-bit words, rows top-down: RGB10A2 one dword per pixel (128 contiguous bytes
//                                  per row of a tile), RGB16 three halfwords per pixel = 48 dwords (192 bytes) per row.  The kernel is here; its
//                                  two halves around the barrier and HdrPackArgs are hdr_pack.h's, which a host build can include without the transform
//                                  (the derived alignment of its dword stores is stated there).
// The functions from hdr_eotf_pq to hdr_openDR_transform restate the algorithm of OpenDRT v0.2.2 ("Open Display Transform", written by Jed Smith,
// https://github.com/jedypod/open-display-transform), which the reference carries as a Taichi port in lib/OpenDRT.py under the notice
// "License: GPL v3" (lib/OpenDRT.py:5-10) — the same notice as on aux_kernels.hip's restatement of the live configuration.
// All float work is f32 in the reference's order with de_pow / de_log / de_sqrt of the arithmetic contract (no hardware transcendentals, no
// contraction: -ffp-contract=off), so a numpy restatement handed the device's own elementary functions (tests/hdr_output_ref.py) gives the same bits.
// No atomics, no scratch; every index is range-checked before its load or store.  Included into de_api.hip's translation unit behind aux_kernels.hip,
// whose helpers (sdivf, sdivf3f, vdot_rows, narrow_hue_angles) it shares; display_kernel is untouched.
#include "de_kernels.h"
#include "hdr_pack.h"

struct HdrConsts {
    float m, s, fl, ds, clamp_max, dch_s;      // lib/OpenDRT.py:270-271, 306-319, 404 for the settings' Lp and EOTF
    float xyz_to_display[9];                   // :72-74, row-major as written there
    float h_a, h_b, h_c, h_e;                  // HLG (:145-146): h_e = (1 - h_g) / h_g
    int transfer;                              // DE_HDR_TRANSFER_*
};

namespace {
// eotf_pq(rgb, 1), lib/OpenDRT.py:166-184; spowf3 is a plain pow per channel (:120-121).  m1, m2, c1, c2, c3 are exact in f32.
DE_DEV float hdr_pq1(float x) {
    const float m1 = (float)(2610.0 / 16384.0), m2 = (float)(2523.0 / 32.0), c1 = (float)(107.0 / 128.0), c2 = (float)(2413.0 / 128.0), c3 = (float)(2392.0 / 128.0);
    const float a = de_pow(x, m1);
    return de_pow((c1 + c2 * a) / (1.0f + c3 * a), m2);
}
DE_DEV vec3 hdr_eotf_pq(vec3 rgb) { return v3(hdr_pq1(rgb.x), hdr_pq1(rgb.y), hdr_pq1(rgb.z)); }
// _logf (:77-79): log2(x) / log2(10), log2(x) = log(x) / log(2) (taichi.math); both divisors are constants rounded to f32.
DE_DEV float hdr_log10(float x) { return (de_log(x) / (float)0.6931471805599453) / (float)3.321928094887362; }
DE_DEV float hdr_hlg1(const HdrConsts& h, float x) {                                                   // :153-155
    return (x <= (float)(1.0 / 12.0)) ? de_sqrt(3.0f * x) : h.h_a * hdr_log10(12.0f * x - h.h_b) + h.h_c;
}
// eotf_hlg(rgb, 1), :133-155.  Yd = 0 gives pow(0, negative) = +inf and 0 * inf = NaN in every channel, as in the reference.
DE_DEV vec3 hdr_eotf_hlg(const HdrConsts& h, vec3 rgb) {
    const float Yd = ((float)0.2627 * rgb.x + (float)0.6780 * rgb.y) + (float)0.0593 * rgb.z;
    rgb = rgb * de_pow(Yd, h.h_e);
    return v3(hdr_hlg1(h, rgb.x), hdr_hlg1(h, rgb.y), hdr_hlg1(h, rgb.z));
}
// openDR_transform, :221-485: aux_kernels.hip's body with the display matrix, the tonescale constants and the display scale of the settings, and the
// inverse EOTF behind the clamp.  drt_w = (rw, 1, bw) / |(rw, 1, bw)| (:369-370).
DE_DEV vec3 hdr_openDR_transform(const HdrConsts& h, vec3 drt_w, float p_R, float p_G, float p_B) {
    const float rec709_to_xyz[9] = {0.412390917540f, 0.357584357262f, 0.180480793118f, 0.212639078498f, 0.715168714523f,
                                    0.072192311287f, 0.019330825657f, 0.119194783270f, 0.950532138348f};
    const float dch_toe = 0.0f, hs_r = 0.3f, hs_g = -0.1f, hs_b = -0.2f;
    vec3 rgb = v3(p_R, p_G, p_B);
    rgb = vdot_rows(rec709_to_xyz, rgb);
    rgb = vdot_rows(h.xyz_to_display, rgb);
    float mx = de_max(rgb.x, de_max(rgb.y, rgb.z));
    float mn = de_min(rgb.x, de_min(rgb.y, rgb.z));
    vec3 h_rgb = narrow_hue_angles(sdivf3f(rgb - v3(mn, mn, mn), mx));
    vec3 w = drt_w * v3(de_max(rgb.x, 1e-5f), de_max(rgb.y, 1e-5f), de_max(rgb.z, 1e-5f));
    float lum_ = length(w);
    vec3 rats = sdivf3f(rgb, lum_);
    float ts = h.m * lum_ / (lum_ + h.s);                                 // spowf(., c = 1)
    ts = ((ts <= 0.0f) ? ts : ts * ts) / (ts + h.fl);                     // flare: spowf(x, 2)/(x + fl)
    ts *= h.ds;
    float ccf = sdivf(1.0f, lum_ * h.dch_s + 1.0f);
    float toe_ccf = (dch_toe + 1.0f) * sdivf(lum_, lum_ + dch_toe) * ccf;
    vec3 hs_w = (1.0f - ccf) * h_rgb;
    rats = v3(rats.x + hs_w.z * hs_b - hs_w.y * hs_g, rats.y + hs_w.x * hs_r - hs_w.z * hs_b, rats.z + hs_w.y * hs_g - hs_w.x * hs_r);
    rats = v3(1.0f - toe_ccf + rats.x * toe_ccf, 1.0f - toe_ccf + rats.y * toe_ccf, 1.0f - toe_ccf + rats.z * toe_ccf);
    rats = v3(de_max(rats.x, 0.0f), de_max(rats.y, 0.0f), de_max(rats.z, 0.0f));
    float rats_mx = de_max(rats.x, de_max(rats.y, rats.z));
    float rats_mn = de_min(rats.x, de_min(rats.y, rats.z));
    float rats_ch = sdivf(rats_mx - rats_mn, rats_mx);
    float chf_in = rats_ch * ts;
    float chf = (chf_in <= 0.0f) ? chf_in : de_sqrt(chf_in);             // spowf(., v_p = 0.5)
    vec3 rats_n = sdivf3f(rats, rats_mx);
    rats = rats_n * chf + rats * (1.0f - chf);
    rgb = rats * ts;
    rgb = v3(de_min(rgb.x, h.clamp_max), de_min(rgb.y, h.clamp_max), de_min(rgb.z, h.clamp_max));
    if (h.transfer == 1) rgb = hdr_eotf_pq(rgb);                          // :480-483
    else if (h.transfer == 2) rgb = hdr_eotf_hlg(h, rgb);
    return rgb;
}
}  // namespace

// display_pixel's first half (renderer.py:349-355), then the transform; nothing behind it.
template <bool PER_TILE>
DE_DEV void hdr_display_pixel(const DisplayArgs& a, const HdrConsts& h, int i, int j, float* o) {
    const int idx = j * a.W + i;
    const FrameConsts& k = *a.fc;
    float u = 1.0f * (float)i / (float)a.W;
    float v = 1.0f * (float)j / (float)a.H;
    float du = u - k.vig_cx, dv = v - k.vig_cy;
    float darken = 1.0f - k.vig_strength * de_max(de_sqrt(du * du + dv * dv) - k.vig_radius, 0.0f);
    const float* px = a.hdr + (size_t)idx * 3;
    float samples = PER_TILE ? (float)a.tile_spp[(j >> 3) * (a.W >> 3) + (i >> 3)] : (float)a.samples;
    vec3 linear = v3(px[0] / samples, px[1] / samples, px[2] / samples) * darken * k.exposure_scale;
    vec3 t = hdr_openDR_transform(h, k.drt_w, linear.x, linear.y, linear.z);
    o[0] = t.x; o[1] = t.y; o[2] = t.z;
}

template <bool PER_TILE>
__global__ void __launch_bounds__(256) hdr_display_kernel(DisplayArgs a, HdrConsts h) {
    __shared__ float tile[32][32 * 3 + 1];
    const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5;      // 32 x 8 threads
    const int i0 = (int)blockIdx.x * 32, j0 = (int)blockIdx.y * 32;
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + tx, j = j0 + ty + 8 * r;
        if (i < a.W && j < a.H) {
            float o[3];
            hdr_display_pixel<PER_TILE>(a, h, i, j, o);
            tile[ty + 8 * r][tx * 3 + 0] = o[0]; tile[ty + 8 * r][tx * 3 + 1] = o[1]; tile[ty + 8 * r][tx * 3 + 2] = o[2];
        }
    }
    __syncthreads();
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty + 8 * r, j = j0 + tx;                        // consecutive threads: consecutive j of one column i
        if (i < a.W && j < a.H) {
            float* o = a.image + ((size_t)i * a.H + j) * 3;
            o[0] = tile[tx][(ty + 8 * r) * 3 + 0]; o[1] = tile[tx][(ty + 8 * r) * 3 + 1]; o[2] = tile[tx][(ty + 8 * r) * 3 + 2];
        }
    }
}

__global__ void __launch_bounds__(256) hdr_transform_kernel(const float* rgb, float* out, size_t n, HdrConsts h) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    vec3 w = v3(0.25f, 1.0f, 0.35f);                                       // lib/OpenDRT.py:369, as setup_kernel states it
    const vec3 t = hdr_openDR_transform(h, w / length(w), rgb[k * 3], rgb[k * 3 + 1], rgb[k * 3 + 2]);
    out[k * 3] = t.x; out[k * 3 + 1] = t.y; out[k * 3 + 2] = t.z;
}

// ------------------------------------------------------------------------------------------------ the pack: its two halves are hdr_pack.h's
__global__ void __launch_bounds__(256) hdr_pack_kernel(HdrPackArgs a) {
    __shared__ uint32_t tile[HPX_PLANES][PACK_TILE][PACK_LDS_STRIDE];
    hdr_stage_tile(a, tile, (int)threadIdx.x, (int)blockIdx.x, (int)blockIdx.y);
    __syncthreads();
    hdr_store_tile(a, tile, (int)threadIdx.x, (int)blockIdx.x, (int)blockIdx.y);
}

// panorama_body.h — the per-pixel body of panorama_kernel and of environment_kernel (panorama_kernels.hip, include/digital_earth_panorama.h and
// include/digital_earth_environment.h) and its arguments,
// free of anything of the device, so that a host build (tools/panorama_host_check.cpp) runs it pixel by pixel under the sanitizers.  The includer
// brings DE_DEV and the three leaves PANO_SINCOS(x, &s, &c), PANO_SQRT(x), PANO_FLOOR(x): de_math.h's on the device.
// Every operation is a float32 operation rounded on its own (the unit is compiled with -ffp-contract=off); the header carries the definition, and
// tests/panorama_ref.py restates it.  Every index is clamped into its buffer before its load: a face tap into [0, N - 1]^2 of one of six slots, a
// table entry by the caller's range check of (i, j).  No atomics, no scratch.
#pragma once
#include <stdint.h>

#define PANO_TILE 32              // one workgroup = one 32 x 32 tile of the output
#define PANO_MAX_S 4

struct PanoArgs {
    const float* faces;           // [6][N][N][3]: slot f at f N N 3, each as the display writes it: index (u N + v) 3 + c
    float* out;                   // (width, height, 3): index (i height + j) 3 + c; environment_kernel: [height][width][3], index (j width + i) 3 + c
    const float* sin_lon;         // equirect: [width S], [width S], [height S], [height S]; fisheye: not read
    const float* cos_lon;
    const float* sin_lat;
    const float* cos_lat;
    int N, width, height, S, fisheye;
    float fov, scale;             // fl32(N / (N - 2 apron)), fl32(N / (2 fov))
    float half_aperture;          // fl32(aperture_deg pi / 360)
    float m[6][4];                // per face: e1.du, e2.du, e1.dv, e2.dv
};

// (cr, cu, cf) -> the bilinear sample of the face it belongs to, three channels.
DE_DEV void pano_sample(const PanoArgs& a, float cr, float cu, float cf, float* rgb) {
    const float ar = cr < 0.0f ? -cr : cr, au = cu < 0.0f ? -cu : cu, af = cf < 0.0f ? -cf : cf;
    int face;
    float p, q;
    if (ar >= au && ar >= af) { face = cr < 0.0f ? 1 : 0; p = cu / ar; q = cf / ar; }
    else if (au >= af) { face = cu < 0.0f ? 3 : 2; p = cr / au; q = cf / au; }
    else { face = cf < 0.0f ? 5 : 4; p = cr / af; q = cu / af; }
    const float* m = a.m[face];
    const float fu = p * m[0] + q * m[1], fv = p * m[2] + q * m[3];
    float X = (fu + a.fov) * a.scale - 0.5f, Y = (fv + a.fov) * a.scale - 0.5f;
    const float top = (float)(a.N - 1);
    X = X > 0.0f ? (X < top ? X : top) : 0.0f;      // NaN gives 0
    Y = Y > 0.0f ? (Y < top ? Y : top) : 0.0f;
    int i0 = (int)PANO_FLOOR(X), j0 = (int)PANO_FLOOR(Y);
    if (i0 > a.N - 2) i0 = a.N - 2;
    if (j0 > a.N - 2) j0 = a.N - 2;
    const float ax = X - (float)i0, ay = Y - (float)j0;
    const float* c0 = a.faces + (((size_t)face * (size_t)a.N + (size_t)i0) * (size_t)a.N + (size_t)j0) * 3;      // taps (i0, j0) and (i0, j0 + 1): six contiguous floats
    const float* c1 = c0 + (size_t)a.N * 3;                                                                          // (i0 + 1, j0) and (i0 + 1, j0 + 1)
    for (int ch = 0; ch < 3; ++ch) {
        const float t0 = c0[ch] + ax * (c1[ch] - c0[ch]);
        const float t1 = c0[3 + ch] + ax * (c1[3 + ch] - c0[3 + ch]);
        rgb[ch] = t0 + ay * (t1 - t0);
    }
}

// Sub-position (ki, kj) of the fisheye -> its value.
DE_DEV void pano_fisheye(const PanoArgs& a, int ki, int kj, float* rgb) {
    const float px = (float)(2 * ki + 1) / (float)(a.width * a.S) - 1.0f, py = (float)(2 * kj + 1) / (float)(a.height * a.S) - 1.0f;
    const float rho = PANO_SQRT(px * px + py * py);
    if (rho > 1.0f) { rgb[0] = 0.0f; rgb[1] = 0.0f; rgb[2] = 0.0f; return; }
    float st, ct;
    PANO_SINCOS(rho * a.half_aperture, &st, &ct);
    // rho == 0 cannot be reached under the size rule: the width is a multiple of 16, so 2 ki + 1 == width S has no solution; the branch is the header's definition
    if (rho == 0.0f) pano_sample(a, 0.0f, 0.0f, 1.0f, rgb);
    else pano_sample(a, st * (px / rho), st * (py / rho), ct, rgb);
}

// The running mean of output pixel (i, j), inside the image, into mean[3].  The four tables' entries of the pixel come through `sin_lon`, `cos_lon`
// (entry s at s lon_stride) and `sin_lat`, `cos_lat` (entry b at b lat_stride) — a kernel hands its LDS copies, the host check the tables themselves.
DE_DEV void pano_pixel_mean(const PanoArgs& a, int i, int j, const float* sin_lon, const float* cos_lon, int lon_stride, const float* sin_lat, const float* cos_lat, int lat_stride, float* mean) {
    mean[0] = 0.0f; mean[1] = 0.0f; mean[2] = 0.0f;
    int k = 0;
    for (int b = 0; b < a.S; ++b)
        for (int s = 0; s < a.S; ++s) {
            float v[3];
            if (a.fisheye) pano_fisheye(a, i * a.S + s, j * a.S + b, v);
            else {
                const float cl = cos_lat[b * lat_stride];
                pano_sample(a, cl * sin_lon[s * lon_stride], sin_lat[b * lat_stride], cl * cos_lon[s * lon_stride], v);
            }
            ++k;
            if (k == 1) { mean[0] = v[0]; mean[1] = v[1]; mean[2] = v[2]; }
            else {
                const float w = 1.0f / (float)k;
                for (int ch = 0; ch < 3; ++ch) mean[ch] = mean[ch] + (v[ch] - mean[ch]) * w;
            }
        }
}

// panorama_kernel's pixel: the display's layout, (width, height, 3) with the pixels of a column contiguous.
DE_DEV void pano_pixel(const PanoArgs& a, int i, int j, const float* sin_lon, const float* cos_lon, const float* sin_lat, const float* cos_lat, int lat_stride) {
    float mean[3];
    pano_pixel_mean(a, i, j, sin_lon, cos_lon, 1, sin_lat, cos_lat, lat_stride, mean);
    float* o = a.out + ((size_t)i * (size_t)a.height + (size_t)j) * 3;
    o[0] = mean[0]; o[1] = mean[1]; o[2] = mean[2];
}

// environment_kernel's pixel (include/digital_earth_environment.h): the same mean into [height][width][3], the pixels of a ROW contiguous
// and j = 0 still the bottom row — what the EXR layout reads with its rows flipped.
DE_DEV void pano_pixel_rows(const PanoArgs& a, int i, int j, const float* sin_lon, const float* cos_lon, int lon_stride, const float* sin_lat, const float* cos_lat, int lat_stride) {
    float mean[3];
    pano_pixel_mean(a, i, j, sin_lon, cos_lon, lon_stride, sin_lat, cos_lat, lat_stride, mean);
    float* o = a.out + ((size_t)j * (size_t)a.width + (size_t)i) * 3;
    o[0] = mean[0]; o[1] = mean[1]; o[2] = mean[2];
}

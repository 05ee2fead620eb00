// panorama_host_check.cpp — the panorama stage's per-pixel body (csrc/panorama_body.h) compiled for the HOST, so that the address and
// undefined-behaviour sanitizers can watch the face lookup and every index the bilinear gather forms (tools/panorama_host_check.py builds and
// drives this).  The body runs pixel by pixel over the whole output on heap blocks of exactly their sizes: the six face slots
// (6 N N 3 floats), the four tables and the output.  The leaves are restated here for the host: de_math.h's de_sincos with the C library's fmaf
// (a correctly rounded fused multiply-add), sqrtf and floorf.
//   panorama_host_check IN OUT [rows]
// rows: environment_kernel's side — pano_pixel_rows into [height][width][3], tile by tile with the tables staged as that kernel
// stages them in LDS, here in heap blocks of exactly the LDS arrays' sizes: longitude [s][il], latitude [jl S + b].
// IN: int32 N, width, height, S, fisheye; f32 fov, scale, half_aperture, m[6][4]; f32 sin_lon[width S], cos_lon[width S], sin_lat[height S],
// cos_lat[height S]; the faces [6][N][N][3] f32.  OUT: (width, height, 3) f32; rows: [height][width][3] f32.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_DEV static inline

static inline void host_sincos(float x, float* s_out, float* c_out) {      // de_math.h: de_sincos
    float k = floorf(fmaf(x, 0x1.45f306p-1f, 0.5f));
    float r = fmaf(-k, 0x1.92p+0f, x);
    r = fmaf(-k, 0x1.fb4p-12f, r);
    r = fmaf(-k, 0x1.4442d2p-24f, r);
    int q = ((int)k) & 3;
    float r2 = r * r;
    float ps = 0x1.6cca94p-19f;
    ps = fmaf(ps, r2, -0x1.a00f5ap-13f);
    ps = fmaf(ps, r2, 0x1.111108p-7f);
    ps = fmaf(ps, r2, -0x1.555556p-3f);
    float sn = fmaf(r * r2, ps, r);
    float pc = -0x1.241daap-22f;
    pc = fmaf(pc, r2, 0x1.a010dap-16f);
    pc = fmaf(pc, r2, -0x1.6c16b8p-10f);
    pc = fmaf(pc, r2, 0x1.555556p-5f);
    float cs = fmaf(r2 * r2, pc, fmaf(-0.5f, r2, 1.0f));
    float s = (q & 1) ? cs : sn;
    float c = (q & 1) ? sn : cs;
    if (q & 2) s = -s;
    if ((q + 1) & 2) c = -c;
    *s_out = s;
    *c_out = c;
}
#define PANO_SINCOS(x, s, c) host_sincos((x), (s), (c))
#define PANO_SQRT(x) sqrtf(x)
#define PANO_FLOOR(x) floorf(x)
#include "../digital_earth_amd/csrc/panorama_body.h"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);      // exactly n elements on the heap: one index past either end is the sanitizer's to find
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3 && !(argc == 4 && strcmp(argv[3], "rows") == 0)) return 2;
    const bool rows = argc == 4;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> head = take<int32_t>(f, 5);
    const std::vector<float> k = take<float>(f, 3 + 24);
    PanoArgs a;
    a.N = head[0]; a.width = head[1]; a.height = head[2]; a.S = head[3]; a.fisheye = head[4];
    if (a.N < 4 || a.width < 1 || a.height < 1 || a.S < 1 || a.S > PANO_MAX_S) return 2;
    a.fov = k[0]; a.scale = k[1]; a.half_aperture = k[2];
    memcpy(a.m, k.data() + 3, sizeof(a.m));
    const size_t nw = (size_t)a.width * a.S, nh = (size_t)a.height * a.S;
    const std::vector<float> sin_lon = take<float>(f, nw), cos_lon = take<float>(f, nw), sin_lat = take<float>(f, nh), cos_lat = take<float>(f, nh);
    const std::vector<float> faces = take<float>(f, (size_t)6 * a.N * a.N * 3);
    fclose(f);
    std::vector<float> out((size_t)a.width * a.height * 3);
    a.faces = faces.data(); a.out = out.data();
    a.sin_lon = sin_lon.data(); a.cos_lon = cos_lon.data(); a.sin_lat = sin_lat.data(); a.cos_lat = cos_lat.data();
    if (rows) {
        for (int j0 = 0; j0 < a.height; j0 += PANO_TILE)
            for (int i0 = 0; i0 < a.width; i0 += PANO_TILE) {
                std::vector<float> lon_s((size_t)PANO_MAX_S * PANO_TILE), lon_c(lon_s.size()), lat_s(lon_s.size()), lat_c(lon_s.size());
                for (int t = 0; t < PANO_TILE * a.S; ++t) {      // the kernel's staging, thread t
                    const long long ki = (long long)i0 * a.S + t, kj = (long long)j0 * a.S + t;
                    const bool in_i = ki < (long long)a.width * a.S, in_j = kj < (long long)a.height * a.S;
                    const int at = (t % a.S) * PANO_TILE + t / a.S;
                    lon_s[at] = in_i ? sin_lon[ki] : 0.0f; lon_c[at] = in_i ? cos_lon[ki] : 0.0f;
                    lat_s[t] = in_j ? sin_lat[kj] : 0.0f; lat_c[t] = in_j ? cos_lat[kj] : 0.0f;
                }
                for (int jl = 0; jl < PANO_TILE && j0 + jl < a.height; ++jl)
                    for (int il = 0; il < PANO_TILE && i0 + il < a.width; ++il)
                        pano_pixel_rows(a, i0 + il, j0 + jl, lon_s.data() + il, lon_c.data() + il, PANO_TILE, lat_s.data() + jl * a.S, lat_c.data() + jl * a.S, 1);
            }
    }
    else for (int i = 0; i < a.width; ++i)
        for (int j = 0; j < a.height; ++j)      // the tables' entries of the pixel, where the kernel hands its LDS copies: [S] along each axis, stride 1
            pano_pixel(a, i, j, sin_lon.data() + (size_t)i * a.S, cos_lon.data() + (size_t)i * a.S, sin_lat.data() + (size_t)j * a.S, cos_lat.data() + (size_t)j * a.S, 1);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    return 0;
}

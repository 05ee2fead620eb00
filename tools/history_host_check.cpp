// history_host_check.cpp — history_blend_kernel's own source (csrc/history_kernels.hip) compiled for the HOST, so that the address and undefined-behaviour
// sanitizers can watch every index it forms (tools/history_host_check.py builds and drives this).  The few device types and helpers the
// kernel file takes from de_kernels.h are restated here in plain C++ with the same expressions; the kernel runs one workgroup at a time, thread by thread.
//   history_host_check IN OUT
// IN: int32 W, H, has_history; float max_history, depth_tolerance; de_params current, history; then, in the device layout, m [H][W][3], n [H][W] (int32),
// dist [H][W], and with a history hist_c [H][W][4], hist_d [H][W].  OUT: the candidate [H][W][4], then the display's mean [H][W][3].
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../include/digital_earth.h"

#define DE_HISTORY_STANDALONE
#define DE_DEV static inline
#define __global__ static
#define __launch_bounds__(n)
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { float4 r = {x, y, z, w}; return r; }
struct vec3 { float x, y, z; };
static inline vec3 v3(float x, float y, float z) { vec3 r = {x, y, z}; return r; }
static inline vec3 operator+(vec3 a, vec3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline vec3 operator-(vec3 a, vec3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline vec3 operator*(vec3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
static inline vec3 operator*(float s, vec3 a) { return v3(s * a.x, s * a.y, s * a.z); }
static inline float dot(vec3 a, vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static inline float de_sqrt(float x) { return sqrtf(x); }
static inline vec3 normalized_ieee(vec3 a) { return a * (1.0f / de_sqrt(dot(a, a))); }
static inline vec3 cross(vec3 a, vec3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
struct FrameConsts { vec3 cam_pos, d, du, dv; float fov, aspect_ratio, aspect_scale; };      // the camera fields: all the kernel file reads
static struct { unsigned x, y; } blockIdx, threadIdx;

#include "../digital_earth_amd/csrc/history_kernels.hip"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);      // exactly n elements on the heap: one index past either end is the sanitizer's to find
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> head = take<int32_t>(f, 3);
    const std::vector<float> set = take<float>(f, 2);
    const std::vector<de_params> par = take<de_params>(f, 2);
    const int W = head[0], H = head[1];
    const bool has = head[2] != 0;
    const size_t npx = (size_t)W * H;
    const std::vector<float> m = take<float>(f, npx * 3);
    const std::vector<int32_t> n = take<int32_t>(f, npx);
    const std::vector<float> dist = take<float>(f, npx);
    const std::vector<float4> hist_c = take<float4>(f, has ? npx : 0);
    const std::vector<float> hist_d = take<float>(f, has ? npx : 0);
    fclose(f);
    std::vector<float> out(npx * 3), cand_d(npx);
    std::vector<float4> cand_c(npx);
    FrameConsts fc;
    HistoryCam cams[2];
    blockIdx.x = blockIdx.y = threadIdx.x = threadIdx.y = 0;
    history_camera_kernel(par[0], W, H, &fc, nullptr);
    history_camera_kernel(par[1], W, H, nullptr, &cams[0]);
    HistoryArgs a;
    a.s.hdr = m.data(); a.s.tile_spp = nullptr; a.s.samples = 1;
    a.n_tile = nullptr; a.n_pixel = n.data(); a.n_frame = 0;
    a.dist = dist.data(); a.fc = &fc;
    a.hist_c = has ? hist_c.data() : nullptr; a.hist_d = hist_d.data(); a.hist_cam = &cams[0];
    a.out = out.data(); a.cand_c = cand_c.data(); a.cand_d = cand_d.data(); a.cand_cam = &cams[1];
    a.s.W = W; a.s.H = H; a.max_history = set[0]; a.depth_tolerance = set[1];
    for (unsigned by = 0; by < (unsigned)((H + 15) / 16); ++by)
        for (unsigned bx = 0; bx < (unsigned)((W + 15) / 16); ++bx)
            for (unsigned t = 0; t < 256u; ++t) {
                blockIdx.x = bx; blockIdx.y = by; threadIdx.x = t;
                history_blend_kernel(a);
            }
    if (memcmp(cand_d.data(), dist.data(), npx * sizeof(float)) != 0 || memcmp(&cams[1].cam_pos, &fc.cam_pos, sizeof(vec3)) != 0) { fprintf(stderr, "candidate distance or camera differs\n"); return 1; }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(cand_c.data(), sizeof(float4), npx, f);
    fwrite(out.data(), sizeof(float), npx * 3, f);
    fclose(f);
    return 0;
}

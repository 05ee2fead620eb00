// panorama_kernels.hip — the opt-in panorama stage behind the display transform and ahead of every pack (include/digital_earth_panorama.h, DESIGN.md
// §25): six captured cube faces, each (N, N, 3) f32 as the display writes it, resampled to one (width, height, 3) equirectangular or fisheye image.
// The header carries the definition; panorama_body.h holds the per-pixel body (also built for the host, tools/panorama_host_check.cpp), this file the
// tables and the launch shape.
//   pano_build_tables   the equirect's four tables on the host, double precision, rounded once.
//   panorama_kernel     one 256-thread workgroup = one 32 x 32 tile of the output; thread t owns row jl = t & 31 of columns t >> 5, + 8, + 16, + 24.
//                       The output's contiguous axis is j (index (i height + j) 3 + c): the 32 lanes of half a wave write 32 consecutive pixels
//                       of one column, 384 contiguous bytes, three floats per lane.  The tile's table entries (32 S per axis, at most 2 KB in
//                       all) are staged in LDS with coalesced loads: the longitude entries of a column are read by all its lanes at once (a
//                       broadcast), the latitude entries are laid out [b][jl] so that the 32 lanes of a column read 32 consecutive words for
//                       every sub-row b, no bank shared.  The face taps are gathers: neighbouring output pixels land on neighbouring face pixels
//                       (an output pixel is about N / (width / 4) face pixels wide), two taps of a column are six contiguous floats, and the
//                       six faces of a 1024^2 camera (75 MB) are read once each per frame through L2; nothing is staged, there is no reuse beyond
//                       what the cache gives.  No atomics, no scratch.
// Included into de_api.hip's translation unit after output_scale_kernels.hip; no other kernel is touched.
#include "de_kernels.h"
#include <math.h>
#include <vector>

#define PANO_SINCOS(x, s, c) de_sincos((x), (s), (c))
#define PANO_SQRT(x) de_sqrt(x)
#define PANO_FLOOR(x) de_floor(x)
#include "panorama_body.h"

#define PANO_THREADS 256

// Entry k of an axis of n S entries: the angle ((k + 0.5) / (n S) - 0.5) span.  sin and cos in double, rounded once.
inline void pano_build_tables(int n, int S, double span, std::vector<float>* s, std::vector<float>* c) {
    const size_t m = (size_t)n * (size_t)S;
    s->resize(m); c->resize(m);
    for (size_t k = 0; k < m; ++k) {
        const double ang = (((double)k + 0.5) / (double)m - 0.5) * span;
        (*s)[k] = (float)sin(ang); (*c)[k] = (float)cos(ang);
    }
}

__host__ __device__ inline int pano_tiles(int n) { return (n + PANO_TILE - 1) / PANO_TILE; }

__global__ void __launch_bounds__(PANO_THREADS) panorama_kernel(PanoArgs a) {
    __shared__ float lon_s[PANO_TILE * PANO_MAX_S], lon_c[PANO_TILE * PANO_MAX_S];      // [il S + s]
    __shared__ float lat_s[PANO_MAX_S * PANO_TILE], lat_c[PANO_MAX_S * PANO_TILE];      // [b][jl]
    const unsigned tiles_j = (unsigned)pano_tiles(a.height);                            // a one-dimensional grid: a dimension of 65 535 blocks would not hold every height
    const int t = (int)threadIdx.x, i0 = (int)(blockIdx.x / tiles_j) * PANO_TILE, j0 = (int)(blockIdx.x % tiles_j) * PANO_TILE;
    if (!a.fisheye) {
        const int n = PANO_TILE * a.S;                                                  // at most 128: one pass of the first 128 threads per table
        if (t < n) {
            const long long ki = (long long)i0 * a.S + t, kj = (long long)j0 * a.S + t;
            const bool in_i = ki < (long long)a.width * a.S, in_j = kj < (long long)a.height * a.S;
            lon_s[t] = in_i ? a.sin_lon[ki] : 0.0f;
            lon_c[t] = in_i ? a.cos_lon[ki] : 0.0f;
            const int at = (t % a.S) * PANO_TILE + t / a.S;                             // entry jl S + b -> [b][jl]
            lat_s[at] = in_j ? a.sin_lat[kj] : 0.0f;
            lat_c[at] = in_j ? a.cos_lat[kj] : 0.0f;
        }
        __syncthreads();
    }
    const int jl = t & 31, j = j0 + jl;
    if (j >= a.height) return;
    for (int il = t >> 5; il < PANO_TILE; il += 8) {
        const int i = i0 + il;
        if (i >= a.width) return;
        pano_pixel(a, i, j, lon_s + il * a.S, lon_c + il * a.S, lat_s + jl, lat_c + jl, PANO_TILE);
    }
}

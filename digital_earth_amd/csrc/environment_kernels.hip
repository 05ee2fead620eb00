// environment_kernels.hip — the scene-linear panorama in FRONT of the display (include/digital_earth_environment.h): six linear face
// slots, captured from the frame's sums, resampled to one row-major image that the unchanged EXR layout (exr_kernels.hip) reads.  Two kernels:
//   environment_capture_kernel   sums -> slot.  One 256-thread workgroup = one 32 x 32 tile of pixels: the float32 division by the count (the frame's,
//                       or inside an adaptive frame the 8 x 8 tile's own: display_source.h) and the transposition from [N][N][3] with the pixels of a
//                       row contiguous to the slot's (i N + j) 3 + c with the pixels of a column contiguous, through a padded LDS tile so that both
//                       the loads and the stores of half a wave are 32 consecutive floats (environment_body.h: the two phases, the bank arithmetic).
//                       For the denoised source the same transposition over the filtered mean with the divisor 1 (x / 1.0f == x).
//   environment_kernel  slots -> [height][width][3].  panorama_kernel's per-pixel arithmetic, every rounded operation unchanged (panorama_body.h:
//                       pano_pixel_mean, shared, not copied), with the image and the tile walked the other way round: thread t owns column
//                       il = t & 31 of rows t >> 5, + 8, + 16, + 24, so the 32 lanes of half a wave store 32 consecutive pixels of one row, 384
//                       contiguous bytes.  The LDS tables are laid out the other way round too: the latitude entries of a row are read by all its
//                       lanes at once (a broadcast), the longitude entries lie [s][il], 32 consecutive words per sub-column s, no bank shared.  The
//                       face taps are gathers through L2 as panorama_kernel's; nothing is staged that is not reused.
// No atomics, no scratch.  Included into de_api.hip's translation unit directly behind panorama_kernels.hip, whose leaves (PANO_SINCOS, PANO_SQRT,
// PANO_FLOOR), tables (pano_build_tables) and launch shape (PANO_THREADS, pano_tiles) it shares; no other kernel is touched.
#include "de_kernels.h"
#include "display_source.h"
#include "panorama_body.h"
#include "environment_body.h"

__global__ void __launch_bounds__(ENV_THREADS) environment_capture_kernel(DisplaySrc s, float* slot) {
    __shared__ float tile[ENV_TILE_FLOATS];
    const unsigned tiles_i = (unsigned)((s.W + ENV_TILE - 1) / ENV_TILE);
    const int t = (int)threadIdx.x, i0 = (int)(blockIdx.x % tiles_i) * ENV_TILE, j0 = (int)(blockIdx.x / tiles_i) * ENV_TILE;
    env_tile_load(s, i0, j0, t, tile);
    __syncthreads();
    env_tile_store(slot, s.W, i0, j0, t, tile);
}

__global__ void __launch_bounds__(PANO_THREADS) environment_kernel(PanoArgs a) {
    __shared__ float lon_s[PANO_MAX_S * PANO_TILE], lon_c[PANO_MAX_S * PANO_TILE];      // [s][il]
    __shared__ float lat_s[PANO_TILE * PANO_MAX_S], lat_c[PANO_TILE * PANO_MAX_S];      // [jl S + b]
    const unsigned tiles_i = (unsigned)pano_tiles(a.width);                             // a one-dimensional grid, consecutive workgroups along a row of the image
    const int t = (int)threadIdx.x, i0 = (int)(blockIdx.x % tiles_i) * PANO_TILE, j0 = (int)(blockIdx.x / tiles_i) * PANO_TILE;
    if (!a.fisheye) {
        const int n = PANO_TILE * a.S;                                                  // at most 128: one pass of the first 128 threads per table
        if (t < n) {
            const long long ki = (long long)i0 * a.S + t, kj = (long long)j0 * a.S + t;
            const bool in_i = ki < (long long)a.width * a.S, in_j = kj < (long long)a.height * a.S;
            const int at = (t % a.S) * PANO_TILE + t / a.S;                             // entry il S + s -> [s][il]
            lon_s[at] = in_i ? a.sin_lon[ki] : 0.0f;
            lon_c[at] = in_i ? a.cos_lon[ki] : 0.0f;
            lat_s[t] = in_j ? a.sin_lat[kj] : 0.0f;
            lat_c[t] = in_j ? a.cos_lat[kj] : 0.0f;
        }
        __syncthreads();
    }
    const int il = t & 31, i = i0 + il;
    if (i >= a.width) return;
    for (int jl = t >> 5; jl < PANO_TILE; jl += 8) {
        const int j = j0 + jl;
        if (j >= a.height) return;
        pano_pixel_rows(a, i, j, lon_s + il, lon_c + il, PANO_TILE, lat_s + jl * a.S, lat_c + jl * a.S, 1);
    }
}

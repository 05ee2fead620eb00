// ibl_kernels.hip — the IBL bake (include/digital_earth_ibl.h): six linear face slots -> a cube map, its mip chain, the GGX-prefiltered
// levels, the nine SH coefficients of the irradiance and the DDS payload.  The per-texel bodies are ibl_body.h's; six kernels:
//   ibl_base_kernel     slots -> level 0.  One 256-thread workgroup = one 16 x 16 tile of one face, a wave an 8 x 8 block of it; the taps are
//                       panorama_body.h's pano_sample (shared, not copied), gathers through L2 as panorama_kernel's.
//   ibl_mip_kernel      level m - 1 -> level m, the same tiles; four texels in, one out.
//   ibl_spec_kernel     the hot path: one thread owns one texel of a specular level and walks the level's sample table in order.  All 64 lanes of a
//                       wave read the SAME table entry at the same time — a uniform address, so the entry travels through the scalar cache and costs
//                       no vector load and no LDS — and their reflected directions differ only by their normals, which are neighbours in an 8 x 8
//                       block: the eight taps of a sample fall into a few cache lines of the two source levels, shared by the wave and, through L2, by
//                       the neighbouring tiles.  Nothing is staged in LDS because no tap's address is known before the sample is: occupancy is bounded
//                       by registers alone.  A texel's samples are NOT spread over lanes: the weighted running mean is sequential by definition, and
//                       one texel per lane already gives 6 e^2 lanes per level (98 304 at e = 128).  The small levels (e <= 8: 384 lanes) leave the
//                       device idle for the microseconds they take; the levels are independent and run back to back on one stream.
//   ibl_sh_kernel       one workgroup = 256 texels of the SH level: 27 terms per thread, summed by a fixed tree in LDS into one partial per workgroup;
//   ibl_sh_final_kernel 27 threads add the partials in ascending order and apply the band factors (ordered_sum_kernel's idea: the order is the
//                       result's definition, not the hardware's choice).
//   ibl_pack_kernel     one thread = one RGBA texel of the file, in file order.
// No atomics, no scratch.  Included into de_api.hip's translation unit behind environment_kernels.hip, whose leaves (PANO_SQRT, PANO_FLOOR) it shares; no
// other kernel is touched.
#include "de_kernels.h"
#include "panorama_body.h"
#include "ibl_body.h"

// block -> (face, tile); false: the thread's texel lies outside the face
DE_DEV bool ibl_block_texel(int e, int* face, int* i, int* j) {
    const unsigned tiles = (unsigned)((e + IBL_TILE - 1) / IBL_TILE), per_face = tiles * tiles;
    const unsigned b = blockIdx.x % per_face;
    int il, jl;
    ibl_tile_texel((int)threadIdx.x, &il, &jl);
    *face = (int)(blockIdx.x / per_face);
    *i = (int)(b % tiles) * IBL_TILE + il;
    *j = (int)(b / tiles) * IBL_TILE + jl;
    return *i < e && *j < e;
}

__global__ void __launch_bounds__(IBL_THREADS) ibl_base_kernel(PanoArgs p, float* out, int E, int S) {
    int face, i, j;
    if (!ibl_block_texel(E, &face, &i, &j)) return;
    ibl_base_texel(p, out, E, S, face, i, j);
}

__global__ void __launch_bounds__(IBL_THREADS) ibl_mip_kernel(const float* src, float* dst, int e) {
    int face, i, j;
    if (!ibl_block_texel(e, &face, &i, &j)) return;
    ibl_mip_texel(src, dst, e, face, i, j);
}

__global__ void __launch_bounds__(IBL_THREADS) ibl_spec_kernel(IblLevelArgs a) {
    int face, i, j;
    if (!ibl_block_texel(a.e, &face, &i, &j)) return;
    ibl_spec_texel(a, face, i, j);
}

__global__ void __launch_bounds__(IBL_THREADS) ibl_sh_kernel(const float* level, const float* omega, int es, float* partial) {
    __shared__ float s[27][IBL_THREADS];
    const int t = (int)threadIdx.x, texel = (int)blockIdx.x * IBL_THREADS + t;
    float terms[27];
    if (texel < 6 * es * es) ibl_sh_terms(level, omega, es, texel, terms);
    else for (int k = 0; k < 27; ++k) terms[k] = 0.0f;
    for (int k = 0; k < 27; ++k) s[k][t] = terms[k];
    __syncthreads();
    for (int h = IBL_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) for (int k = 0; k < 27; ++k) s[k][t] = s[k][t] + s[k][t + h];
        __syncthreads();
    }
    if (t < 27) partial[(size_t)blockIdx.x * 27 + t] = s[t][0];
}

__global__ void __launch_bounds__(64) ibl_sh_final_kernel(const float* partial, int groups, float* sh) {
    const int k = (int)threadIdx.x;
    if (k >= 27) return;
    float acc = partial[k];
    for (int g = 1; g < groups; ++g) acc = acc + partial[(size_t)g * 27 + k];
    sh[k] = acc * ibl_sh_band_factor(k % 9);
}

__global__ void __launch_bounds__(IBL_THREADS) ibl_pack_kernel(IblPackArgs a) {
    const uint32_t idx = blockIdx.x * IBL_THREADS + threadIdx.x;
    if (idx >= 6u * a.texels_per_face) return;
    ibl_pack_texel(a, idx);
}

// adaptive_kernels.hip — adaptive sampling (de_accumulate_adaptive) around the unchanged render kernels:
//   accumulate_moments_kernel  accumulate_kernel plus the per-pixel sums of squares S2, in the same loop and the same association
//   adaptive_start_kernel      a frame's first active list (every tile, ascending) and its zero tile counts
//   adaptive_test_kernel       one wave64 per active tile: add the round's samples to the tile's count, decide whether it stays active
//   adaptive_compact_kernel    one 1024-thread workgroup: the tiles that stay, in ascending order, into the other list (ballot, popcount, workgroup scan)
// The display's per-tile sample count is display_kernel<true> (aux_kernels.hip).
#include "de_kernels.h"

// accumulate_kernel (aux_kernels.hip) inside an adaptive frame: the same sums S1 into the HDR buffer, and S2 = sum of rgb_s^2 per channel in sample
// order, acc = acc + x * x (the build has -ffp-contract=off: no fused multiply-add).  Same item layout, same grid.
__global__ void __launch_bounds__(256) accumulate_moments_kernel(RenderArgs a, float* s2) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t k = gid >> 6;
    if (k >= (uint32_t)a.n_tiles) return;
    const int sub = (int)(gid & 63u);
    const uint32_t tile = a.tiles[k];
    const int u = (int)(tile % (uint32_t)a.tiles_x) * 8 + (sub & 7);
    const int v = (int)(tile / (uint32_t)a.tiles_x) * 8 + (sub >> 3);
    const size_t p = ((size_t)v * a.W + u) * 3;
    float* px = a.hdr + p;
    float* sq = s2 + p;
    float acc_r = px[0], acc_g = px[1], acc_b = px[2];
    float sq_r = sq[0], sq_g = sq[1], sq_b = sq[2];
    const uint2* c = a.contrib + (size_t)k * 64u * (uint32_t)a.spp_count + sub;
    for (int s = 0; s < a.spp_count; ++s) {
        const uint2 q = c[(size_t)s * 64u];
        const float sample = __builtin_bit_cast(float, q.x);
        const LambdaNode& L = a.nodes[q.y];
        vec3 xyz = (sample * v3(L.rx, L.ry, L.rz)) * L.rcp_pdf;
        vec3 rgb = xyz_to_rgb_d65(xyz);
        acc_r += rgb.x; acc_g += rgb.y; acc_b += rgb.z;
        sq_r = sq_r + rgb.x * rgb.x; sq_g = sq_g + rgb.y * rgb.y; sq_b = sq_b + rgb.z * rgb.z;
    }
    px[0] = acc_r; px[1] = acc_g; px[2] = acc_b;
    sq[0] = sq_r; sq[1] = sq_g; sq[2] = sq_b;
}

__global__ void __launch_bounds__(256) adaptive_start_kernel(uint32_t* list, int32_t* tile_spp, int n_tiles) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (uint32_t)n_tiles) return;
    list[k] = k;
    tile_spp[k] = 0;
}

struct AdaptiveArgs {
    const float* hdr;        // S1, [H][W][3]
    const float* s2;         // S2, [H][W][3]
    const uint32_t* list;    // the round's active tiles (tile id = ty * tiles_x + tx), ascending
    int n_active;
    int32_t* tile_spp;       // [tiles_y][tiles_x]
    uint32_t* keep;          // [n_active]: 1 = the tile stays active
    int W, tiles_x;
    int n;                   // sample count of every active tile after the round
    int round;               // samples the round added
    int test;                // n >= min_spp: the noise test runs
    int stop;                // n >= max_spp: every tile leaves
    float tau2, floor2;      // threshold^2, floor^2
};

// One wave64 = one active tile, lane = pixel.  The tile stays iff some pixel and channel has var_c > tau^2 n (Y^2 + floor^2), with
// mean_c = S1_c / n, var_c = max(0, (S2_c - S1_c mean_c) / (n - 1)), Y = Rec.709 luminance of the means (include/digital_earth.h: de_adaptive).
__global__ void __launch_bounds__(256) adaptive_test_kernel(AdaptiveArgs a) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t k = gid >> 6;
    if (k >= (uint32_t)a.n_active) return;      // whole waves (64 | 256): the ballot below sees full waves only
    const int sub = (int)(gid & 63u);
    const uint32_t tile = a.list[k];
    bool noisy = false;
    if (a.test && !a.stop) {
        const int u = (int)(tile % (uint32_t)a.tiles_x) * 8 + (sub & 7);
        const int v = (int)(tile / (uint32_t)a.tiles_x) * 8 + (sub >> 3);
        const size_t p = ((size_t)v * a.W + u) * 3;
        const float n = (float)a.n, n1 = (float)(a.n - 1);
        float mean[3], var[3];
        for (int ch = 0; ch < 3; ++ch) {
            const float s1 = a.hdr[p + ch];
            mean[ch] = s1 / n;
            var[ch] = fmaxf(0.0f, (a.s2[p + ch] - s1 * mean[ch]) / n1);
        }
        const float Y = 0.2126f * mean[0] + 0.7152f * mean[1] + 0.0722f * mean[2];
        const float lim = a.tau2 * n * (Y * Y + a.floor2);
        noisy = var[0] > lim || var[1] > lim || var[2] > lim;
    }
    const bool stays = !a.stop && (!a.test || __ballot(noisy) != 0ull);
    if (sub == 0) {
        a.tile_spp[tile] += a.round;
        a.keep[k] = stays ? 1u : 0u;
    }
}

// Stable stream compaction of the active list: chunks of 1024 entries; per wave a ballot of the entries that stay and their popcount below each lane,
// across the 16 waves a scan of the per-wave totals in LDS.  out[] never aliases in[] (the two lists of the context alternate).
__global__ void __launch_bounds__(1024) adaptive_compact_kernel(const uint32_t* in, const uint32_t* keep, int n, uint32_t* out, int32_t* count) {
    __shared__ uint32_t wave_total[16];
    const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t base = 0;
    for (int k0 = 0; k0 < n; k0 += 1024) {
        const int k = k0 + t;
        const bool stays = k < n && keep[k] != 0u;
        const unsigned long long b = __ballot(stays);
        const uint32_t below = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[w] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t off = 0, total = 0;
        for (int i = 0; i < 16; ++i) {
            const uint32_t s = wave_total[i];
            off += i < w ? s : 0u;
            total += s;
        }
        if (stays) out[base + off + below] = in[k];
        base += total;
        __syncthreads();      // wave_total is written again by the next chunk
    }
    if (t == 0) *count = (int32_t)base;
}

// pt_leaves.h — the LEAVES of path_tracer / ray_marcher: pure functions of their arguments, stated once and called by every statement of the
// integrator (per-lane loops: render_kernel.hip, legacy/render_kernel_v1.hip; wave-level state machine: render_kernel_v2.hip; stage form:
// de_stages.h under render_kernel_v6.hip and legacy/render_kernel_v3.hip / _v5.hip).  The integrators stay independent texts — "v6 = v2 = legacy
// v1 / v3 / v5 = oracle, bit for bit" compares THEM; what they share is only what takes no path state by reference.
#pragma once
#include "de_kernels.h"

namespace pt {

// what a tracking loop reports (pathtracer.py:73-75)
enum { EV_NULL = 0, EV_ABSORB = 1, EV_SCATTER = 2 };

// get_density(h) for the gas stage's look-ahead (de_stages.h: GasStageT<true>), h = max(|C| - R, 0) — or a NaN.  The altitude table's entry 2h where
// the table has one (aux_kernels.hip, dens_table_kernel: entry i IS get_density(i / 2), and a step's altitude is a multiple of 0.5 m), the profiles
// evaluated elsewhere: what the state machine reads.  `live` = the lane is still inside its segment; one that is not reads a clamped entry, which
// nothing consumes (its point may lie anywhere above the table: evaluating there would send the whole wave through four exponentials).
// Every lane reads, live or not: a load under a lane condition is a select on its result, and the select waits next to the load.  The result is ONE
// 96-bit value, read through a pointer known to be global memory (a global_load counts on the vector-memory counter alone; dens_table_read's
// flat_load counts on the LDS counter too) at a 32-bit byte offset (index < 2^18: the full-rate multiply) from a base that can stay in scalar registers.
// de_debug_math evaluates it as functions 20-22 (tests/test_gpu_gas_lookahead.py: the index boundary).
typedef float f3v __attribute__((ext_vector_type(3)));
DE_DEV f3v density_ahead(const float* table, float h, bool live) {
    typedef const __attribute__((address_space(1))) char* de_gbytes;
    typedef f3v f3v_entry __attribute__((aligned(4)));      // an entry is 12 bytes at a multiple of 12
    typedef const __attribute__((address_space(1))) f3v_entry* de_gf3;
    static_assert(DE_DENS_STRIDE == 3, "one 96-bit read per entry");
    const float h2 = h * 2.0f;
    const uint32_t off = (uint32_t)__umul24((uint32_t)(int)__builtin_fminf(h2, (float)(DE_DENS_TABLE_N - 1)), (uint32_t)(DE_DENS_STRIDE * sizeof(float)));
    f3v dens = *(de_gf3)((de_gbytes)table + off);
    if (live & !(h2 < (float)DE_DENS_TABLE_N)) { const vec3 d = get_density(h); dens = f3v{d.x, d.y, d.z}; }
    return dens;
}

// pathtracer.py:145-169
DE_DEV void intersect_cloud_limits(vec3 ray_pos, vec3 ray_dir, float land_isection, float* t_start_out, float* t_max_out) {
    float t_start = 0.0f, t_max = 0.0f;
    float elevation = length(ray_pos);
    vec2_ lower = rsi(ray_pos, ray_dir, DE_CLOUDS_LOWER);
    vec2_ upper = rsi(ray_pos, ray_dir, DE_CLOUDS_UPPER);
    if (elevation >= DE_CLOUDS_UPPER) {
        t_start = de_max(0.0f, upper.x);
        t_max = (lower.y >= 0.0f) ? lower.x : upper.y;
        if (upper.y < 0.0f) t_max = -1.0f;
    } else if (elevation >= DE_CLOUDS_LOWER) {
        t_start = 0.0f;
        t_max = (lower.y >= 0.0f) ? lower.x : upper.y;
    } else {
        t_start = lower.y;
        t_max = upper.y;
        if (land_isection > 0.0f) t_max = -1.0f;
    }
    *t_start_out = t_start; *t_max_out = t_max;
}
// pathtracer.py:145-168 up to (not including) the `if land_isection > 0.0: t_max = -1.0` of the below-cloud branch:
// everything that depends on the ray alone, computed when the ray is set up.  `below` tells the caller to apply that line.
DE_DEV void cloud_limits_of_ray(vec3 ray_pos, vec3 ray_dir, float* t_start_out, float* t_max_out, int* below_out) {
    float t_start = 0.0f, t_max = 0.0f;
    int below = 0;
    float elevation = length_nr(ray_pos);
    vec2_ lower = rsi(ray_pos, ray_dir, DE_CLOUDS_LOWER);
    vec2_ upper = rsi(ray_pos, ray_dir, DE_CLOUDS_UPPER);
    if (elevation >= DE_CLOUDS_UPPER) {
        t_start = de_max(0.0f, upper.x);
        t_max = (lower.y >= 0.0f) ? lower.x : upper.y;
        if (upper.y < 0.0f) t_max = -1.0f;
    } else if (elevation >= DE_CLOUDS_LOWER) {
        t_start = 0.0f;
        t_max = (lower.y >= 0.0f) ? lower.x : upper.y;
    } else {
        t_start = lower.y;
        t_max = upper.y;
        below = 1;
    }
    *t_start_out = t_start; *t_max_out = t_max; *below_out = below;
}
// pathtracer.py:235-247
DE_DEV float evaluate_phase(const FrameConsts& fc, vec3 ray_dir, vec3 light_dir, int id, bool reduce_peak) {
    float phase = 0.0f;
    float c = dot(ray_dir, light_dir);
    if (id == RAYLEIGH_ID) phase += rayleigh_phase(c);
    else if (id == MIE_ID) phase += klein_nishina_phase(c, DE_MIE_ASYMMETRY, fc.kn_log);
    else if (id == CLOUD_ID) phase += cloud_phase(fc.cloud, c, reduce_peak);
    else if (id == ISOTROPIC_CLOUD_ID) phase += (float)(1.0 / (4.0 * M_PI));
    return phase;
}
// pathtracer.py:249-261
DE_DEV vec3 sample_phase(const FrameConsts& fc, Rng& rng, vec3 ray_dir, int id, bool reduce_peak, float* phase_div_pdf) {
    *phase_div_pdf = 1.0f;
    if (id == RAYLEIGH_ID || id == ISOTROPIC_CLOUD_ID) {
        float r0 = rng_next(rng);
        float r1 = rng_next(rng);
        vec3 d = sample_sphere(r0, r1);
        *phase_div_pdf = evaluate_phase(fc, ray_dir, d, id, reduce_peak) * (float)(4.0 * M_PI);
        return d;
    } else if (id == MIE_ID) {
        return sample_klein_nishina_phase(rng, ray_dir, DE_MIE_ASYMMETRY);
    }
    return sample_cloud_phase(fc.cloud, rng, ray_dir, reduce_peak);
}
DE_DEV float srgb_to_spectrum(const LambdaNode& L, vec3 rgb) {   // lib/colour.py:62-71 with the per-wavelength part tabulated
    return (L.s2s_valid != 0.0f) ? dot(rgb, v3(L.c0, L.c1, L.c2)) : 0.0f;
}
// renderer.py:269-279
DE_DEV vec3 get_cast_dir(Rng& rng, const FrameConsts& fc, int H, int u, int v) {
    float fov = fc.fov;
    float fu = (2.0f * fov * ((float)u + rng_next(rng)) / (float)H - fov * fc.aspect_ratio - 1e-5f) * fc.aspect_scale;
    float fv = 2.0f * fov * ((float)v + rng_next(rng)) / (float)H - fov - 1e-5f;
    return normalized(fc.d + fu * fc.du + fv * fc.dv);
}

// spectrum_sample's bisection (lib/colour.py:21-39) on the tabulated node values; returns the heap index of the node.  The first LDS_LEVELS
// levels of the tree are read from lds_val (a wave's LDS copy of node_val[0 .. 2^LDS_LEVELS)), the rest from global memory; LDS_LEVELS = 0
// reads global memory only (lds_val is not touched).
template <int LDS_LEVELS>
DE_DEV int spectrum_node(const float* lds_val, const float* node_val, float sample) {
    int n = 1;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        float val = (it < LDS_LEVELS) ? lds_val[n] : node_val[n];
        if (val < sample) n = 2 * n + 1;
        else if (val > sample) n = 2 * n;
        else break;
    }
    return n;
}
// The state machine's LDS_LEVELS (measured per frame: 0 levels 232 ms, 5 levels 230 ms, 6 levels 228 ms, 7 levels 238 ms — the LDS
// they take is what limits the waves per CU; reading the last two levels with one 32-byte block read changed nothing).
#ifndef DE_V2_LDS_TREE_LEVELS
#define DE_V2_LDS_TREE_LEVELS 6
#endif

// NOT here: get_land_material's grading (pathtracer.py:294-305).  Stated as a function it is simplified on its own before it is inlined, and the
// compiler then schedules render_kernel_v2 and render_kernel_v6's surface stage differently (same arithmetic, other instruction order): each of the
// three statements keeps its own copy so that the product kernels' machine code does not depend on this header's shape.

// pathtracer.py:466-467 (ray_marcher: :682-683): inf, NaN or negative -> 0
DE_DEV float clean_radiance(float x) {
    if (__builtin_isinf(x) || x != x || x < 0.0f) x = 0.0f;
    return x;
}

// pathtracer.py:461-463 (ray_marcher: :677-679): what the star map adds to a primary ray that leaves the scene
DE_DEV float stars_term(const LambdaNode& L, vec3 stars_srgb) {
    float stars_power = srgb_to_spectrum(L, stars_srgb);
    return stars_power * L.sun_power * 0.0000001f;
}

// MODE 1 of the per-lane kernels and the state machine: one lane's work counters into the launch's (de_counters; digital_earth_debug.h)
DE_DEV void flush_work_counters(unsigned long long* counters, uint32_t samples, uint32_t taps_r8, uint32_t taps_rgb, uint32_t sphere_steps,
                                uint32_t tracking_steps, uint32_t vertices, uint32_t draws) {
    atomicAdd(&counters[0], (unsigned long long)samples);
    atomicAdd(&counters[1], (unsigned long long)taps_r8);
    atomicAdd(&counters[2], (unsigned long long)taps_rgb);
    atomicAdd(&counters[3], (unsigned long long)sphere_steps);
    atomicAdd(&counters[4], (unsigned long long)tracking_steps);
    atomicAdd(&counters[5], (unsigned long long)vertices);
    atomicAdd(&counters[6], (unsigned long long)draws);
}

}  // namespace pt

// render_kernel.hip — the ray marcher's file: Renderer.render (renderer.py:283-330) with pathtracer.ray_marcher (pathtracer.py:544-685) for gfx950,
// the per-lane pieces it is made of (struct Tracer: the land SDF, its normal and sphere trace, the density lookups, the land material — what
// denoise_kernels.hip's guide kernel and the legacy per-lane path tracer, legacy/render_kernel_v1.hip, build on too) and the one per-lane kernel body.
//
// Work decomposition: one 64-lane wavefront owns one 8x8-pixel tile, one lane owns one pixel and traces that
// pixel's samples in order, so `color_buffer[u, v] += ...` (renderer.py:330) keeps the reference's association
// ((c + s0) + s1) + ... whatever the launch shape or the number of GPUs.  The RGB sum lives in registers for the
// whole launch: one read-modify-write of the HDR buffer per pixel per launch instead of one per sample.
//
// Differences from a literal transcription, all value-preserving under the arithmetic contract:
//  * everything that depends only on the wavelength comes from the LambdaNode table (setup_kernel);
//  * |pos| is computed once per evaluation point and shared by the SDF, the normalisation and the elevation.
#pragma once
#include "pt_leaves.h"

namespace {

struct Work { uint32_t taps_r8, taps_rgb, sphere_steps, tracking_steps, vertices; };

// TABLE: gas densities from the altitude table (de_kernels.h DE_DENS_TABLE_N) instead of four exponentials per point —
// the ray marcher evaluates 64 x 17 points per bounce.  Same values by construction (the table holds get_density itself).
template <bool CLAMP, bool TABLE = false>
struct Tracer {
    const RenderArgs& a;
    const FrameConsts& fc;
    Work& wk;
    __device__ Tracer(const RenderArgs& a_, const FrameConsts& fc_, Work& wk_) : a(a_), fc(fc_), wk(wk_) {}

    // pathtracer.py:11-14
    DE_DEV float land_sdf(vec3 pos) {
        float len = length(pos);
        vec3 n = pos * (1.0f / len);            // normalized() under contract 2
        wk.taps_r8++;
        return len - DE_PLANET_R - fc.land_height_scale * sphere_tap_r8<CLAMP>(a.topo, n);
    }
    // pathtracer.py:16-25
    DE_DEV vec3 land_normal(vec3 pos) {
        float d = land_sdf(pos);
        float e = fc.normal_eps;
        vec3 n = v3(d - land_sdf(pos - v3(e, 0.0f, 0.0f)), d - land_sdf(pos - v3(0.0f, e, 0.0f)), d - land_sdf(pos - v3(0.0f, 0.0f, e)));
        return normalized(n);
    }
    // pathtracer.py:27-46
    DE_DEV float intersect_land(vec3 pos, vec3 dir) {
        float ray_dist = 0.0f;
        const float max_ray_dist = (float)(6371e3 * 10.0);
        vec2_ rsi_dist = rsi(pos, dir, DE_ATMOS_UPPER);
        if (rsi_dist.x > 0.0f) ray_dist = rsi_dist.x;
        for (int i = 0; i < 250; ++i) {
            vec3 ro = pos + dir * ray_dist;
            float dist = land_sdf(ro);
            ray_dist += dist;
            wk.sphere_steps++;
            if (ray_dist > max_ray_dist || de_abs(dist) < ray_dist * 0.0001f) break;
        }
        return (ray_dist < max_ray_dist) ? ray_dist : -1.0f;
    }
    // pathtracer.py:48-65
    DE_DEV float get_clouds_density(vec3 pos) {
        float r = length(pos);
        float density = 0.0f;
        if (r > DE_CLOUDS_LOWER && r < DE_CLOUDS_UPPER) {
            float h = (r - DE_CLOUDS_LOWER) * (1.0f / DE_CLOUDS_THICKNESS);
            wk.taps_r8++;
            float cloud_texture = sphere_tap_r8<CLAMP>(a.clouds, pos * (1.0f / r));
            float column_height = cloud_texture;
            const float split = 0.2f;
            density = (h - split < column_height * (float)(1.0 - 0.2) && split - h < column_height * split) ? de_max(cloud_texture, 0.4f) : 0.0f;
        }
        return density * DE_CLOUDS_DENSITY;
    }
    DE_DEV vec3 gas_density(vec3 pos) {   // volume.get_density(volume.get_elevation(pos))
        if (TABLE) {
            // |pos| in [2^22, 2^23) m has a spacing of 0.5 m: h is an exact multiple of 0.5 and 2h is the table index
            const float len = de_sqrt_nr((pos.x * pos.x + pos.y * pos.y) + pos.z * pos.z);
            const float h2 = de_max(len - DE_PLANET_R, 0.0f) * 2.0f;
            if (h2 < (float)DE_DENS_TABLE_N) {
                return dens_table_read(a.dens_table, (uint32_t)(int)h2);
            }
            return get_density(len - DE_PLANET_R);
        }
        return get_density(de_sqrt((pos.x * pos.x + pos.y * pos.y) + pos.z * pos.z) - DE_PLANET_R);
    }
    // pathtracer.py:284-313
    DE_DEV void get_land_material(vec3 pos, vec3* albedo_srgb, float* ocean_out, float* bathy_out, float* emissive_out) {
        vec3 n = normalized(pos);
        vec2_ uv = sphere_UV_map(n);
        float u = fract_(uv.x * 1.0f), v = fract_(uv.y * 1.0f);
        float ocean = tap_r8<CLAMP>(a.ocean, u, v);
        vec3 tex = tap_rgb<CLAMP>(a.albedo, u, v);
        vec3 land = mix3(lum3(tex), tex, 6.5f);
        float greenery = sqr(land.y / lum(land));
        greenery = smoothstep_(1.5f, 1.9f, greenery);
        land = (1.0f * tex) / (greenery * 0.7f + 1.0f);
        land = mix3(lum3(land), land, 1.4f - greenery * 0.45f);
        land = mix3(land, (land * v3(255.0f, 128.0f, 64.0f)) / 255.0f, 0.2f * (1.0f - greenery));
        vec3 ocean_albedo = mix3(lum3(tex), tex, 0.75f) * 0.9f;
        *albedo_srgb = mix3(land, ocean_albedo, ocean);
        *ocean_out = ocean;
        *bathy_out = tap_r8<CLAMP>(a.bathy, u, v);
        *emissive_out = tap_r8<CLAMP>(a.emissive, u, v);
        wk.taps_r8 += 3;
        wk.taps_rgb += 1;
    }

    // ---------------------------------------------------------------- ray marcher, pathtracer.py:471-685
    DE_DEV float ray_march_transmittance(vec3 ray_pos, vec3 ray_dir, vec3 rmo_ext) {
        const int steps = 16;
        const float r_steps = 1.0f / (float)steps;
        float tr = 0.0f;
        bool blocked = rsi(ray_pos, ray_dir, DE_PLANET_R).y > 0.0f;
        if (!blocked) {
            vec2_ atmos = rsi(ray_pos, ray_dir, DE_ATMOS_UPPER);
            float t_max = atmos.y;
            if (atmos.y < 0.0f) t_max = -1.0f;
            float dd = t_max * r_steps;
            vec3 ray_step = ray_dir * dd;
            vec3 od = v3(0.0f, 0.0f, 0.0f);
            for (int i = 0; i < steps; ++i) {
                vec3 density = gas_density(ray_pos);
                od = od + density * dd;
                ray_pos = ray_pos + ray_step;
            }
            tr = de_exp(-dot(rmo_ext, od));
        }
        return tr;
    }
    DE_DEV void ray_march_atmos(vec3 ray_pos, vec3 ray_dir, float t_start, float t_max, vec3 sun_dir, vec3 rmo_ext, float sc_r, float sc_m,
                                float* in_scatter_out, float* tr_out) {
        const int steps = 64;
        const float r_steps = 1.0f / (float)steps;
        float dd = (t_max - t_start) * r_steps;
        vec3 ray_step = ray_dir * dd;
        ray_pos = ray_pos + ray_dir * t_start;
        float c = dot(ray_dir, sun_dir);
        float ph_r = rayleigh_phase(c), ph_m = klein_nishina_phase(c, DE_MIE_ASYMMETRY, fc.kn_log);
        float tr = 1.0f, in_scatter = 0.0f;
        for (int i = 0; i < steps; ++i) {
            vec3 density = gas_density(ray_pos);
            float step_od = dot(rmo_ext, density * dd);
            float step_tr = de_saturate(de_exp(-step_od));
            float step_integral = de_saturate((1.0f - step_tr) / step_od);
            float visible = tr * step_integral;
            float sun_tr = ray_march_transmittance(ray_pos, sun_dir, rmo_ext);
            float step_scattering = sc_r * (density.x * ph_r) + sc_m * (density.y * ph_m);
            in_scatter += step_scattering * sun_tr * visible * dd;
            tr *= step_tr;
            ray_pos = ray_pos + ray_step;
        }
        *in_scatter_out = in_scatter; *tr_out = tr;
    }
    DE_DEV float ray_marcher(Rng& rng, const LambdaNode& L, vec3 ray_pos, vec3 ray_dir) {
        const vec3 primary_dir = ray_dir;
        vec3 ext = v3(L.ext_r, L.ext_m, L.ext_o);
        float sc_r = ext.x * 1.0f, sc_m = ext.y * 0.95f;
        bool primary_miss = false;
        float accum = 0.0f, throughput = 1.0f;
        for (int scatter_count = 0; scatter_count < 3; ++scatter_count) {
            wk.vertices++;
            float earth_intersection = intersect_land(ray_pos, ray_dir);
            vec2_ atmos = rsi(ray_pos, ray_dir, DE_ATMOS_UPPER);
            float t_start = de_max(0.0f, atmos.x);
            float t_max = (earth_intersection > 0.0f) ? earth_intersection : atmos.y;
            if (atmos.y < 0.0f) {
                primary_miss = (scatter_count == 0);
                break;
            }
            vec3 light_dir = tangent_space_apply(fc.light_dir, sample_cone(rng, fc.sun_cos_angle));
            float in_scatter, tr;
            ray_march_atmos(ray_pos, ray_dir, t_start, t_max, light_dir, ext, sc_r, sc_m, &in_scatter, &tr);
            accum += throughput * in_scatter;
            throughput *= tr;
            if (earth_intersection > 0.0f) {
                vec3 land_pos = ray_pos + ray_dir * earth_intersection;
                vec3 land_n = land_normal(land_pos);
                vec3 albedo_srgb;
                float ocean, bathy, emissive;
                get_land_material(land_pos, &albedo_srgb, &ocean, &bathy, &emissive);
                float albedo = pt::srgb_to_spectrum(L, albedo_srgb);
                accum += throughput * emissive * L.night_power;
                vec3 offset_pos = land_pos * fc.offset_scale;
                bool visible = intersect_land(offset_pos, light_dir) < 0.0f;
                float direct_tr = 1.0f;
                float direct_ndl;
                float direct_brdf = earth_brdf(albedo, ocean, bathy, -ray_dir, land_n, light_dir, &direct_ndl);
                accum += throughput * direct_tr * (visible ? 1.0f : 0.0f) * L.sun_irradiance * direct_brdf * direct_ndl;
                vec3 view_dir = -ray_dir;
                ray_dir = sample_hemisphere_cosine_weighted(rng, land_n);
                ray_pos = offset_pos;
                float unused;
                float brdf = earth_brdf(albedo, ocean, bathy, view_dir, land_n, ray_dir, &unused);
                throughput *= brdf * (float)M_PI;
            }
        }
        if (primary_miss) {
            if (dot(fc.light_dir, primary_dir) > fc.sun_cos_angle) accum += L.sun_power;
            wk.taps_rgb += 1;
            accum += pt::stars_term(L, sphere_tap_rgb<CLAMP>(a.stars, normalized(primary_dir)));
        }
        return pt::clean_radiance(accum);
    }
};

// The per-lane kernels' body: tile -> pixel, the HDR read, the pixel's samples in order, the HDR write, the counters.  `trace` is how one sample
// is traced: (Work&, Rng&, const LambdaNode&, ray_pos, ray_dir) -> radiance.
// MODE 0: accumulate; 1: accumulate + work counters; 2: trace one sample per pixel into debug_out (no accumulation)
template <int MODE, typename Trace>
DE_DEV void per_lane_body(const RenderArgs& a, Trace trace) {
    const int wave = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= a.n_tiles) return;
    const uint32_t tile = a.tiles[wave];
    const int lane = threadIdx.x & 63;
    const int u = (int)(tile % (uint32_t)a.tiles_x) * 8 + (lane & 7);
    const int v = (int)(tile / (uint32_t)a.tiles_x) * 8 + (lane >> 3);
    const uint32_t pixel = (uint32_t)(v * a.W + u);
    const FrameConsts& fc = *a.fc;
    Work wk = {0, 0, 0, 0, 0};
    float* px = a.hdr + (size_t)pixel * 3;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
    if (MODE != 2) { acc_r = px[0]; acc_g = px[1]; acc_b = px[2]; }
    uint32_t draws = 0;
    for (int s = 0; s < a.spp_count; ++s) {
        Rng rng;
        rng_seed(rng, a.seed_lo, a.seed_hi, pixel, (uint32_t)(a.spp_begin + s * a.spp_stride));
        int node = 0;
        if (!a.fixed_wavelength) node = pt::spectrum_node<0>(nullptr, a.node_val, rng_next(rng));
        const LambdaNode L = a.nodes[node];
        vec3 ray_dir = pt::get_cast_dir(rng, fc, a.H, u, v);
        float sample = trace(wk, rng, L, fc.cam_pos, ray_dir);
        vec3 xyz = (sample * v3(L.rx, L.ry, L.rz)) * L.rcp_pdf;
        vec3 rgb = xyz_to_rgb_d65(xyz);
        acc_r += rgb.x; acc_g += rgb.y; acc_b += rgb.z;
        draws += rng.draws;
        if (MODE == 2) {
            float* q = a.debug_out + (size_t)pixel * 4;
            q[0] = sample; q[1] = L.wavelength; q[2] = (float)rng.draws; q[3] = (float)wk.vertices;
        }
    }
    if (MODE != 2) { px[0] = acc_r; px[1] = acc_g; px[2] = acc_b; }
    if (MODE == 1) pt::flush_work_counters(a.counters, (uint32_t)a.spp_count, wk.taps_r8, wk.taps_rgb, wk.sphere_steps, wk.tracking_steps, wk.vertices, draws);
}

}  // namespace

// ray_marcher (pathtracer.py:471-685) as its own kernel: the deterministic 64 x 16 march has fixed trip counts, so one
// lane = one pixel keeps the wave coherent through the march (only the sphere trace of intersect_land diverges); the
// gas densities come from the altitude table, the per-pixel RGB sum stays in registers over the launch's samples.
template <bool CLAMP, int MODE>
__global__ void __launch_bounds__(256) ray_march_kernel(RenderArgs a) {
    per_lane_body<MODE>(a, [&](Work& wk, Rng& rng, const LambdaNode& L, vec3 ray_pos, vec3 ray_dir) {
        return Tracer<CLAMP, true>(a, *a.fc, wk).ray_marcher(rng, L, ray_pos, ray_dir); });
}

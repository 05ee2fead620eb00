// legacy/render_kernel_v1.hip — kernel variant 1: pathtracer.path_tracer (pathtracer.py:316-469) as PER-LANE LOOPS, the straightforward statement of
// the integrator: every lane walks the reference's nested loops (250-step sphere trace, two delta-tracking loops, two ratio-tracking loops per
// light sample, 25 vertices) for its own pixel.  The 64 lanes of a wave serialise on each other's trip counts (11.5 % VALU lane utilisation,
// profiles/r1a_summary.md), which is why the product runs render_kernel_v2 / render_kernel_v6; this text stays as one more independent statement for
// the cross-check tests (tests/legacy/).  Built into the legacy library only (-DDE_LEGACY_VARIANTS), on the per-lane pieces and the kernel body of
// ../render_kernel.hip.
//
// Value-preserving difference from a literal transcription: tracking through Rayleigh/Mie/ozone does not tap the cloud map and tracking through
// the cloud shell does not evaluate the gas profiles: the reference multiplies those terms by an extinction of exactly 0
// (pathtracer.py:185,197), and x + 0*finite == x bit for bit.
#pragma once
#include "../render_kernel.hip"

namespace {

template <bool CLAMP>
struct PathTracer : Tracer<CLAMP> {
    using Base = Tracer<CLAMP>;
    using Base::a; using Base::fc; using Base::wk;
    using Base::intersect_land; using Base::land_normal; using Base::get_clouds_density; using Base::gas_density; using Base::get_land_material;
    __device__ PathTracer(const RenderArgs& a_, const FrameConsts& fc_, Work& wk_) : Base(a_, fc_, wk_) {}

    // pathtracer.py:77-115 with extinctions = (r, m, o, 0)
    DE_DEV void delta_tracking_rmo(Rng& rng, vec3 ray_pos, vec3 ray_dir, float t_start, float t_max, vec3 ext, float max_ext,
                                   int* event_out, float* t_out, int* id_out) {
        float t = t_start;
        const float inv_max = 1.0f / max_ext;      // contract 2: quotients by the majorant are products with RN(1 / majorant)
        ray_pos = ray_pos + t * ray_dir;
        int id = 0;
        int event = pt::EV_NULL;
        while (t < t_max) {
            float t_step = -de_log_unit(rng_next(rng)) * inv_max;
            ray_pos = ray_pos + t_step * ray_dir;
            t += t_step;
            wk.tracking_steps++;
            if (t >= t_max) break;
            vec3 es = ext * gas_density(ray_pos);
            float rand = rng_next(rng);
            float sum = (es.x + es.y) + es.z;
            if (rand < sum * inv_max) {
                float cmf = es.x;
                if (!(rand < cmf * inv_max)) {
                    id = 1;
                    cmf += es.y;
                    if (!(rand < cmf * inv_max)) {
                        id = 2;
                        cmf += es.z;
                        if (!(rand < cmf * inv_max)) id = 3;
                    }
                }
                const float albedo = (id == 0) ? 1.0f : ((id == 1) ? 0.95f : ((id == 2) ? 0.0f : 0.99f));   // pathtracer.py:263-270
                event = (rng_next(rng) < albedo) ? pt::EV_SCATTER : pt::EV_ABSORB;
                break;
            }
        }
        *event_out = event; *t_out = t; *id_out = id;
    }
    // pathtracer.py:77-115 with extinctions = (0, 0, 0, w): the species walk always ends at id 3
    DE_DEV void delta_tracking_cloud(Rng& rng, vec3 ray_pos, vec3 ray_dir, float t_start, float t_max, float ext_w, float max_ext,
                                     int* event_out, float* t_out) {
        float t = t_start;
        const float inv_max = 1.0f / max_ext;      // contract 2: quotients by the majorant are products with RN(1 / majorant)
        ray_pos = ray_pos + t * ray_dir;
        int event = pt::EV_NULL;
        while (t < t_max) {
            float t_step = -de_log_unit(rng_next(rng)) * inv_max;
            ray_pos = ray_pos + t_step * ray_dir;
            t += t_step;
            wk.tracking_steps++;
            if (t >= t_max) break;
            float es = ext_w * get_clouds_density(ray_pos);
            float rand = rng_next(rng);
            if (rand < es * inv_max) {
                event = (rng_next(rng) < 0.99f) ? pt::EV_SCATTER : pt::EV_ABSORB;
                break;
            }
        }
        *event_out = event; *t_out = t;
    }
    // pathtracer.py:117-143, gas part
    DE_DEV float ratio_tracking_rmo(Rng& rng, vec3 ray_pos, vec3 ray_dir, float t_start, float t_max, vec3 ext, float max_ext) {
        float t = t_start;
        const float inv_max = 1.0f / max_ext;      // contract 2: quotients by the majorant are products with RN(1 / majorant)
        ray_pos = ray_pos + t * ray_dir;
        float tr = 1.0f;
        while (t < t_max) {
            float t_step = -de_log_unit(rng_next(rng)) * inv_max;
            ray_pos = ray_pos + t_step * ray_dir;
            t += t_step;
            wk.tracking_steps++;
            if (t >= t_max) break;
            vec3 es = ext * gas_density(ray_pos);
            tr *= 1.0f - ((es.x + es.y) + es.z) * inv_max;
            if (tr < 1e-5f) break;
        }
        return tr;
    }
    // pathtracer.py:117-143, cloud part
    DE_DEV float ratio_tracking_cloud(Rng& rng, vec3 ray_pos, vec3 ray_dir, float t_start, float t_max, float ext_w, float max_ext) {
        float t = t_start;
        const float inv_max = 1.0f / max_ext;      // contract 2: quotients by the majorant are products with RN(1 / majorant)
        ray_pos = ray_pos + t * ray_dir;
        float tr = 1.0f;
        while (t < t_max) {
            float t_step = -de_log_unit(rng_next(rng)) * inv_max;
            ray_pos = ray_pos + t_step * ray_dir;
            t += t_step;
            wk.tracking_steps++;
            if (t >= t_max) break;
            float es = ext_w * get_clouds_density(ray_pos);
            tr *= 1.0f - es * inv_max;
            if (tr < 1e-5f) break;
        }
        return tr;
    }
    // pathtracer.py:172-207
    DE_DEV void sample_interaction(Rng& rng, vec3 ray_pos, vec3 ray_dir, float land_isection, vec3 ext, float ext_w,
                                   float max_ext_rmo, float max_ext_cloud, int* event_out, float* t_out, int* id_out) {
        vec2_ atmos = rsi(ray_pos, ray_dir, DE_ATMOS_UPPER);
        float t_start = de_max(0.0f, atmos.x);
        float t_max = (land_isection >= 0.0f) ? land_isection : atmos.y;
        if (atmos.y < 0.0f) t_max = -1.0f;
        int rmo_event, rmo_id;
        float rmo_t;
        delta_tracking_rmo(rng, ray_pos, ray_dir, t_start, t_max, ext, max_ext_rmo, &rmo_event, &rmo_t, &rmo_id);
        pt::intersect_cloud_limits(ray_pos, ray_dir, land_isection, &t_start, &t_max);
        int event = rmo_event;
        float t = rmo_t;
        int id = rmo_id;
        if (rmo_event == pt::EV_NULL || rmo_t > t_start) {
            int cloud_event;
            float cloud_t;
            delta_tracking_cloud(rng, ray_pos, ray_dir, t_start, t_max, ext_w, max_ext_cloud, &cloud_event, &cloud_t);
            if (cloud_event > 0 && (cloud_t < rmo_t || rmo_event == pt::EV_NULL)) {
                t = cloud_t;
                id = CLOUD_ID;
                event = cloud_event;
            }
        }
        *event_out = event; *t_out = t; *id_out = id;
    }
    // pathtracer.py:211-232
    DE_DEV float sample_transmittance(Rng& rng, vec3 ray_pos, vec3 ray_dir, float land_isection, vec3 ext, float ext_w,
                                      float max_ext_rmo, float max_ext_cloud) {
        vec2_ atmos = rsi(ray_pos, ray_dir, DE_ATMOS_UPPER);
        float t_start = de_max(0.0f, atmos.x);
        float t_max = (land_isection >= 0.0f) ? land_isection : atmos.y;
        if (atmos.y < 0.0f) t_max = -1.0f;
        float tr = ratio_tracking_rmo(rng, ray_pos, ray_dir, t_start, t_max, ext, max_ext_rmo);
        pt::intersect_cloud_limits(ray_pos, ray_dir, land_isection, &t_start, &t_max);
        tr *= ratio_tracking_cloud(rng, ray_pos, ray_dir, t_start, t_max, ext_w, max_ext_cloud);
        return tr;
    }
    // pathtracer.py:316-469
    DE_DEV float path_tracer(Rng& rng, const LambdaNode& L, vec3 ray_pos, vec3 ray_dir) {
        const vec3 primary_dir = ray_dir;
        vec3 ext = v3(L.ext_r, L.ext_m, L.ext_o);
        float ext_w = DE_CLOUDS_EXTINCT;
        bool primary_miss = false;
        float in_scattering = 0.0f;
        float throughput = 1.0f;
        for (int scatter_count = 0; scatter_count < 25; ++scatter_count) {
            wk.vertices++;
            if (scatter_count > 9) ext_w = 0.02f;
            float max_ext_rmo = L.max_ext_rmo;
            float max_ext_cloud = ext_w * DE_CLOUDS_DENSITY;
            float earth_intersection = intersect_land(ray_pos, ray_dir);
            int event, id;
            float interaction_dist;
            sample_interaction(rng, ray_pos, ray_dir, earth_intersection, ext, ext_w, max_ext_rmo, max_ext_cloud, &event, &interaction_dist, &id);
            if (scatter_count > 9 && id == CLOUD_ID) id = ISOTROPIC_CLOUD_ID;
            vec3 light_dir = tangent_space_apply(fc.light_dir, sample_cone(rng, fc.sun_cos_angle));
            if (event == pt::EV_ABSORB) {
                break;
            } else if (event == pt::EV_SCATTER) {
                vec3 ipos = ray_pos + interaction_dist * ray_dir;
                bool blocked = rsi(ipos, light_dir, DE_PLANET_R).y > 0.0f;
                float direct_tr = 0.0f;
                if (!blocked) direct_tr = sample_transmittance(rng, ipos, light_dir, -1.0f, ext, ext_w, max_ext_rmo, max_ext_cloud);
                float direct_phase = pt::evaluate_phase(fc, ray_dir, light_dir, id, scatter_count > 0);
                in_scattering += throughput * direct_tr * L.sun_irradiance * direct_phase;
                float phase_div_pdf;
                vec3 scatter_dir = pt::sample_phase(fc, rng, ray_dir, id, scatter_count > 0, &phase_div_pdf);
                ray_dir = scatter_dir;
                ray_pos = ipos;
                throughput *= phase_div_pdf;
            } else if (earth_intersection > 0.0f) {
                vec3 land_pos = ray_pos + ray_dir * earth_intersection;
                vec3 land_n = land_normal(land_pos);
                vec3 albedo_srgb;
                float ocean, bathy, emissive;
                get_land_material(land_pos, &albedo_srgb, &ocean, &bathy, &emissive);
                float albedo = pt::srgb_to_spectrum(L, albedo_srgb);
                in_scattering += throughput * emissive * L.night_power;
                vec3 offset_pos = land_pos * fc.offset_scale;
                bool visible = intersect_land(offset_pos, light_dir) < 0.0f;
                float direct_tr = sample_transmittance(rng, offset_pos, light_dir, visible ? -1.0f : 0.0f, ext, ext_w, max_ext_rmo, max_ext_cloud);
                float direct_ndl;
                float direct_brdf = earth_brdf(albedo, ocean, bathy, -ray_dir, land_n, light_dir, &direct_ndl);
                in_scattering += throughput * direct_tr * (visible ? 1.0f : 0.0f) * L.sun_irradiance * direct_brdf * direct_ndl;
                vec3 view_dir = -ray_dir;
                ray_dir = sample_hemisphere_cosine_weighted(rng, land_n);
                ray_pos = offset_pos;
                float unused;
                float brdf = earth_brdf(albedo, ocean, bathy, view_dir, land_n, ray_dir, &unused);
                throughput *= brdf * (float)M_PI;
            } else {
                if (scatter_count == 0) primary_miss = true;
                break;
            }
            if (scatter_count > 3) {
                float termination_p = de_max(0.05f, 1.0f - throughput);
                if (rng_next(rng) < termination_p) break;
                throughput /= 1.0f - termination_p;
            }
        }
        if (primary_miss) {
            if (dot(fc.light_dir, primary_dir) > fc.sun_cos_angle) in_scattering += L.sun_power;
            wk.taps_rgb += 1;
            in_scattering += pt::stars_term(L, sphere_tap_rgb<CLAMP>(a.stars, normalized(primary_dir)));
        }
        return pt::clean_radiance(in_scattering);
    }
};

}  // namespace

template <bool CLAMP, int MODE>
__global__ void __launch_bounds__(256) render_kernel(RenderArgs a) {
    per_lane_body<MODE>(a, [&](Work& wk, Rng& rng, const LambdaNode& L, vec3 ray_pos, vec3 ray_dir) {
        return PathTracer<CLAMP>(a, *a.fc, wk).path_tracer(rng, L, ray_pos, ray_dir); });
}

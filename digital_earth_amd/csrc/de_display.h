// de_display.h — the host side of the display path: what runs on the context stream between the frame's sums and the image a caller is handed.
//   * the small helpers every entry point of that path shares: host <-> device layouts, a transposed fetch, a settings getter, device scratch buffers
//     (how an output leaves the GPU — staging, the rings, the packed outputs' conversion frame — is de_fetch.h);
//   * each opt-in stage's allocation and launch sequence (denoiser, auto-exposure, bloom, history reprojection, local exposure), the stages behind the
//     display (look LUTs, output scaling, 8-bit and HDR pixels, video frames, JPEG streams) and the two refusals;
//   * display_chain: the ONE statement of the order denoise -> history -> meter -> bloom -> local exposure -> display and of its preconditions, which
//     de_render_to_image and the four intermediate fetches of de_api.hip run up to their own stage.
// The kernels are in *_kernels.hip; the tent pyramid the bloom and local exposure share is pyramid.h, what the packed outputs share pack.h, the source
// every stage reads display_source.h.
#pragma once
#include "de_fetch.h"
#include "../../include/digital_earth_denoise.h"

namespace {
// ---- layouts.  The host's arrays are (W, H, k), u outermost (the reference's fields); the device's are [H][W][k].
template <class T>
void to_device_layout(const T* host, T* dev, int W, int H, int k) {
    for (int i = 0; i < W; ++i)
        for (int j = 0; j < H; ++j)
            for (int ch = 0; ch < k; ++ch) dev[((size_t)j * W + i) * k + ch] = host[((size_t)i * H + j) * k + ch];
}
template <class T>
void to_host_layout(const T* dev, T* host, int W, int H, int k) {
    for (int i = 0; i < W; ++i)
        for (int j = 0; j < H; ++j)
            for (int ch = 0; ch < k; ++ch) host[((size_t)i * H + j) * k + ch] = dev[((size_t)j * W + i) * k + ch];
}
dim3 tiles16(int w, int h) { return dim3((unsigned)((w + 15) / 16), (unsigned)((h + 15) / 16)); }
dim3 tiles32(const de_ctx* c) { return dim3((unsigned)((c->W + 31) / 32), (unsigned)((c->H + 31) / 32)); }
// A device [H][W][3] buffer to the caller's (W, H, 3) array: transposed into d_scratch on the context stream, then copied out.  Ends in frame_status.
int fetch_transposed(de_ctx* c, const float* d_src, float* out) {
    hipLaunchKernelGGL(hdr_transpose_kernel, tiles32(c), dim3(256), 0, c->stream, d_src, c->d_scratch, c->W, c->H);
    HIP_TRY(hipGetLastError());
    return copy_out(c, out, c->d_scratch);
}
// de_get_<stage>: the settings while the stage is on, zeros while it is off; struct_bytes always.
template <class S>
int get_settings(de_ctx* c, bool de_ctx::*on, S de_ctx::*settings, S* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (c->*on) *out = c->*settings; else memset(out, 0, sizeof(*out));
    out->struct_bytes = (uint32_t)sizeof(S);
    return DE_OK;
}
// A debug entry point's round trip on `stream`: N device buffers of its own (bytes[k] each; 0: none, the launch sees a null pointer), in[k] uploaded
// into buffer k where given, `launch(buffers)` and its launch error, buffer `result` downloaded into `out`, and a wait.  Freed on every exit path.
template <int N, class Launch>
int debug_round_trip(hipStream_t stream, const size_t (&bytes)[N], const void* const (&in)[N], int result, void* out, Launch launch) {
    Dev<void> b[N];
    void* p[N] = {};      // what the launch sees
    for (int k = 0; k < N; ++k) if (bytes[k]) { HIP_TRY(b[k].ensure(bytes[k])); p[k] = b[k]; }
    for (int k = 0; k < N; ++k) if (in[k]) HIP_TRY(hipMemcpyAsync(p[k], in[k], bytes[k], hipMemcpyHostToDevice, stream));
    HIP_TRY(launch(p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, p[result], bytes[result], hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return DE_OK;
}

// ---- the source (display_source.h) of a display launch's arguments
DisplaySrc display_src(const DisplayArgs& d, bool per_tile) {
    DisplaySrc s;
    s.hdr = d.hdr; s.tile_spp = per_tile ? d.tile_spp : nullptr; s.samples = d.samples; s.W = d.W; s.H = d.H;
    return s;
}
// 16-byte aligned: the kernels' float4 loads (the context's own buffers always are; a bound buffer or a display source may not be)
bool src_aligned(const DisplaySrc& s) { return (reinterpret_cast<uintptr_t>(s.hdr) & 15u) == 0u; }

// ---- the denoiser (include/digital_earth_denoise.h, denoise_kernels.hip)
int denoise_refusal(de_ctx* c) {
    if (c->tiles_world > 1) return fail(DE_ERR_STATE, "the denoiser filters whole frames: not under a tile partition");
    if (c->sample_world > 1) return fail(DE_ERR_STATE, "the denoiser filters whole frames: not under a sample partition");
    if (c->display_src) return fail(DE_ERR_STATE, "the denoiser filters this context's own frame: not with a display source or after de_reduce_progressive");
    return DE_OK;
}
// ---- the HDR display output (include/digital_earth_hdr_output.h, hdr_output_kernels.hip)
int hdr_output_refusal(de_ctx* c) {
    if (c->p.flags & DE_FLAG_AGX) return fail(DE_ERR_STATE, "the HDR display output runs OpenDRT: not with DE_FLAG_AGX, an SDR transform");
    return DE_OK;
}
// the guides alone: what guide_kernel writes (the history reprojection reads their distance without the denoiser's other buffers)
int dn_alloc_guides(de_ctx* c) {
    const size_t npx = (size_t)c->W * c->H;
    HIP_TRY(c->d_dn_nc.ensure(npx * sizeof(float4)));
    HIP_TRY(c->d_dn_at.ensure(npx * sizeof(float4)));
    HIP_TRY(c->d_dn_dist.ensure(npx * sizeof(float)));
    return DE_OK;
}
int dn_alloc(de_ctx* c) {
    const size_t npx = (size_t)c->W * c->H;
    { int rc = dn_alloc_guides(c); if (rc) return rc; }
    for (int k = 0; k < 2; ++k) HIP_TRY(c->d_dn_buf[k].ensure(npx * sizeof(float4)));
    HIP_TRY(c->d_dn_out.ensure(npx * 3 * sizeof(float)));
    return DE_OK;
}
DenoiseGuides dn_guides(de_ctx* c) { DenoiseGuides g; g.nc = c->d_dn_nc; g.at = c->d_dn_at; g.dist = c->d_dn_dist; return g; }
dim3 dn_grid(de_ctx* c) { return tiles16(c->W, c->H); }
// The guides of the current camera, maps and address mode: once per frame (de_reset, a map or a camera change clears them).
int dn_ensure_guides(de_ctx* c) {
    int rc = dn_alloc_guides(c);
    if (rc) return rc;
    if (c->dn_guides_valid) return DE_OK;
    RenderArgs a;
    rc = fill_render_args(c, &a);          // packs the maps and rebuilds the frame constants if needed
    if (rc) return rc;
    if (c->p.flags & DE_FLAG_CLAMP_SAMPLER) hipLaunchKernelGGL(guide_kernel<true>, dn_grid(c), dim3(256), 0, c->stream, a, dn_guides(c));
    else hipLaunchKernelGGL(guide_kernel<false>, dn_grid(c), dim3(256), 0, c->stream, a, dn_guides(c));
    HIP_TRY(hipGetLastError());
    c->dn_guides_valid = true;
    return DE_OK;
}
// The a-trous levels over d_dn_buf[1] (colour, variance); the last one also writes the filtered mean to d_dn_out.  Returns the buffer that holds the result.
int dn_levels(de_ctx* c, int levels, float sigma_l, float4** result) {
    AtrousArgs t;
    t.g = dn_guides(c); t.W = c->W; t.H = c->H; t.sigma_l = sigma_l;
    int cur = 1;
    for (int l = 0; l < levels; ++l) {
        t.in = c->d_dn_buf[cur]; t.out = c->d_dn_buf[cur ^ 1]; t.step = 1 << l;
        t.out3 = l == levels - 1 ? c->d_dn_out : nullptr;
        hipLaunchKernelGGL(atrous_kernel, dn_grid(c), dim3(256), 0, c->stream, t);
        HIP_TRY(hipGetLastError());
        cur ^= 1;
    }
    *result = c->d_dn_buf[cur];
    return DE_OK;
}
// The frame's filtered mean into d_dn_out, on the context stream (the caller has joined the launch slots and marked the HDR buffer as read).
// Variance source: the per-pixel estimate from S2 when S2 is complete and the pixel has n >= 4 samples, else the 7x7 spatial estimate.
int run_denoise(de_ctx* c) {
    int rc = dn_alloc(c);
    if (rc) return rc;
    rc = dn_ensure_guides(c);
    if (rc) return rc;
    DenoisePrepArgs pa;
    const bool adaptive = c->frame_kind == DE_FRAME_ADAPTIVE;
    pa.s1 = c->display_src ? c->display_src : c->d_hdr;
    pa.s2 = (c->dn_s2_complete || adaptive) ? c->d_s2 : nullptr;
    pa.tile_spp = adaptive ? c->d_tile_spp : nullptr;
    pa.spp = c->current_spp; pa.W = c->W; pa.H = c->H; pa.out = c->d_dn_buf[0];
    hipLaunchKernelGGL(prep_mean_kernel, dn_grid(c), dim3(256), 0, c->stream, pa);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(prep_spatial_kernel, dn_grid(c), dim3(256), 0, c->stream, (const float4*)c->d_dn_buf[0], c->d_dn_buf[1], c->W, c->H);
    HIP_TRY(hipGetLastError());
    float4* res = nullptr;
    rc = dn_levels(c, c->dn_levels, c->dn_sigma_l, &res);
    if (rc) return rc;
    c->dn_out_valid = true;
    return DE_OK;
}
// ---- auto-exposure (include/digital_earth_exposure.h, exposure_kernels.hip)
int ae_alloc(de_ctx* c) {
    HIP_TRY(c->d_ae_partial.ensure((size_t)AE_MAX_WG * AE_ROW * sizeof(uint32_t)));
    HIP_TRY(c->d_ae_state.ensure(sizeof(MeterState)));
    HIP_TRY(c->d_fc_ae.ensure(sizeof(FrameConsts)));
    HIP_TRY(c->d_ae_result.ensure(sizeof(MeterResult)));
    if (!c->d_ae_centre) {
        // log2 of the bins' centres: bin k = octave (k >> 3) - 24, sub-bin k & 7 of 8 linear ones; uploaded once, so that the device computes no logarithm
        double centre[AE_BINS];
        for (int k = 0; k < AE_BINS; ++k) centre[k] = (double)((k >> 3) - 24) + log2(1.0 + ((double)(k & 7) + 0.5) / 8.0);
        HIP_TRY(c->d_ae_centre.ensure(sizeof(centre)));
        HIP_TRY(hipMemcpyAsync(c->d_ae_centre, centre, sizeof(centre), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));      // the table is a local: once per context, when the feature is first turned on, never in a display
    }
    return DE_OK;
}
// The two metering kernels on the context stream, over exactly what the display launch `d` is about to read (per_tile: display_kernel<true>).
int run_meter(de_ctx* c, const DisplayArgs& d, bool per_tile) {
    const de_auto_exposure& s = c->ae;
    const bool whole = !(s.region[0] | s.region[1] | s.region[2] | s.region[3]);
    MeterArgs m;
    m.s = display_src(d, per_tile);
    m.x0 = whole ? 0 : s.region[0]; m.y0 = whole ? 0 : s.region[1]; m.x1 = whole ? c->W : s.region[2]; m.y1 = whole ? c->H : s.region[3];
    m.gx0 = m.x0 >> 2; m.gw = ((m.x1 + 3) >> 2) - m.gx0;
    const unsigned long long items = (unsigned long long)m.gw * (unsigned long long)(m.y1 - m.y0);      // at most the region's pixels
    if ((unsigned long long)(m.x1 - m.x0) * (unsigned long long)(m.y1 - m.y0) >= (1ull << 31))
        return fail(DE_ERR_INVALID, "the metering region must hold fewer than 2^31 pixels (the counts and the item index are 32-bit)");
    m.n_items = (uint32_t)items;
    m.partial = c->d_ae_partial;
    const unsigned n_wg = (unsigned)std::min<unsigned long long>((items + 255ull) / 256ull, (unsigned long long)AE_MAX_WG);
    if (src_aligned(m.s)) hipLaunchKernelGGL(meter_hist_kernel<true>, dim3(n_wg), dim3(256), 0, c->stream, m);
    else hipLaunchKernelGGL(meter_hist_kernel<false>, dim3(n_wg), dim3(256), 0, c->stream, m);
    HIP_TRY(hipGetLastError());
    MeterSolveArgs v;
    v.partial = c->d_ae_partial; v.n_rows = (int)n_wg;
    v.low = s.low_fraction; v.high = s.high_fraction; v.adapt = s.adapt; v.compensation = s.compensation; v.ev_min = s.ev_min; v.ev_max = s.ev_max;
    v.manual = c->p.exposure;
    v.log2_key = log2((double)s.key);
    v.centre = c->d_ae_centre; v.state = c->d_ae_state; v.fc = c->d_fc; v.fc_ae = c->d_fc_ae; v.res = c->d_ae_result;
    hipLaunchKernelGGL(meter_solve_kernel, dim3(1), dim3(1024), 0, c->stream, v);
    HIP_TRY(hipGetLastError());
    c->ae_displayed = true;
    return DE_OK;
}
// ---- bloom (include/digital_earth_bloom.h, bloom_kernels.hip).  d_bl_pyr holds D_l at the plan's off[l] and U_l `total` further, in float4.
int bl_alloc(de_ctx* c) {
    const PyramidPlan p = pyr_plan(c->W, c->H, BL_MAX_LEVELS);      // room for every setting of `levels`: the offsets of a level do not depend on it
    HIP_TRY(c->d_bl_pyr.ensure(2 * p.total * sizeof(float4)));
    HIP_TRY(c->d_bl_out.ensure((size_t)c->W * c->H * 3 * sizeof(float)));
    return DE_OK;
}
// The bloom kernels on the context stream, over exactly what the display launch `d` is about to read (per_tile: display_kernel<true>).  Afterwards `d`
// describes the composited mean: the unchanged display_kernel<false> with samples = 1 (x / 1.0f == x).
int run_bloom(de_ctx* c, DisplayArgs& d, bool& per_tile) {
    const de_bloom& b = c->bl;
    const PyramidPlan p = pyr_plan(c->W, c->H, b.levels);
    float4* D = c->d_bl_pyr;
    float4* U = c->d_bl_pyr + pyr_plan(c->W, c->H, BL_MAX_LEVELS).total;
    BloomSrc s;
    static_cast<DisplaySrc&>(s) = display_src(d, per_tile);
    s.threshold = b.threshold; s.knee = b.knee; s.clamp = b.clamp;
    const bool vec = src_aligned(s);
    if (vec) hipLaunchKernelGGL(bloom_down0_kernel<true>, tiles16(p.w[1], p.h[1]), dim3(256), 0, c->stream, s, D + p.off[1], p.w[1], p.h[1]);
    else hipLaunchKernelGGL(bloom_down0_kernel<false>, tiles16(p.w[1], p.h[1]), dim3(256), 0, c->stream, s, D + p.off[1], p.w[1], p.h[1]);
    HIP_TRY(hipGetLastError());
    for (int l = 1; l < p.L; ++l) {
        hipLaunchKernelGGL(bloom_down_kernel, tiles16(p.w[l + 1], p.h[l + 1]), dim3(256), 0, c->stream, (const float4*)(D + p.off[l]), p.w[l], p.h[l], D + p.off[l + 1], p.w[l + 1], p.h[l + 1]);
        HIP_TRY(hipGetLastError());
    }
    const float4* top = D + p.off[p.L];      // U_L = D_L
    for (int l = p.L - 1; l >= 1; --l) {
        BloomUpArgs u;
        u.coarse = top; u.fine = D + p.off[l]; u.out = U + p.off[l];
        u.Wc = p.w[l + 1]; u.Hc = p.h[l + 1]; u.Wf = p.w[l]; u.Hf = p.h[l];
        u.keep = 1.0f - b.spread; u.spread = b.spread;
        hipLaunchKernelGGL(bloom_up_kernel, tiles16(p.w[l], p.h[l]), dim3(256), 0, c->stream, u);
        HIP_TRY(hipGetLastError());
        top = u.out;
    }
    // level 0 is not blended in: the glow never holds the unblurred image
    const unsigned n_wg = (unsigned)(((size_t)(c->W >> 2) * (size_t)c->H + 255u) / 256u);
    if (vec) hipLaunchKernelGGL(bloom_composite_kernel<true>, dim3(n_wg), dim3(256), 0, c->stream, s, top, p.w[1], p.h[1], b.intensity, c->d_bl_out);
    else hipLaunchKernelGGL(bloom_composite_kernel<false>, dim3(n_wg), dim3(256), 0, c->stream, s, top, p.w[1], p.h[1], b.intensity, c->d_bl_out);
    HIP_TRY(hipGetLastError());
    d.hdr = c->d_bl_out; d.samples = 1; per_tile = false;
    return DE_OK;
}
// ---- history reprojection (include/digital_earth_history.h, history_kernels.hip)
int hs_alloc(de_ctx* c) {
    const size_t npx = (size_t)c->W * c->H;
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(c->d_hs_c[k].ensure(npx * sizeof(float4)));
        HIP_TRY(c->d_hs_d[k].ensure(npx * sizeof(float)));
        HIP_TRY(c->d_hs_cam[k].ensure(sizeof(HistoryCam)));
    }
    HIP_TRY(c->d_hs_out.ensure(npx * 3 * sizeof(float)));
    return DE_OK;
}
// All weights 0: neither the history nor a candidate written before this point is read again (host flags: the buffers need no clearing).
void hs_drop(de_ctx* c) { c->hs_valid = false; c->hs_cand_valid = false; }
// Does the step from de_params a to b change radiance?  Camera fields reproject; exposure, gamma, CRF, vignette and DE_FLAG_AGX are display-only.
bool hs_radiance_changed(const de_params& a, const de_params& b) {
    return memcmp(&a.sun_angle, &b.sun_angle, sizeof(float)) != 0 || memcmp(&a.sun_path_rot, &b.sun_path_rot, sizeof(float)) != 0 ||
           memcmp(&a.land_height_scale, &b.land_height_scale, sizeof(float)) != 0 || memcmp(&a.fixed_wavelength, &b.fixed_wavelength, sizeof(float)) != 0 ||
           a.topo_res_override != b.topo_res_override || ((a.flags ^ b.flags) & ~(uint32_t)DE_FLAG_AGX) != 0u;
}
// The blend on the context stream, over exactly what the display launch `d` is about to read (per_tile: display_kernel<true>).  Afterwards `d` describes
// the blended mean: the unchanged display_kernel<false> with samples = 1 (x / 1.0f == x).  The same launch writes the next history candidate.
int run_history(de_ctx* c, DisplayArgs& d, bool& per_tile) {
    int rc = hs_alloc(c);
    if (rc) return rc;
    rc = dn_ensure_guides(c);      // the distance of the current camera: once per frame, shared with the denoiser
    if (rc) return rc;
    const int cur = c->hs_cur, cand = cur ^ 1;
    HistoryArgs a;
    a.s = display_src(d, per_tile);
    a.n_tile = c->frame_kind == DE_FRAME_ADAPTIVE ? c->d_tile_spp : nullptr; a.n_pixel = nullptr; a.n_frame = c->current_spp;
    a.dist = c->d_dn_dist; a.fc = c->d_fc;
    a.hist_c = c->hs_valid ? c->d_hs_c[cur] : nullptr; a.hist_d = c->d_hs_d[cur]; a.hist_cam = c->d_hs_cam[cur];
    a.out = c->d_hs_out; a.cand_c = c->d_hs_c[cand]; a.cand_d = c->d_hs_d[cand]; a.cand_cam = c->d_hs_cam[cand];
    a.max_history = c->hs.max_history; a.depth_tolerance = c->hs.depth_tolerance;
    hipLaunchKernelGGL(history_blend_kernel, dn_grid(c), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    c->hs_cand_valid = true;
    d.hdr = c->d_hs_out; d.samples = 1; per_tile = false;
    return DE_OK;
}
// ---- local exposure (include/digital_earth_local_exposure.h, local_exposure_kernels.hip)
int lx_alloc(de_ctx* c) {
    const PyramidPlan p = pyr_plan(c->W, c->H, LX_MAX_LEVELS);      // room for every setting of `levels`: the offsets of a level do not depend on it
    HIP_TRY(c->d_lx_pyr.ensure(p.total * sizeof(float2)));
    HIP_TRY(c->d_lx_base.ensure(p.total * sizeof(float)));
    HIP_TRY(c->d_lx_out.ensure((size_t)c->W * c->H * 3 * sizeof(float)));
    return DE_OK;
}
int lx_settings_check(const de_local_exposure* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_local_exposure)) return fail(DE_ERR_INVALID, "de_local_exposure.struct_bytes does not match this library's struct");
    if (!(s->highlights >= 0.0f) || !(s->highlights <= 1.0f) || !(s->shadows >= 0.0f) || !(s->shadows <= 1.0f))
        return fail(DE_ERR_INVALID, "local exposure settings: highlights and shadows in [0, 1]");
    if (!(s->sigma > 0.0f) || !(s->sigma < 1e30f) || !(s->max_ev >= 0.0f) || !(s->max_ev < 1e30f) || !(s->key > 0.0f) || !(s->key < 1e30f))
        return fail(DE_ERR_INVALID, "local exposure settings: finite sigma > 0, finite max_ev >= 0, finite key > 0");
    if (s->levels < 1 || s->levels > LX_MAX_LEVELS) return fail(DE_ERR_INVALID, "local exposure settings: levels in 1 .. 10");
    return DE_OK;
}
// The kernels on the context stream with the settings `x`, over exactly what the display launch `d` is about to read (per_tile: display_kernel<true>)
// and with the anchor from d.fc (the metered FrameConsts while auto-exposure is on: no host round trip).  Afterwards `d` describes the dodged mean: the
// unchanged display_kernel<false> with samples = 1 (x / 1.0f == x).
int lx_run(de_ctx* c, const de_local_exposure& x, DisplayArgs& d, bool& per_tile) {
    const PyramidPlan p = pyr_plan(c->W, c->H, x.levels);
    float2* D = c->d_lx_pyr;
    float* B = c->d_lx_base;
    const DisplaySrc s = display_src(d, per_tile);
    const bool vec = src_aligned(s);
    const float inv_sigma = 1.0f / x.sigma;
    if (vec) hipLaunchKernelGGL(lx_down0_kernel<true>, tiles16(p.w[1], p.h[1]), dim3(256), 0, c->stream, s, D + p.off[1], p.w[1], p.h[1]);
    else hipLaunchKernelGGL(lx_down0_kernel<false>, tiles16(p.w[1], p.h[1]), dim3(256), 0, c->stream, s, D + p.off[1], p.w[1], p.h[1]);
    HIP_TRY(hipGetLastError());
    for (int l = 1; l < p.L; ++l) {
        hipLaunchKernelGGL(lx_down_kernel, tiles16(p.w[l + 1], p.h[l + 1]), dim3(256), 0, c->stream, (const float2*)(D + p.off[l]), p.w[l], p.h[l], D + p.off[l + 1], p.w[l + 1], p.h[l + 1]);
        HIP_TRY(hipGetLastError());
    }
    const float* top = nullptr;      // B_L is the top level's guide: not stored
    for (int l = p.L - 1; l >= 1; --l) {
        LxUpArgs u;
        u.fine = D + p.off[l]; u.coarse = D + p.off[l + 1]; u.coarse_b = top; u.out = B + p.off[l];
        u.Wc = p.w[l + 1]; u.Hc = p.h[l + 1]; u.Wf = p.w[l]; u.Hf = p.h[l]; u.inv_sigma = inv_sigma;
        hipLaunchKernelGGL(lx_up_kernel, dim3((unsigned)(((size_t)u.Wf * (size_t)u.Hf + 255u) / 256u)), dim3(256), 0, c->stream, u);
        HIP_TRY(hipGetLastError());
        top = u.out;
    }
    LxApplyArgs a;
    a.s = s; a.d1 = D + p.off[1]; a.b1 = top; a.W1 = p.w[1]; a.H1 = p.h[1]; a.fc = d.fc;
    a.highlights = x.highlights; a.shadows = x.shadows; a.inv_sigma = inv_sigma; a.max_ev = x.max_ev; a.key = x.key; a.out = c->d_lx_out;
    const unsigned n_wg = (unsigned)(((size_t)(c->W >> 2) * (size_t)c->H + 255u) / 256u);
    if (vec) hipLaunchKernelGGL(lx_apply_kernel<true>, dim3(n_wg), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(lx_apply_kernel<false>, dim3(n_wg), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    d.hdr = c->d_lx_out; d.samples = 1; per_tile = false;
    return DE_OK;
}
int run_local_exposure(de_ctx* c, DisplayArgs& d, bool& per_tile) { return lx_run(c, c->lx, d, per_tile); }
// ---- output scaling (include/digital_earth_output_scale.h, output_scale_kernels.hip): every call that hands out the displayed image sizes itself from these
bool os_active(const de_ctx* c) { return c->os.enabled && c->os.width > 0 && (c->os.width != c->W || c->os.height != c->H); }      // on at W x H is the identity: nothing runs
// the panorama (include/digital_earth_panorama.h, below) stands in the same place; de_set_output_scale and de_set_panorama refuse each other, so at most one of the two is on
int out_w(const de_ctx* c) { return c->pano.on ? c->pano.width : os_active(c) ? c->os.width : c->W; }
int out_h(const de_ctx* c) { return c->pano.on ? c->pano.height : os_active(c) ? c->os.height : c->H; }
size_t out_image_bytes(const de_ctx* c) { return (size_t)out_w(c) * (size_t)out_h(c) * 3 * sizeof(float); }
const float* shown_image(const de_ctx* c) { return c->pano.on ? c->pano_out : os_active(c) ? c->os_out : c->d_image; }
// The settings against a source size; *ow, *oh = the output size they ask for (0, 0: the source's).
int os_settings_check(const de_output_scale* s, int W, int H, int* ow, int* oh) {
    if (s->struct_bytes != (uint32_t)sizeof(de_output_scale)) return fail(DE_ERR_INVALID, "de_output_scale.struct_bytes does not match this library's struct");
    if (s->filter < DE_SCALE_BOX || s->filter > DE_SCALE_LANCZOS3) return fail(DE_ERR_INVALID, "de_output_scale.filter must be DE_SCALE_BOX, _TRIANGLE, _MITCHELL or _LANCZOS3");
    const int w = (s->width == 0 && s->height == 0) ? W : s->width, h = (s->width == 0 && s->height == 0) ? H : s->height;
    if (w <= 0 || h <= 0 || (w % 16) != 0 || (h % 8) != 0) return fail(DE_ERR_INVALID, "de_output_scale: width must be a positive multiple of 16 and height of 8");
    if ((long long)w * 8 < W || (long long)W * 8 < w || (long long)h * 8 < H || (long long)H * 8 < h) return fail(DE_ERR_INVALID, "de_output_scale: each axis' ratio out / source must lie in [1/8, 8]");
    if ((long long)w * h > (1ll << 28)) return fail(DE_ERR_INVALID, "de_output_scale: width * height must not exceed 2^28");
    *ow = w; *oh = h;
    return DE_OK;
}
// One axis' table on the device, rebuilt only when the axis or the filter changed.  The upload reads pageable host memory that dies with this call: waited for.
int os_table_ensure(hipStream_t stream, de_ctx::ScaleDev& d, int n_src, int n_dst, int filter) {
    if (d.first && d.n_src == n_src && d.n_dst == n_dst && d.filter == filter) return DE_OK;
    ScaleTable T;
    if (!os_build_table(n_src, n_dst, filter, &T)) return fail(DE_ERR_INVALID, "output scaling: no table for this pair of sizes");
    int rc = d.first.ensure(T.first.size() * sizeof(int32_t), "output scaling's buffers");
    if (rc) return rc;
    rc = d.w.ensure(T.w.size() * sizeof(float), "output scaling's buffers");
    if (rc) return rc;
    d.filter = -1;
    HIP_TRY(hipMemcpyAsync(d.first, T.first.data(), T.first.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d.w, T.w.data(), T.w.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    d.n_src = n_src; d.n_dst = n_dst; d.filter = filter; d.taps = T.taps;
    return DE_OK;
}
// The passes of (W, H, 3) -> (ow, oh, 3), not both sizes equal: along v into `mid` (or straight into `out` when the other axis is a copy), then along u.
int os_launch(hipStream_t stream, const float* src, int W, int H, int ow, int oh, const de_ctx::ScaleDev& tv, const de_ctx::ScaleDev& tu, float* mid, float* out) {
    const float* in = src;
    if (oh != H) {
        ScaleArgs a;
        a.src = in; a.dst = ow != W ? mid : out; a.first = tv.first; a.w = tv.w; a.n_src = H; a.n_dst = oh; a.taps = tv.taps; a.lines = W; a.clamp = ow != W ? 0 : 1;
        const unsigned long long blocks = (unsigned long long)W * (unsigned long long)os_v_tiles(oh);
        if (blocks * OS_V_THREADS >= (1ull << 32)) return fail(DE_ERR_INVALID, "output scaling: the image has too many columns for one launch");
        hipLaunchKernelGGL(output_scale_v_kernel, dim3((unsigned)blocks), dim3(OS_V_THREADS), 0, stream, a);
        HIP_TRY(hipGetLastError());
        in = a.dst;
    }
    if (ow != W) {
        ScaleArgs a;
        a.src = in; a.dst = out; a.first = tu.first; a.w = tu.w; a.n_src = W; a.n_dst = ow; a.taps = tu.taps; a.lines = oh * 3; a.clamp = 1;
        const unsigned long long blocks = (unsigned long long)ow * (unsigned long long)os_u_chunks(oh * 3);
        if (blocks * OS_U_THREADS >= (1ull << 32)) return fail(DE_ERR_INVALID, "output scaling: the output has too many columns for one launch");
        hipLaunchKernelGGL(output_scale_u_kernel, dim3((unsigned)blocks), dim3(OS_U_THREADS), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return DE_OK;
}
// Behind the display on the context stream: d_image -> os_out.
int run_output_scale(de_ctx* c) {
    const int W = c->W, H = c->H, ow = c->os.width, oh = c->os.height;
    int rc = DE_OK;
    if (oh != H) { rc = os_table_ensure(c->stream, c->os_tab[0], H, oh, c->os.filter); if (rc) return rc; }
    if (ow != W) { rc = os_table_ensure(c->stream, c->os_tab[1], W, ow, c->os.filter); if (rc) return rc; }
    if (oh != H && ow != W) { rc = c->os_mid.ensure((size_t)W * (size_t)oh * 3 * sizeof(float), "output scaling's buffers"); if (rc) return rc; }
    rc = c->os_out.ensure((size_t)ow * (size_t)oh * 3 * sizeof(float), "output scaling's buffers");
    if (rc) return rc;
    return os_launch(c->stream, c->d_image, W, H, ow, oh, c->os_tab[0], c->os_tab[1], c->os_mid, c->os_out);
}
// ---- the panorama output (include/digital_earth_panorama.h, panorama_kernels.hip, panorama_body.h)
// The settings against a face size N (the context's W = H, or de_debug_panorama's n).
int pano_settings_check(const de_panorama* s, int N) {
    if (s->struct_bytes != (uint32_t)sizeof(de_panorama)) return fail(DE_ERR_INVALID, "de_panorama.struct_bytes does not match this library's struct");
    if (s->projection != DE_PANO_EQUIRECT && s->projection != DE_PANO_FISHEYE) return fail(DE_ERR_INVALID, "de_panorama.projection must be DE_PANO_EQUIRECT or DE_PANO_FISHEYE");
    if (s->width <= 0 || s->height <= 0 || (s->width % 16) != 0 || (s->height % 8) != 0) return fail(DE_ERR_INVALID, "de_panorama: width must be a positive multiple of 16 and height of 8");
    if ((long long)s->width * s->height > (1ll << 28)) return fail(DE_ERR_INVALID, "de_panorama: width * height must not exceed 2^28");
    if (s->projection == DE_PANO_FISHEYE) {
        if (s->width != s->height) return fail(DE_ERR_INVALID, "de_panorama: a fisheye frame needs width == height");
        if (!(s->aperture_deg > 0.0f && s->aperture_deg <= 360.0f)) return fail(DE_ERR_INVALID, "de_panorama.aperture_deg must lie in (0, 360]");      // NaN fails both
    }
    if (s->apron < 1 || s->apron > N / 4) return fail(DE_ERR_INVALID, "de_panorama.apron must lie in 1 ... N / 4");
    if (s->supersample < 1 || s->supersample > PANO_MAX_S) return fail(DE_ERR_INVALID, "de_panorama.supersample must lie in 1 ... 4");
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += (double)s->basis[3 * i + k] * (double)s->basis[3 * j + k];
            if (!(fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-4)) return fail(DE_ERR_INVALID, "de_panorama.basis must be orthonormal within 1e-4");      // NaN fails
        }
    return DE_OK;
}
// The header's face table: look and up of face 0 ... 5 from basis = r, u, f, in double.
void pano_face_frame(const float* basis, int face, double look[3], double up[3]) {
    static const int look_of[6] = {0, 0, 1, 1, 2, 2}, up_of[6] = {1, 1, 2, 2, 1, 1};
    static const double look_sign[6] = {1, -1, 1, -1, 1, -1}, up_sign[6] = {1, 1, -1, 1, 1, 1};
    for (int k = 0; k < 3; ++k) { look[k] = look_sign[face] * (double)basis[3 * look_of[face] + k]; up[k] = up_sign[face] * (double)basis[3 * up_of[face] + k]; }
}
// What the kernel reads of the settings beside the sizes: fov, scale, the half aperture and every face's m, as the header defines them.
void pano_make_consts(const de_panorama& s, int N, PanoArgs* k) {
    const double pi = 3.14159265358979323846;
    k->fov = (float)((double)N / (double)(N - 2 * s.apron));
    k->scale = (float)((double)N / (2.0 * (double)k->fov));
    k->half_aperture = (float)((double)s.aperture_deg * pi / 360.0);
    for (int face = 0; face < 6; ++face) {
        double d[3], up[3], du[3], dv[3];
        pano_face_frame(s.basis, face, d, up);
        auto cross = [](const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; };
        auto normalize = [](double* v) { const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= n; v[1] /= n; v[2] /= n; };
        cross(d, up, du); normalize(du);
        cross(du, d, dv); normalize(dv);
        const int axis = face / 2, e1 = axis == 0 ? 1 : 0, e2 = axis == 2 ? 1 : 2;      // the other two, in r, u, f order
        double m[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < 3; ++c) {
            m[0] += (double)s.basis[3 * e1 + c] * du[c]; m[1] += (double)s.basis[3 * e2 + c] * du[c];
            m[2] += (double)s.basis[3 * e1 + c] * dv[c]; m[3] += (double)s.basis[3 * e2 + c] * dv[c];
        }
        for (int c = 0; c < 4; ++c) k->m[face][c] = (float)m[c];
    }
}
// The equirect's tables on the device, rebuilt only when the size or S changed.  The upload reads pageable host memory that dies with this call: waited for.
int pano_tables_ensure(hipStream_t stream, de_ctx::PanoTab& d, int width, int height, int S) {
    if (d.t[0] && d.width == width && d.height == height && d.S == S) return DE_OK;
    std::vector<float> h[4];
    const double pi = 3.14159265358979323846;
    pano_build_tables(width, S, 2.0 * pi, &h[0], &h[1]);
    pano_build_tables(height, S, pi, &h[2], &h[3]);
    d.S = 0;
    for (int k = 0; k < 4; ++k) { int rc = d.t[k].ensure(h[k].size() * sizeof(float), "the panorama's buffers"); if (rc) return rc; }
    for (int k = 0; k < 4; ++k) HIP_TRY(hipMemcpyAsync(d.t[k], h[k].data(), h[k].size() * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    d.width = width; d.height = height; d.S = S;
    return DE_OK;
}
// faces [6][N][N][3] -> out (width, height, 3) on `stream`; `k` carries the settings' constants (pano_make_consts), `tab` the equirect's tables.
// rows: environment_kernel instead (include/digital_earth_environment.h) — the same arithmetic into out [height][width][3].
int pano_launch(hipStream_t stream, const de_panorama& s, const PanoArgs& k, int N, const float* faces, const de_ctx::PanoTab& tab, float* out, bool rows = false) {
    PanoArgs a = k;
    a.faces = faces; a.out = out; a.N = N; a.width = s.width; a.height = s.height; a.S = s.supersample; a.fisheye = s.projection == DE_PANO_FISHEYE ? 1 : 0;
    a.sin_lon = tab.t[0]; a.cos_lon = tab.t[1]; a.sin_lat = tab.t[2]; a.cos_lat = tab.t[3];
    const unsigned long long blocks = (unsigned long long)pano_tiles(s.width) * (unsigned long long)pano_tiles(s.height);      // at most 2^28 / 128 + ...: one dimension holds it
    if (rows) hipLaunchKernelGGL(environment_kernel, dim3((unsigned)blocks), dim3(PANO_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(panorama_kernel, dim3((unsigned)blocks), dim3(PANO_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return DE_OK;
}
// What every call that hands out the shown image answers before anything is enqueued while the stage is on without its six faces.
int pano_refusal(const de_ctx* c) {
    if (c->pano.on && c->pano_mask != 63u) return fail(DE_ERR_STATE, "the panorama is on and fewer than six faces are captured (de_panorama_capture)");
    return DE_OK;
}
// Behind the display on the context stream: the six slots -> pano_out.
int run_panorama(de_ctx* c) {
    if (c->pano.projection == DE_PANO_EQUIRECT) { int rc = pano_tables_ensure(c->stream, c->pano_tab, c->pano.width, c->pano.height, c->pano.supersample); if (rc) return rc; }
    return pano_launch(c->stream, c->pano, c->pano_consts, c->W, c->pano_faces, c->pano_tab, c->pano_out);
}
// ---- the scene-linear panorama (include/digital_earth_environment.h, environment_kernels.hip, environment_body.h)
// The scene-linear outputs (EXR, RGBE) are the panorama's: the stage on and all six LINEAR slots held.  (On with fewer, their calls refuse: linear_pano_refusal.)
bool env_active(const de_ctx* c) { return c->pano.on && c->env_mask == 63u; }
size_t env_face_floats(const de_ctx* c) { return (size_t)c->W * (size_t)c->W * 3; }
// src ([N][N][3] and its divisor) -> one linear slot on `stream`: the division and the transposition.
int env_capture_launch(hipStream_t stream, const DisplaySrc& src, float* slot) {
    const unsigned tiles = (unsigned)((src.W + ENV_TILE - 1) / ENV_TILE);      // a face is square
    hipLaunchKernelGGL(environment_capture_kernel, dim3(tiles * tiles), dim3(ENV_THREADS), 0, stream, src, slot);
    HIP_TRY(hipGetLastError());
    return DE_OK;
}
// ---- the packed outputs (pack.h): their settings share the quantiser's mode, their launches the grid (pack_grid).  `who`: the settings struct's name.
int pack_mode_check(int mode, const char* who) {
    if (mode < DE_PIXELS_TRUNCATE || mode > DE_PIXELS_DITHER) return fail(DE_ERR_INVALID, std::string(who) + ".mode must be DE_PIXELS_TRUNCATE, _ROUND or _DITHER");
    return DE_OK;
}
// ---- 8-bit pixel output (include/digital_earth_pixels.h, pixels_kernels.hip)
size_t px_size(const de_ctx* c) { return (size_t)out_w(c) * (size_t)out_h(c) * (size_t)c->px.channels; }      // of the output size (include/digital_earth_output_scale.h): W x H while that stage is off
size_t px_capacity(const de_ctx* c) { return (size_t)out_w(c) * (size_t)out_h(c) * 4; }      // every buffer holds either format: de_set_pixels frees nothing
int px_settings_check(const de_pixels* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_pixels)) return fail(DE_ERR_INVALID, "de_pixels.struct_bytes does not match this library's struct");
    if (s->channels != 3 && s->channels != 4) return fail(DE_ERR_INVALID, "de_pixels.channels must be 3 or 4");
    return pack_mode_check(s->mode, "de_pixels");
}
void px_launch(hipStream_t stream, const float* image, uint8_t* out, int W, int H, const de_pixels& s, uint32_t phase) {
    PixelsArgs a;
    a.image = image; a.out = out; a.W = W; a.H = H; a.channels = s.channels; a.mode = s.mode; a.seed = s.seed; a.phase = phase;
    hipLaunchKernelGGL(pixels_pack_kernel, pack_grid(W, H), dim3(256), 0, stream, a);
}
// ---- HDR display output: the packed pixels (include/digital_earth_hdr_output.h, hdr_output_kernels.hip, hdr_pack.h)
size_t hpx_size(const de_ctx* c) { return (size_t)out_w(c) * (size_t)out_h(c) * (c->ho.pixel_format == DE_HDR_PIXELS_RGB16 ? 6u : 4u); }
size_t hpx_capacity(const de_ctx* c) { return (size_t)out_w(c) * (size_t)out_h(c) * 6; }      // every buffer holds either format
int ho_settings_check(const de_hdr_output* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_hdr_output)) return fail(DE_ERR_INVALID, "de_hdr_output.struct_bytes does not match this library's struct");
    if (!(s->peak_nits >= 100.0f && s->peak_nits <= 10000.0f)) return fail(DE_ERR_INVALID, "de_hdr_output.peak_nits must lie in [100, 10000]");      // NaN fails both
    if (s->gamut < DE_HDR_GAMUT_REC709 || s->gamut > DE_HDR_GAMUT_REC2020) return fail(DE_ERR_INVALID, "de_hdr_output.gamut must be DE_HDR_GAMUT_REC709, _P3D65 or _REC2020");
    if (s->transfer < DE_HDR_TRANSFER_LINEAR || s->transfer > DE_HDR_TRANSFER_HLG) return fail(DE_ERR_INVALID, "de_hdr_output.transfer must be DE_HDR_TRANSFER_LINEAR, _PQ or _HLG");
    if (s->pixel_format < DE_HDR_PIXELS_RGB10A2 || s->pixel_format > DE_HDR_PIXELS_RGB16) return fail(DE_ERR_INVALID, "de_hdr_output.pixel_format must be DE_HDR_PIXELS_RGB10A2 or _RGB16");
    return pack_mode_check(s->mode, "de_hdr_output");
}
void hpx_launch(hipStream_t stream, const float* image, void* out, int W, int H, const de_hdr_output& s, uint32_t phase) {
    HdrPackArgs a;
    a.image = image; a.out = out; a.W = W; a.H = H; a.format = s.pixel_format; a.mode = s.mode; a.seed = s.seed; a.phase = phase;
    hipLaunchKernelGGL(hdr_pack_kernel, pack_grid(W, H), dim3(256), 0, stream, a);
}
// ---- video frame output (include/digital_earth_video.h, videoframe_kernels.hip)
size_t vd_sample_bytes(const de_video& s) { return s.format >= DE_VIDEO_P010 ? 2u : 1u; }
size_t vd_frame_bytes(int W, int H, const de_video& s) { return (size_t)W * (size_t)H / 2 * 3 * vd_sample_bytes(s); }
size_t vd_size(const de_ctx* c) { return vd_frame_bytes(out_w(c), out_h(c), c->vd); }      // of the output size, as px_size
size_t vd_capacity(const de_ctx* c) { return (size_t)out_w(c) * (size_t)out_h(c) * 3; }      // every buffer holds any format: de_set_video frees nothing
int vd_settings_check(const de_video* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_video)) return fail(DE_ERR_INVALID, "de_video.struct_bytes does not match this library's struct");
    if (s->format < DE_VIDEO_NV12 || s->format > DE_VIDEO_I010) return fail(DE_ERR_INVALID, "de_video.format must be DE_VIDEO_NV12, _I420, _P010 or _I010");
    if (s->matrix < DE_VIDEO_MATRIX_BT709 || s->matrix > DE_VIDEO_MATRIX_BT2020) return fail(DE_ERR_INVALID, "de_video.matrix must be DE_VIDEO_MATRIX_BT709, _BT601 or _BT2020");
    if (s->range < DE_VIDEO_RANGE_LIMITED || s->range > DE_VIDEO_RANGE_FULL) return fail(DE_ERR_INVALID, "de_video.range must be DE_VIDEO_RANGE_LIMITED or _FULL");
    if (s->siting < DE_VIDEO_SITING_LEFT || s->siting > DE_VIDEO_SITING_TOPLEFT) return fail(DE_ERR_INVALID, "de_video.siting must be DE_VIDEO_SITING_LEFT, _CENTER or _TOPLEFT");
    return pack_mode_check(s->mode, "de_video");
}
int vd_even_check(const de_ctx* c) {
    if ((out_w(c) | out_h(c)) & 1) return fail(DE_ERR_STATE, "a 4:2:0 frame needs an even width and height: the output size is odd");
    return DE_OK;
}
void vd_launch(hipStream_t stream, const float* image, uint8_t* out, int W, int H, const de_video& s, const VideoConsts& k, uint32_t phase) {
    VideoArgs a;
    a.image = image; a.out = out; a.W = W; a.H = H; a.format = s.format; a.siting = s.siting; a.mode = s.mode; a.seed = s.seed; a.phase = phase; a.k = k;
    hipLaunchKernelGGL(videoframe_pack_kernel, pack_grid(W, H), dim3(256), 0, stream, a);
}
// ---- JPEG output (include/digital_earth_jpeg.h, jpeg_kernels.hip, jpeg_tables.h)
int jp_settings_check(const de_jpeg* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_jpeg)) return fail(DE_ERR_INVALID, "de_jpeg.struct_bytes does not match this library's struct");
    if (s->quality < 1 || s->quality > 100) return fail(DE_ERR_INVALID, "de_jpeg.quality must lie in 1 ... 100");
    if (s->restart_mcus < 1 || s->restart_mcus > 65535) return fail(DE_ERR_INVALID, "de_jpeg.restart_mcus must lie in 1 ... 65535");
    return DE_OK;
}
int jp_geometry_check(const JpegGeometry& g) {      // the kernels count bytes in 32 bits
    if (g.capacity + 64 >= (1ull << 32)) return fail(DE_ERR_INVALID, "the JPEG output's worst case does not fit 2^32 bytes at this size");
    return DE_OK;
}
// The buffers of one conversion of geometry g; `words` holds len[intervals], offset[intervals] and the status word.
int jp_work_ensure(de_ctx::JpegWork& w, const JpegGeometry& g) {
    int rc = w.planes.ensure((size_t)g.W * (size_t)g.H / 2 * 3, "JPEG buffers");
    if (!rc) rc = w.coef.ensure(g.blocks * 64 * sizeof(int16_t), "JPEG buffers");
    if (!rc) rc = w.mask.ensure(g.blocks * sizeof(unsigned long long), "JPEG buffers");
    if (!rc) rc = w.slots.ensure(g.intervals * g.slot_bytes, "JPEG buffers");
    if (!rc) rc = w.words.ensure((2 * g.intervals + 4) * sizeof(uint32_t), "JPEG buffers");
    if (!rc) rc = w.tab.ensure(sizeof(JpegTables), "JPEG buffers");
    return rc;
}
// image -> planes -> coefficients -> slots -> the stream at `out` (whose framing is in place or on its way on this stream).  w.tab holds the tables.
void jp_launch(hipStream_t stream, const float* image, const de_ctx::JpegWork& w, const JpegGeometry& g, uint8_t* out) {
    static const de_video jfif = {(uint32_t)sizeof(de_video), DE_VIDEO_I420, DE_VIDEO_MATRIX_BT601, DE_VIDEO_RANGE_FULL, DE_VIDEO_SITING_CENTER, DE_PIXELS_ROUND, 0u, 0};
    vd_launch(stream, image, w.planes, g.W, g.H, jfif, vd_make_consts(jfif.format, jfif.matrix, jfif.range), 0u);
    JpegArgs a;
    a.planes = w.planes; a.tab = w.tab; a.coef = w.coef; a.mask = w.mask; a.slots = w.slots;
    a.len = w.words; a.offset = w.words + g.intervals; a.status = w.words + 2 * g.intervals; a.out = out;
    a.W = g.W; a.H = g.H; a.mcus_x = g.mcus_x; a.restart = g.restart;
    a.blocks = (uint32_t)g.blocks; a.mcus = (uint32_t)g.mcus; a.count = (uint32_t)g.intervals; a.slot_bytes = (uint32_t)g.slot_bytes;
    a.front = JP_FRAMING_BYTES; a.extra = 2u; a.trailer = 0u; a.capacity = (uint32_t)g.capacity;
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)((g.blocks + JP_WG_BLOCKS - 1) / JP_WG_BLOCKS)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((g.intervals + 63) / 64)), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(CS_SCAN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(jpeg_compact_kernel, dim3((unsigned)g.intervals), dim3(256), 0, stream, a);
}
JpegGeometry jp_ctx_geometry(const de_ctx* c) { return jp_geometry(out_w(c), out_h(c), c->jp.restart_mcus); }
int jp_length(const void* word, uint64_t* len) {
    return coded_read_word(word, len, "the JPEG encoder met a stream longer than its proven worst case: nothing was written past a buffer", "the JPEG encoder met a coefficient outside the DCT's proven range");
}
// One conversion of the frame as it stands into `dev`, a stream on the device that is (re-)allocated and framed as needed.  Nothing is waited for.
int jp_render(de_ctx* c, Dev<uint8_t>& dev, uint64_t& framed) {
    HIP_TRY(hipSetDevice(c->device));
    const JpegGeometry g = jp_ctx_geometry(c);
    int rc = jp_geometry_check(g);
    if (rc) return rc;
    if (c->jp_w != g.W || c->jp_h != g.H || c->jp_tab_gen == 0) {      // the first conversion, or a new output size: tables (the defaults') and framing
        if (c->jp_tab_gen == 0) jp_make_tables(c->jp.quality, &c->jp_tab);
        c->jp_gen++; c->jp_tab_gen = c->jp_gen; c->jp_w = g.W; c->jp_h = g.H;
        jp_write_framing(c->jp_tab, g.W, g.H, c->jp.restart_mcus, c->jp_framing);
    }
    const uint8_t* before = dev.get();
    rc = dev.ensure(coded_stream_bytes(g.capacity), "JPEG buffers");      // one that is too small is replaced: hipFree waits for the work that reads it
    if (rc) return rc;
    if (dev.get() != before) framed = 0;
    const JpegTables* tab_before = c->jp_work.tab.get();
    rc = jp_work_ensure(c->jp_work, g);
    if (rc) return rc;
    if (c->jp_work.tab.get() != tab_before) c->jp_tab_uploaded = 0;
    // pageable sources: the runtime has read them when the call returns; on the device they are ordered behind the conversions already enqueued
    if (c->jp_tab_uploaded != c->jp_tab_gen) { HIP_TRY(hipMemcpyAsync(c->jp_work.tab, &c->jp_tab, sizeof(JpegTables), hipMemcpyHostToDevice, c->stream)); c->jp_tab_uploaded = c->jp_tab_gen; }
    if (framed != c->jp_gen) { HIP_TRY(hipMemcpyAsync(dev + CS_WORD_BYTES, c->jp_framing, JP_FRAMING_BYTES, hipMemcpyHostToDevice, c->stream)); framed = c->jp_gen; }
    rc = de_render_to_image(c, nullptr);
    if (rc) return rc;
    jp_launch(c->stream, shown_image(c), c->jp_work, g, dev);
    HIP_TRY(hipGetLastError());
    c->jp_coded.out.count++;
    return DE_OK;
}
struct JpegOut {      // the descriptor of de_fetch.h's entry points
    static constexpr const char* too_small = "out_bytes is smaller than the frame (*len; de_jpeg_capacity bounds every frame)";
    static CodedOut& coded(de_ctx* c) { return c->jp_coded; }
    static int size_refusal(const de_ctx* c) { return vd_even_check(c); }
    static int refusal(const de_ctx* c) { return vd_even_check(c); }
    static JpegGeometry geometry(const de_ctx* c) { return jp_ctx_geometry(c); }
    static size_t first_prefix(const JpegGeometry& g) { return JP_FRAMING_BYTES + (size_t)g.W * (size_t)g.H / 4; }      // two bits per pixel
    static int render(de_ctx* c, Dev<uint8_t>& dev, int k) { return jp_render(c, dev, k < 0 ? c->jp_out_framed : c->jp_cell_framed[k]); }
    static bool reads_panorama(const de_ctx*) { return true; }      // the shown image
    static int length(const void* word, uint64_t* len) { return jp_length(word, len); }
};
// ---- PNG output (include/digital_earth_png.h, png_kernels.hip, png_tables.h)
int pn_settings_check(const de_png* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_png)) return fail(DE_ERR_INVALID, "de_png.struct_bytes does not match this library's struct");
    if (s->source < DE_PNG_SOURCE_PIXELS || s->source > DE_PNG_SOURCE_HDR_PIXELS) return fail(DE_ERR_INVALID, "de_png.source must be DE_PNG_SOURCE_PIXELS or _HDR_PIXELS");
    if (s->filter < DE_PNG_FILTER_NONE || s->filter > DE_PNG_FILTER_ADAPTIVE) return fail(DE_ERR_INVALID, "de_png.filter must be DE_PNG_FILTER_NONE ... _PAETH or _ADAPTIVE");
    if (s->chunk_bytes < 1024 || s->chunk_bytes > 65535) return fail(DE_ERR_INVALID, "de_png.chunk_bytes must lie in 1024 ... 65535");
    return DE_OK;
}
int pn_shape_check(int W, int H, int channels, int depth) {      // what one conversion can take: the kernels count filtered bytes in 32 bits
    if (W <= 0 || H <= 0 || !((depth == 8 && (channels == 3 || channels == 4)) || (depth == 16 && channels == 3)))
        return fail(DE_ERR_INVALID, "a PNG frame needs W, H >= 1 and 3 or 4 channels of 8 bits or 3 of 16");
    if ((unsigned long long)H * (1ull + (unsigned long long)W * (unsigned long long)(channels * depth / 8)) > PNG_MAX_FILTERED)
        return fail(DE_ERR_INVALID, "the PNG output takes at most 2^27 filtered bytes, H (1 + W bpp)");
    return DE_OK;
}
void pn_cicp(const de_hdr_output& ho, uint8_t cicp[4]) {      // as png16.cicp_of: {primaries, transfer, RGB, full range}
    static const uint8_t primaries[3] = {1, 12, 9}, transfer[3] = {8, 16, 18};
    cicp[0] = primaries[ho.gamut]; cicp[1] = transfer[ho.transfer]; cicp[2] = 0; cicp[3] = 1;
}
// The buffers of one conversion of geometry g; `words` holds len[chunks], offset[chunks], adler[chunks][2] and the status word.
int pn_work_ensure(de_ctx::PngWork& w, const PngGeometry& g) {
    const PngTables* before = w.tab.get();
    int rc = w.pixels.ensure((size_t)g.H * g.row_bytes, "PNG buffers");
    if (!rc) rc = w.filtered.ensure(g.filtered, "PNG buffers");
    if (!rc) rc = w.slots.ensure(g.chunks * g.slot_bytes, "PNG buffers");
    if (!rc) rc = w.words.ensure((4 * g.chunks + 4) * sizeof(uint32_t), "PNG buffers");
    if (!rc) rc = w.tab.ensure(sizeof(PngTables), "PNG buffers");
    if (w.tab.get() != before) w.tab_uploaded = false;
    return rc;
}
// The tables onto the device, once per buffer.  The source is static: the copy may read it whenever it runs.
const PngTables& pn_host_tables() { static const PngTables tables = [] { PngTables t; png_make_tables(&t); return t; }(); return tables; }
hipError_t pn_tables_upload(hipStream_t stream, de_ctx::PngWork& w) {
    if (w.tab_uploaded) return hipSuccess;
    hipError_t e = hipMemcpyAsync(w.tab, &pn_host_tables(), sizeof(PngTables), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) w.tab_uploaded = true;
    return e;
}
// w.pixels (packed, on this stream) -> filtered -> slots -> the file at `out`.  w.tab holds the tables.
void pn_launch(hipStream_t stream, const de_ctx::PngWork& w, const PngGeometry& g, int filter, const uint8_t cicp[4], uint8_t* out) {
    PngArgs a;
    a.pixels = w.pixels; a.tab = w.tab; a.filtered = w.filtered; a.slots = w.slots;
    a.len = w.words; a.offset = w.words + g.chunks; a.adler = w.words + 2 * g.chunks; a.status = w.words + 4 * g.chunks; a.out = out;
    a.H = g.H; a.bpp = g.bpp; a.swap16 = g.depth == 16 ? 1 : 0; a.filter = filter; a.chunk_bytes = g.chunk_bytes;
    a.row_bytes = (uint32_t)g.row_bytes; a.total = (uint32_t)g.filtered; a.count = (uint32_t)g.chunks; a.slot_bytes = (uint32_t)g.slot_bytes;
    a.extra = 0u; a.trailer = PNG_TRAILER_BYTES; a.capacity = (uint32_t)g.capacity;
    memset(a.front_bytes, 0, sizeof(a.front_bytes));
    a.front = (uint32_t)png_write_front(pn_host_tables(), g, cicp, a.front_bytes);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)g.H), dim3(PNG_FILTER_THREADS), 0, stream, a);
    hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)g.chunks), dim3(PNG_THREADS), 0, stream, a);
    hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(CS_SCAN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(png_compact_kernel, dim3((unsigned)g.chunks), dim3(256), 0, stream, a);
}
int pn_source_check(const de_ctx* c) {
    if (c->pn.source == DE_PNG_SOURCE_HDR_PIXELS && !(c->ho.on && c->ho.pixel_format == DE_HDR_PIXELS_RGB16))
        return fail(DE_ERR_STATE, "the PNG output's HDR source needs the HDR display output on at DE_HDR_PIXELS_RGB16");
    return DE_OK;
}
PngGeometry pn_ctx_geometry(const de_ctx* c) {
    const bool hdr = c->pn.source == DE_PNG_SOURCE_HDR_PIXELS;
    return png_geometry(out_w(c), out_h(c), hdr ? 3 : c->px.channels, hdr ? 16 : 8, c->pn.chunk_bytes);
}
int pn_length(const void* word, uint64_t* len) {      // its coders raise no range status
    static const char* const text = "the PNG encoder met a chunk longer than its proven worst case: nothing was written past a buffer";
    return coded_read_word(word, len, text, text);
}
// One conversion of the frame as it stands into `dev`, a file on the device that is (re-)allocated as needed.  Nothing is waited for.
int pn_render(de_ctx* c, Dev<uint8_t>& dev) {
    HIP_TRY(hipSetDevice(c->device));
    const PngGeometry g = pn_ctx_geometry(c);
    int rc = pn_shape_check(g.W, g.H, g.channels, g.depth);
    if (rc) return rc;
    rc = dev.ensure(coded_stream_bytes(g.capacity), "PNG buffers");      // one that is too small is replaced: hipFree waits for the work that reads it
    if (rc) return rc;
    rc = pn_work_ensure(c->pn_work, g);
    if (rc) return rc;
    HIP_TRY(pn_tables_upload(c->stream, c->pn_work));
    rc = de_render_to_image(c, nullptr);
    if (rc) return rc;
    uint8_t cicp[4] = {1, 8, 0, 1};
    if (g.depth == 16) {
        const uint32_t phase = c->ho.animate ? c->pn_coded.out.count : 0u;
        hpx_launch(c->stream, shown_image(c), c->pn_work.pixels, g.W, g.H, c->ho, phase);
        pn_cicp(c->ho, cicp);
        c->pn_coded.out.last_phase = phase;
    } else {
        const uint32_t phase = c->px.animate ? c->pn_coded.out.count : 0u;
        px_launch(c->stream, shown_image(c), c->pn_work.pixels, g.W, g.H, c->px, phase);
        c->pn_coded.out.last_phase = phase;
    }
    pn_launch(c->stream, c->pn_work, g, c->pn.filter, cicp, dev);
    HIP_TRY(hipGetLastError());
    c->pn_coded.out.count++;
    return DE_OK;
}
struct PngOut {
    static constexpr const char* too_small = "out_bytes is smaller than the file (*len; de_png_capacity bounds every frame)";
    static CodedOut& coded(de_ctx* c) { return c->pn_coded; }
    static int size_refusal(const de_ctx* c) { return pn_source_check(c); }
    static int refusal(const de_ctx* c) { return pn_source_check(c); }
    static PngGeometry geometry(const de_ctx* c) { return pn_ctx_geometry(c); }
    static size_t first_prefix(const PngGeometry& g) { return g.front + g.filtered / 4; }      // a quarter of the filtered bytes
    static int render(de_ctx* c, Dev<uint8_t>& dev, int) { return pn_render(c, dev); }
    static bool reads_panorama(const de_ctx*) { return true; }      // the shown image
    static int length(const void* word, uint64_t* len) { return pn_length(word, len); }
};
// ---- look LUTs (include/digital_earth_look.h, look_kernels.hip): in place on the displayed image, directly behind the display launch
// Everything de_set_look and de_debug_look refuse, in the header's order.
int lk_settings_check(const de_look* s, const float* t1, const float* t3) {
    if (s->struct_bytes != (uint32_t)sizeof(de_look)) return fail(DE_ERR_INVALID, "de_look.struct_bytes does not match this library's struct");
    if (s->interpolation < DE_LOOK_TRILINEAR || s->interpolation > DE_LOOK_TETRAHEDRAL) return fail(DE_ERR_INVALID, "de_look.interpolation must be DE_LOOK_TRILINEAR or _TETRAHEDRAL");
    if (!(s->strength >= 0.0f && s->strength <= 1.0f)) return fail(DE_ERR_INVALID, "de_look.strength must lie in [0, 1]");      // NaN fails both
    if (s->size_1d != 0 && (s->size_1d < 2 || s->size_1d > DE_LOOK_MAX_1D)) return fail(DE_ERR_INVALID, "de_look.size_1d must be 0 or 2 ... DE_LOOK_MAX_1D");
    if (s->size_3d != 0 && (s->size_3d < 2 || s->size_3d > DE_LOOK_MAX_3D)) return fail(DE_ERR_INVALID, "de_look.size_3d must be 0 or 2 ... DE_LOOK_MAX_3D");
    if (s->enabled && !s->size_1d && !s->size_3d) return fail(DE_ERR_INVALID, "de_look: the stage cannot be on without a table");
    if ((s->size_1d && !t1) || (s->size_3d && !t3)) return fail(DE_ERR_INVALID, "de_look: a table of non-zero size is null");
    for (int tab = 0; tab < 2; ++tab) {
        const int N = tab ? s->size_3d : s->size_1d;
        if (!N) continue;
        const float* lo = tab ? s->min_3d : s->min_1d;
        const float* hi = tab ? s->max_3d : s->max_1d;
        for (int c = 0; c < 3; ++c)
            if (!isfinite(lo[c]) || !isfinite(hi[c]) || !(hi[c] > lo[c]) || !isfinite(lk_scale(N, lo[c], hi[c])))
                return fail(DE_ERR_INVALID, "de_look: a table's domain must be finite with max > min");
        const float* t = tab ? t3 : t1;
        const size_t n = tab ? (size_t)N * N * N * 3 : (size_t)N * 3;
        for (size_t i = 0; i < n; ++i)
            if (!isfinite(t[i])) return fail(DE_ERR_INVALID, "de_look: a table value is not finite");
    }
    return DE_OK;
}
// Checked settings and tables onto the device, into `d` (empty on entry; empty again when the call fails).  The upload reads host memory that dies
// with the caller: waited for.
int lk_upload(hipStream_t stream, const de_look& s, const float* t1, const float* t3, de_ctx::LookDev& d) {
    std::vector<float> wide;      // the 3D table, one float4 per lattice point; alive until the copy has been waited for
    for (int c = 0; c < 3; ++c) {
        if (s.size_1d) { d.a1[c].lo = s.min_1d[c]; d.a1[c].k = lk_scale(s.size_1d, s.min_1d[c], s.max_1d[c]); }
        if (s.size_3d) { d.a3[c].lo = s.min_3d[c]; d.a3[c].k = lk_scale(s.size_3d, s.min_3d[c], s.max_3d[c]); }
    }
    hipError_t e = hipSuccess;
    if (s.size_1d) {
        const size_t bytes = (size_t)s.size_1d * 3 * sizeof(float);
        e = d.t1.ensure(bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(d.t1, t1, bytes, hipMemcpyHostToDevice, stream);
    }
    if (e == hipSuccess && s.size_3d) {
        const size_t n = (size_t)s.size_3d * s.size_3d * s.size_3d;
        wide.resize(n * 4);
        for (size_t i = 0; i < n; ++i) { wide[4 * i] = t3[3 * i]; wide[4 * i + 1] = t3[3 * i + 1]; wide[4 * i + 2] = t3[3 * i + 2]; wide[4 * i + 3] = 0.0f; }
        e = d.t3.ensure(n * sizeof(float4));
        if (e == hipSuccess) e = hipMemcpyAsync(d.t3, wide.data(), n * sizeof(float4), hipMemcpyHostToDevice, stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { (void)hipGetLastError(); d.t1.release(); d.t3.release(); return fail(DE_ERR_HIP, std::string("look tables: ") + hipGetErrorString(e)); }
    return DE_OK;
}
void lk_launch(hipStream_t stream, float* image, uint64_t n_pixels, const de_look& s, const de_ctx::LookDev& d) {
    LookArgs a;
    a.image = image; a.n = n_pixels; a.t1 = s.size_1d ? d.t1 : nullptr; a.t3 = s.size_3d ? d.t3 : nullptr; a.n1 = s.size_1d; a.n3 = s.size_3d;
    a.tetrahedral = s.interpolation == DE_LOOK_TETRAHEDRAL ? 1 : 0; a.strength = s.strength;
    for (int c = 0; c < 3; ++c) { a.a1[c] = d.a1[c]; a.a3[c] = d.a3[c]; }
    hipLaunchKernelGGL(look_apply_kernel, dim3((unsigned)((lk_threads(n_pixels) + 255u) / 256u)), dim3(256), 0, stream, a);
}

// The guides of the frame as it stands, for a consumer outside the denoiser (the EXR output's AOV channels, §24): de_fetch_guides' two steps, its refusals.
int guides_of_the_frame(de_ctx* c) {
    int rc = run_setup(c);
    if (rc) return rc;
    return dn_ensure_guides(c);
}

// ---- the chain.  Where a caller leaves it: behind the stage it hands out (an intermediate fetch), or in front of the display launch.
enum DisplayStop { STOP_DENOISE, STOP_HISTORY, STOP_BLOOM, STOP_LOCAL_EXPOSURE, STOP_IMAGE };

// What must hold before anything is enqueued, in the order in which a caller learns of it: the stage it asks for is on; the maps (the history's own
// fetch only: it answers before the guides' launch would); the LUTs, wherever the frame constants are read — the history's camera, the anchor of local
// exposure, the display transform — so not for the bloom or the denoiser alone; the denoiser's refusal whenever it is on; the HDR output's for the display.
int display_chain_refusal(de_ctx* c, DisplayStop stop) {
    static const char* const fetch_name[] = {"fetch_denoised_hdr", "fetch_history_hdr", "fetch_bloom_hdr", "fetch_local_exposure_hdr", "fetch_image"};
    if (stop == STOP_DENOISE && !c->dn_on) return fail(DE_ERR_STATE, "the denoiser is off (de_set_denoise)");
    if (stop == STOP_HISTORY && !c->hs_on) return fail(DE_ERR_STATE, "history reprojection is off (de_set_history)");
    if (stop == STOP_BLOOM && !c->bl_on) return fail(DE_ERR_STATE, "bloom is off (de_set_bloom)");
    if (stop == STOP_LOCAL_EXPOSURE && !c->lx_on) return fail(DE_ERR_STATE, "local exposure is off (de_set_local_exposure)");
    if (stop == STOP_HISTORY)
        for (int i = 0; i < DE_TEX_COUNT; ++i)
            if (!c->tex[i].set) return fail(DE_ERR_STATE, "history reprojection takes its distances from the maps: all 7 must be uploaded or generated first");
    if ((stop == STOP_HISTORY || stop == STOP_LOCAL_EXPOSURE || stop == STOP_IMAGE) && !c->luts_set)
        return fail(DE_ERR_STATE, std::string("LUTs must be uploaded before ") + fetch_name[stop]);
    if (c->dn_on) { int rc = denoise_refusal(c); if (rc) return rc; }
    if (stop == STOP_IMAGE && c->ho.on) { int rc = hdr_output_refusal(c); if (rc) return rc; }
    return DE_OK;
}

// The stages that are on, in their one order, up to and including `stop`'s, on the context stream.  Afterwards *d and *per_tile describe what the next
// consumer reads: a transposed copy-out of d->hdr, or the display launch (per_tile: display_kernel<true>, every tile divided by its own count).  Every
// stage replaces d->hdr by a mean of its own, to be read with samples = 1 through the unchanged transform: x / 1.0f == x.
int display_chain(de_ctx* c, DisplayStop stop, DisplayArgs* d, bool* per_tile) {
    int rc = display_chain_refusal(c, stop);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // The frame constants of the current parameters.  A no-op unless a parameter changed; every caller runs it, also the bloom's fetch of a context
    // whose later stages are off and that reads none: what setup_kernel writes is a function of the parameters and the LUTs alone, whoever reads the
    // constants next runs it anyway, and every change of either marks them dirty again.
    rc = run_setup(c);
    if (rc) return rc;
    // The launches in flight first, and the next accumulate_kernel must not overwrite what this reads; then the filter, which reads S1 and S2: all
    // ahead of everything below, which reads the sums or the filtered mean.
    rc = join_slots(c);
    if (rc) return rc;
    touched_hdr(c);
    if (c->dn_on) { rc = run_denoise(c); if (rc) return rc; }
    // what the display reads: the sums with the frame's or the tiles' counts, a display source, or the filtered mean
    d->fc = c->d_fc; d->hdr = c->display_src ? c->display_src : c->d_hdr; d->image = c->d_image;
    d->crf.data = c->d_crf; d->crf.w = 1024; d->crf.h = c->n_crf;
    d->W = c->W; d->H = c->H; d->samples = c->current_spp; d->clamp = (c->p.flags & DE_FLAG_CLAMP_SAMPLER) ? 1 : 0;
    d->tile_spp = c->d_tile_spp;
    if (c->dn_on) { d->hdr = c->d_dn_out; d->samples = 1; }
    *per_tile = c->frame_kind == DE_FRAME_ADAPTIVE && !c->dn_on;
    if (stop == STOP_DENOISE) return DE_OK;
    // ahead of the meter and the bloom: they see the stabilised image
    if (c->hs_on) { rc = run_history(c, *d, *per_tile); if (rc) return rc; }
    if (stop == STOP_HISTORY) return DE_OK;
    // The meter, only when the chain goes past the bloom: local exposure and the display alone read d->fc, and the meter has state (the adaptation in
    // d_ae_state, ae_displayed) that a fetch of the history's or the bloom's mean must not advance.  Ahead of the bloom: the scene is metered, not the
    // lens.  The same transform over the metered exposure: a second FrameConsts, written on the device.
    if (c->ae_on && stop > STOP_BLOOM) { rc = run_meter(c, *d, *per_tile); if (rc) return rc; d->fc = c->d_fc_ae; }
    if (c->bl_on) { rc = run_bloom(c, *d, *per_tile); if (rc) return rc; }
    if (stop == STOP_BLOOM) return DE_OK;
    // last: the scene is metered, the lens glares, the print is dodged; the anchor is d->fc's exposure
    if (c->lx_on) { rc = run_local_exposure(c, *d, *per_tile); if (rc) return rc; }
    return DE_OK;
}

// ---- the scene-linear outputs (OpenEXR, Radiance RGBE): in FRONT of the display, behind the chain's stages.  What they share, and
// with de_environment_capture, which reads the same source.
static const DisplayStop linear_stop_of[] = {STOP_IMAGE, STOP_DENOISE, STOP_HISTORY, STOP_BLOOM, STOP_LOCAL_EXPOSURE};      // by DE_EXR_SOURCE_*; MEAN runs no chain
// What a scene-linear output of `source` reads of the frame as it stands, on the context stream: MEAN reads what the display launch would read with
// every stage off; the other sources are the chain left at their stage — its refusals, its side effects.
int linear_source(de_ctx* c, int source, DisplayArgs* d, bool* per_tile) {
    if (source != DE_EXR_SOURCE_MEAN) return display_chain(c, linear_stop_of[source], d, per_tile);
    int rc = join_slots(c);      // the launches in flight first, and the next accumulate_kernel must not overwrite what this reads
    if (rc) return rc;
    touched_hdr(c);
    d->hdr = c->display_src ? c->display_src : c->d_hdr; d->tile_spp = c->d_tile_spp; d->samples = c->current_spp; d->W = c->W; d->H = c->H;
    *per_tile = c->frame_kind == DE_FRAME_ADAPTIVE;
    return DE_OK;
}
// what the next accumulate_kernel must wait for ends behind the kernel that has read the sums, as behind the display launch in de_render_to_image
int linear_sums_read(de_ctx* c) {
    HIP_TRY(hipEventRecord(c->ev_main, c->stream));
    c->rec_render = c->gen_render; c->rec_hdr = c->gen_hdr;
    return DE_OK;
}
// a host-given or resampled image [H][W][3] as a source: no tile counts and a divisor of 1, x / 1.0f == x
DisplaySrc linear_src(const float* image, int W, int H) {
    DisplaySrc src;
    src.hdr = image; src.tile_spp = nullptr; src.samples = 1; src.W = W; src.H = H;
    return src;
}
// What these outputs deliver: the context's frame, or the scene-linear panorama while that is held (env_active; no AOV channel exists there).
struct LinearFrame { int W, H; bool env; };
LinearFrame linear_frame(const de_ctx* c) {
    const bool env = env_active(c);
    return {env ? c->pano.width : c->W, env ? c->pano.height : c->H, env};
}
// They sit in FRONT of the display: a face's scene-linear frame is not the panorama.  The scene-linear panorama is made of the six LINEAR slots alone
// (include/digital_earth_environment.h); without all six there is none.
int linear_pano_refusal(const de_ctx* c, const char* noun) {
    if (c->pano.on && c->env_mask != 63u) return fail(DE_ERR_STATE, std::string("the panorama is on (de_set_panorama): the ") + noun + " output reads the frame in front of the display, where a panorama exists only once six linear faces are captured (de_environment_capture)");
    return DE_OK;
}
// The environment as a source: six linear faces [6][n][n][3] resampled into `image`, [height][width][3] with row 0 at the bottom, which a layout reads
// with its rows flipped.  (The context's faces and tables, or a debug call's own.)
int env_source(hipStream_t stream, const de_panorama& p, const PanoArgs& k, int n, const float* faces, de_ctx::PanoTab& tab, float* image, DisplaySrc* src) {
    if (p.projection == DE_PANO_EQUIRECT) { int rc = pano_tables_ensure(stream, tab, p.width, p.height, p.supersample); if (rc) return rc; }
    int rc = pano_launch(stream, p, k, n, faces, tab, image, true);
    if (rc) return rc;
    *src = linear_src(image, p.width, p.height);
    return DE_OK;
}
// The resampling half of de_debug_environment_*, inside coded_debug's body: the caller's faces uploaded and resampled on buffers and tables of its own.
struct EnvDebug { Dev<float> faces, image; de_ctx::PanoTab tab; };
int env_debug_source(hipStream_t stream, EnvDebug& b, const float* faces, int n, const de_panorama& p, DisplaySrc* src) {
    PanoArgs k = {};
    pano_make_consts(p, n, &k);
    int rc = debug_upload(stream, b.faces, faces, (size_t)DE_PANO_FACES * (size_t)n * (size_t)n * 3 * sizeof(float));
    if (rc) return rc;
    HIP_TRY(b.image.ensure((size_t)p.width * (size_t)p.height * 3 * sizeof(float)));
    return env_source(stream, p, k, n, b.faces, b.tab, b.image, src);
}
int no_hook() { return DE_OK; }      // a launch's `after` where nothing of the context was read
// One conversion of what a scene-linear output F (ExrOut, RgbeOut) delivers into `dev`, a file on the device that is (re-)allocated as needed; behind
// F::refusal.  Nothing is waited for.  The panorama is read from the six linear slots alone: the frame as it stands is not.  F brings its settings'
// source, its geometry, what it refuses and prepares of the frame ahead of every allocation (frame_prepare), its noun, its work buffers with their
// tables (work) and its launch, which runs `after` behind the one kernel that reads the source.
template <class F>
int linear_render(de_ctx* c, Dev<uint8_t>& dev) {
    HIP_TRY(hipSetDevice(c->device));
    const auto g = F::geometry(c);
    const bool env = env_active(c);
    const int source = F::source(c);
    int rc = DE_OK;
    if (env) rc = c->env_out.ensure((size_t)g.W * (size_t)g.H * 3 * sizeof(float), "the environment's buffers");      // its size changes with de_set_panorama alone, which waits for the fetches that read it
    else {
        if (source != DE_EXR_SOURCE_MEAN) rc = display_chain_refusal(c, linear_stop_of[source]);      // ahead of every allocation: a refused call changes nothing
        if (!rc) rc = F::frame_prepare(c);
    }
    if (!rc) rc = dev.ensure(coded_stream_bytes(g.capacity), F::buffers);      // one that is too small is replaced: hipFree waits for the work that reads it
    if (!rc) rc = F::work(c, g);
    if (rc) return rc;
    DisplaySrc src;
    if (env) rc = env_source(c->stream, c->pano, c->pano_consts, c->W, c->env_faces, c->pano_tab, c->env_out, &src);
    else {
        DisplayArgs d;
        bool per_tile;
        rc = linear_source(c, source, &d, &per_tile);
        if (!rc) src = display_src(d, per_tile);
    }
    if (!rc) rc = F::launch(c, g, src, dev, [c, env] { return env ? (int)DE_OK : linear_sums_read(c); });      // the frame: the sums have been read
    if (rc) return rc;
    F::coded(c).out.count++;
    return DE_OK;
}

// ---- OpenEXR output (include/digital_earth_exr.h, exr_kernels.hip, exr_tables.h)
int ex_settings_check(const de_exr* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_exr)) return fail(DE_ERR_INVALID, "de_exr.struct_bytes does not match this library's struct");
    if (s->source < DE_EXR_SOURCE_MEAN || s->source > DE_EXR_SOURCE_LOCAL_EXPOSURE) return fail(DE_ERR_INVALID, "de_exr.source must be DE_EXR_SOURCE_MEAN, _DENOISED, _HISTORY, _BLOOM or _LOCAL_EXPOSURE");
    if (s->pixel_type != DE_EXR_PIXEL_HALF && s->pixel_type != DE_EXR_PIXEL_FLOAT) return fail(DE_ERR_INVALID, "de_exr.pixel_type must be DE_EXR_PIXEL_HALF or _FLOAT");
    if (s->compression != DE_EXR_COMPRESSION_NONE && s->compression != DE_EXR_COMPRESSION_ZIPS && s->compression != DE_EXR_COMPRESSION_ZIP)
        return fail(DE_ERR_INVALID, "de_exr.compression must be DE_EXR_COMPRESSION_NONE, _ZIPS or _ZIP");
    if (s->chunk_bytes < 1024 || s->chunk_bytes > 65535) return fail(DE_ERR_INVALID, "de_exr.chunk_bytes must lie in 1024 ... 65535");
    if (!(s->scale > 0.0f) || !(s->scale < INFINITY)) return fail(DE_ERR_INVALID, "de_exr.scale must be finite and greater than 0");      // NaN fails the first
    return DE_OK;
}
int ex_mask_check(uint32_t mask) {
    if (mask & ~(uint32_t)DE_EXR_AOV_ALL) return fail(DE_ERR_INVALID, "unknown DE_EXR_AOV_* bit");
    return DE_OK;
}
int ex_shape_check(int W, int H, int pixel_type, uint32_t mask = 0u) {      // what one conversion can take: the kernels count bytes in 32 bits
    if (W <= 0 || H <= 0) return fail(DE_ERR_INVALID, "an EXR frame needs W, H >= 1");
    if (!mask) {
        if ((unsigned long long)W * (unsigned long long)H * 3ull * (pixel_type == DE_EXR_PIXEL_FLOAT ? 4ull : 2ull) > EXR_MAX_RAW)
            return fail(DE_ERR_INVALID, "the EXR output takes at most 2^27 raw bytes, H W 3 bps");
        return DE_OK;
    }
    ExrChannel ch[EXR_MAX_CHANNELS];
    const int n = exr_channel_list(mask, pixel_type, 1, ch);
    unsigned long long sum = 0ull;
    for (int k = 0; k < n; ++k) sum += (unsigned long long)ch[k].bps;
    if ((unsigned long long)W * (unsigned long long)H * sum > EXR_MAX_RAW)
        return fail(DE_ERR_INVALID, "the EXR output takes at most 2^27 raw bytes, H W times the channels' bytes per pixel (fewer AOV channels, or HALF, make a frame smaller)");
    return DE_OK;
}
ExrGeometry ex_geometry(int W, int H, const de_exr& s, uint32_t mask = 0u) { return exr_geometry(W, H, s.pixel_type, s.compression, s.chunk_bytes, mask); }
// The buffers of one conversion of geometry g; `words` holds len[pieces], offset[pieces], alt_at[pieces], adler[pieces][2] and the status word.
int ex_work_ensure(de_ctx::ExrWork& w, const ExrGeometry& g) {
    const PngTables* before = w.tab.get();
    const bool zip = g.compression != DE_EXR_COMPRESSION_NONE;
    int rc = w.raw.ensure(g.blocks * g.r_stride, "EXR buffers");
    if (!rc && zip) rc = w.pred.ensure(g.blocks * g.p_stride, "EXR buffers");
    if (!rc) rc = w.slots.ensure(zip ? g.pieces * g.slot_bytes : 16, "EXR buffers");
    if (!rc) rc = w.words.ensure((5 * g.pieces + 4) * sizeof(uint32_t), "EXR buffers");
    if (!rc) rc = w.tab.ensure(sizeof(PngTables), "EXR buffers");
    if (w.tab.get() != before) w.tab_uploaded = false;
    return rc;
}
hipError_t ex_tables_upload(hipStream_t stream, de_ctx::ExrWork& w) {      // deflate's length codes: the PNG output's tables, static on the host
    if (w.tab_uploaded) return hipSuccess;
    hipError_t e = hipMemcpyAsync(w.tab, &pn_host_tables(), sizeof(PngTables), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) w.tab_uploaded = true;
    return e;
}
// src (on this stream) -> framed raw blocks -> predicted bytes -> slots -> the file at `out`.  w.tab holds the tables.  `after_layout` runs behind
// the one kernel that reads `src`.
// What the AOV planes of geometry g read: the guides, the sums with S2 and the divisor, each null (0) where no selected channel needs it.
struct ExrAovSrc {
    const float4* nc = nullptr; const float4* at = nullptr; const float* dist = nullptr;
    const float* s1 = nullptr; const float* s2 = nullptr;
    const int32_t* tile_spp = nullptr; const float* counts = nullptr; int samples = 1;
};
template <class AfterLayout>
int ex_launch(hipStream_t stream, const de_ctx::ExrWork& w, const ExrGeometry& g, const DisplaySrc& src, bool flip, float scale, uint8_t* out, AfterLayout after_layout,
              const ExrAovSrc& av = ExrAovSrc()) {
    ExrArgs a;
    a.front_fixed = (uint32_t)g.front_fixed; a.rgb_bps = (uint32_t)g.bps; a.counts = av.counts;
    a.aov = ExrAov();
    for (int k = 0; k < g.channels; ++k) {
        const ExrChannel& ch = g.ch[k];
        if (ch.slot <= EXR_SLOT_B) { a.rgb_offset[ch.slot] = (uint32_t)ch.offset; continue; }
        if (a.aov.planes >= EXR_MAX_AOV_PLANES) return fail(DE_ERR_INTERNAL, "the EXR output's channel list holds more AOV planes than the kernel takes");
        ExrPlane& pl = a.aov.plane[a.aov.planes++];
        pl.slot = (uint32_t)ch.slot; pl.bps = (uint32_t)ch.bps; pl.offset = (uint32_t)ch.offset;
        a.aov.need |= exr_slot_need(ch.slot);
    }
    const uint32_t need = a.aov.need;
    a.aov.nc = (need & EXR_NEED_NC) ? reinterpret_cast<const ExrF4*>(av.nc) : nullptr;
    a.aov.at = (need & EXR_NEED_AT) ? reinterpret_cast<const ExrF4*>(av.at) : nullptr;
    a.aov.dist = (need & EXR_NEED_DIST) ? av.dist : nullptr;
    a.aov.s1 = (need & EXR_NEED_MOMENTS) ? av.s1 : nullptr;
    a.aov.s2 = (need & EXR_NEED_MOMENTS) ? av.s2 : nullptr;
    a.aov.tile_spp = av.tile_spp; a.aov.counts = av.counts; a.aov.samples = av.samples;
    if (((need & EXR_NEED_NC) && !a.aov.nc) || ((need & EXR_NEED_AT) && !a.aov.at) || ((need & EXR_NEED_DIST) && !a.aov.dist) ||
        ((need & EXR_NEED_MOMENTS) && (!a.aov.s1 || !a.aov.s2)))
        return fail(DE_ERR_INTERNAL, "the EXR output's AOV channels were given no buffer to read");
    a.src = src; a.flip = flip ? 1 : 0; a.scale = scale; a.tab = w.tab; a.raw = w.raw; a.pred = w.pred; a.slots = w.slots;
    a.len = w.words; a.offset = w.words + g.pieces; a.alt_w = w.words + 2 * g.pieces; a.adler = w.words + 3 * g.pieces; a.status = w.words + 5 * g.pieces; a.out = out;
    a.alt = w.raw; a.alt_at = a.alt_w; a.alt_bytes = (uint32_t)(g.blocks * g.r_stride);
    a.pixel_type = g.pixel_type; a.compression = g.compression;
    a.W = (uint32_t)g.W; a.H = (uint32_t)g.H; a.L = (uint32_t)g.L; a.line_bytes = (uint32_t)g.line_bytes; a.block_bytes = (uint32_t)g.block_bytes;
    a.blocks = (uint32_t)g.blocks; a.chunk = (uint32_t)g.chunk; a.cpb = (uint32_t)g.cpb; a.r_stride = (uint32_t)g.r_stride; a.p_stride = (uint32_t)g.p_stride;
    a.count = (uint32_t)g.pieces; a.slot_bytes = (uint32_t)g.slot_bytes;
    a.front = (uint32_t)g.front; a.extra = 0u; a.trailer = 0u; a.capacity = (uint32_t)g.capacity;
    memset(a.front_bytes, 0, sizeof(a.front_bytes));
    exr_write_front(g, a.front_bytes);
    const unsigned row_wgs = (unsigned)((((size_t)g.W + 3) / 4 + 255) / 256), block_wgs = (unsigned)(((g.block_bytes + 3) / 4 + 255) / 256);      // exr_row_workgroups, exr_block_workgroups
    if (src_aligned(src) && (g.W & 3) == 0) hipLaunchKernelGGL(exr_layout_kernel<true>, dim3(row_wgs * (unsigned)g.H), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(exr_layout_kernel<false>, dim3(row_wgs * (unsigned)g.H), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    if (a.aov.planes) {      // the same grid; it reads the sums too, so ahead of after_layout
        const uintptr_t bits = reinterpret_cast<uintptr_t>(a.aov.dist) | reinterpret_cast<uintptr_t>(a.aov.s1) | reinterpret_cast<uintptr_t>(a.aov.s2);
        if ((bits & 15u) == 0u && (g.W & 3) == 0) hipLaunchKernelGGL(exr_aov_layout_kernel<true>, dim3(row_wgs * (unsigned)g.H), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(exr_aov_layout_kernel<false>, dim3(row_wgs * (unsigned)g.H), dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    { int rc = after_layout(); if (rc) return rc; }
    if (g.compression != DE_EXR_COMPRESSION_NONE) {
        hipLaunchKernelGGL(exr_predict_kernel, dim3(block_wgs * (unsigned)g.blocks), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(exr_deflate_kernel, dim3((unsigned)g.pieces), dim3(PNG_THREADS), 0, stream, a);
    }
    hipLaunchKernelGGL(exr_block_kernel, dim3((unsigned)((g.blocks + 255) / 256)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(exr_scan_kernel, dim3(1), dim3(CS_SCAN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(exr_compact_kernel, dim3((unsigned)g.pieces), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return DE_OK;
}
// What the AOV channels in force refuse before anything is enqueued.  The variance is this context's own sums beside its own S2: not with a display
// source (the sums shown are another buffer's, S2 is not) and not under a tile or sample partition (this rank's S2 is a part's), as the denoiser,
// S2's other reader, refuses (denoise_refusal); and not without a complete S2.  The guides' own refusal, before maps and LUTs, is de_fetch_guides'.
int ex_aov_refusal(de_ctx* c) {
    if (c->ex_aovs & DE_EXR_AOV_VARIANCE) {
        if (c->display_src) return fail(DE_ERR_STATE, "the EXR variance channels describe this context's own frame: not with a display source or after de_reduce_progressive");
        if (c->tiles_world > 1) return fail(DE_ERR_STATE, "the EXR variance channels describe whole frames: not under a tile partition");
        if (c->sample_world > 1) return fail(DE_ERR_STATE, "the EXR variance channels describe whole frames: not under a sample partition");
    }
    if ((c->ex_aovs & DE_EXR_AOV_VARIANCE) && !(c->d_s2 && (c->dn_s2_complete || c->frame_kind == DE_FRAME_ADAPTIVE)))
        return fail(DE_ERR_STATE, "the EXR variance channels need the sums of squares of every sample of this frame: turn the denoiser on (de_set_denoise) before the frame's first sample, or render adaptively");
    return DE_OK;
}
int ex_length(const void* word, uint64_t* len) {      // its coders raise no range status
    static const char* const text = "the EXR encoder met a piece longer than its proven worst case: nothing was written past a buffer";
    return coded_read_word(word, len, text, text);
}
struct ExrOut {      // the descriptor of de_fetch.h's entry points and of linear_render
    static constexpr const char* too_small = "out_bytes is smaller than the file (*len; de_exr_capacity bounds every frame)";
    static constexpr const char* buffers = "EXR buffers";
    static CodedOut& coded(de_ctx* c) { return c->ex_coded; }
    static int source(const de_ctx* c) { return c->ex.source; }
    static uint32_t aovs(const de_ctx* c, const LinearFrame& f) { return f.env ? 0u : c->ex_aovs; }      // B, G, R alone in the panorama
    static ExrGeometry geometry(const de_ctx* c) { const LinearFrame f = linear_frame(c); return ex_geometry(f.W, f.H, c->ex, aovs(c, f)); }
    static int size_refusal(const de_ctx* c) { const LinearFrame f = linear_frame(c); return ex_shape_check(f.W, f.H, c->ex.pixel_type, aovs(c, f)); }
    static int refusal(const de_ctx* c) {
        int rc = linear_pano_refusal(c, "EXR");
        if (!rc && c->pano.on && c->ex_aovs) rc = fail(DE_ERR_STATE, "the panorama is on (de_set_panorama): a scene-linear panorama has no AOV channels (de_set_exr_aovs(ctx, 0) first)");
        return rc ? rc : size_refusal(c);
    }
    static size_t first_prefix(const ExrGeometry& g) { return g.front + g.raw / 2; }      // the front and half the raw bytes
    static int render(de_ctx* c, Dev<uint8_t>& dev, int) { return linear_render<ExrOut>(c, dev); }
    static bool reads_panorama(const de_ctx* c) { return env_active(c); }
    static int length(const void* word, uint64_t* len) { return ex_length(word, len); }
    // of the frame alone, where the AOV channels live: their refusal, then the guides of the frame's geometry, whatever the source — made if stale, as
    // for de_fetch_guides and the denoiser
    static int frame_prepare(de_ctx* c) {
        int rc = ex_aov_refusal(c);
        if (!rc && (c->ex_aovs & (DE_EXR_AOV_DEPTH | DE_EXR_AOV_NORMAL | DE_EXR_AOV_ALBEDO | DE_EXR_AOV_COVERAGE | DE_EXR_AOV_TRANSMITTANCE))) rc = guides_of_the_frame(c);
        return rc;
    }
    static int work(de_ctx* c, const ExrGeometry& g) {
        int rc = ex_work_ensure(c->ex_work, g);
        if (rc) return rc;
        HIP_TRY(ex_tables_upload(c->stream, c->ex_work));
        return DE_OK;
    }
    template <class After>
    static int launch(de_ctx* c, const ExrGeometry& g, const DisplaySrc& src, uint8_t* out, After after) {
        ExrAovSrc av;      // the frame's own sums and counts, whatever the source: a stage's mean has no S2
        if (c->ex_aovs) {
            av.nc = c->d_dn_nc; av.at = c->d_dn_at; av.dist = c->d_dn_dist;
            av.s1 = c->d_hdr; av.s2 = c->d_s2;      // the context's own sums beside its own S2 (ex_aov_refusal: no display source)
            av.tile_spp = c->frame_kind == DE_FRAME_ADAPTIVE ? c->d_tile_spp : nullptr; av.samples = c->current_spp;
        }
        return ex_launch(c->stream, c->ex_work, g, src, true, c->ex.scale, out, after, av);
    }
};

// ---- Radiance HDR output (include/digital_earth_rgbe.h, rgbe_kernels.hip, rgbe_tables.h): where the EXR output sits, another file
int rg_settings_check(const de_rgbe* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_rgbe)) return fail(DE_ERR_INVALID, "de_rgbe.struct_bytes does not match this library's struct");
    if (s->source < DE_EXR_SOURCE_MEAN || s->source > DE_EXR_SOURCE_LOCAL_EXPOSURE) return fail(DE_ERR_INVALID, "de_rgbe.source must be DE_EXR_SOURCE_MEAN, _DENOISED, _HISTORY, _BLOOM or _LOCAL_EXPOSURE");
    if (s->rle != 0 && s->rle != 1) return fail(DE_ERR_INVALID, "de_rgbe.rle must be 0 or 1");
    if (s->rounding != DE_RGBE_ROUND_TRUNC && s->rounding != DE_RGBE_ROUND_NEAREST) return fail(DE_ERR_INVALID, "de_rgbe.rounding must be DE_RGBE_ROUND_TRUNC or _NEAREST");
    if (!(s->scale > 0.0f) || !(s->scale < INFINITY)) return fail(DE_ERR_INVALID, "de_rgbe.scale must be finite and greater than 0");      // NaN fails the first
    return DE_OK;
}
int rg_shape_check(int W, int H) {      // what one conversion can take: the kernels count bytes in 32 bits
    if (W <= 0 || H <= 0) return fail(DE_ERR_INVALID, "an RGBE frame needs W, H >= 1");
    if (4ull * (unsigned long long)W * (unsigned long long)H > RGBE_MAX_FLAT) return fail(DE_ERR_INVALID, "the RGBE output takes at most 2^27 flat bytes, 4 W H");
    return DE_OK;
}
RgbeGeometry rg_geometry(int W, int H, const de_rgbe& s) { return rgbe_geometry(W, H, s.rle, s.scale); }
// The buffers of one conversion of geometry g; `words` holds len[pieces], offset[pieces] and the status word.  Flat rows need the word alone.
int rg_work_ensure(de_ctx::RgbeWork& w, const RgbeGeometry& g) {
    int rc = w.planes.ensure(g.rle ? g.pieces * g.plane_stride : 16, "RGBE buffers");
    if (!rc) rc = w.slots.ensure(g.rle ? g.pieces * g.slot_bytes : 16, "RGBE buffers");
    if (!rc) rc = w.words.ensure((2 * g.pieces + 4) * sizeof(uint32_t), "RGBE buffers");
    return rc;
}
// src (on this stream) -> the planar bytes -> slots -> the file at `out`; flat rows straight into the file.  `after_convert` runs behind the one
// kernel that reads `src`.
template <class AfterConvert>
int rg_launch(hipStream_t stream, const de_ctx::RgbeWork& w, const RgbeGeometry& g, const DisplaySrc& src, bool flip, int rounding, uint8_t* out, AfterConvert after_convert) {
    RgbeArgs a;
    a.src = src; a.flip = flip ? 1 : 0; a.scale = g.scale; a.rounding = rounding; a.rle = g.rle; a.planes = w.planes; a.slots = w.slots;
    a.len = w.words; a.offset = w.words + g.pieces; a.status = w.words + 2 * g.pieces; a.out = out;
    a.W = (uint32_t)g.W; a.H = (uint32_t)g.H; a.plane_stride = (uint32_t)g.plane_stride; a.header = (uint32_t)g.header;
    a.count = (uint32_t)g.pieces; a.slot_bytes = (uint32_t)g.slot_bytes;
    a.front = (uint32_t)g.front; a.extra = 0u; a.trailer = 0u; a.capacity = (uint32_t)g.capacity;
    memcpy(a.front_bytes, g.text, sizeof(a.front_bytes));
    const unsigned row_wgs = (unsigned)((((size_t)g.W + 3) / 4 + 255) / 256);      // rgbe_row_workgroups
    if (src_aligned(src) && (g.W & 3) == 0) hipLaunchKernelGGL(rgbe_convert_kernel<true>, dim3(row_wgs * (unsigned)g.H), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(rgbe_convert_kernel<false>, dim3(row_wgs * (unsigned)g.H), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    { int rc = after_convert(); if (rc) return rc; }
    if (g.rle) hipLaunchKernelGGL(rgbe_code_kernel, dim3((unsigned)g.pieces), dim3(RGBE_THREADS), g.plane_stride, stream, a);      // the plane is its dynamic LDS
    hipLaunchKernelGGL(rgbe_scan_kernel, dim3(1), dim3(CS_SCAN_THREADS), 0, stream, a);
    if (g.rle) hipLaunchKernelGGL(rgbe_compact_kernel, dim3((unsigned)g.pieces), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return DE_OK;
}
int rg_length(const void* word, uint64_t* len) {      // its coder raises no range status
    static const char* const text = "the RGBE encoder met a plane longer than its proven worst case: nothing was written past a buffer";
    return coded_read_word(word, len, text, text);
}
struct RgbeOut {      // as ExrOut
    static constexpr const char* too_small = "out_bytes is smaller than the file (*len; de_rgbe_capacity bounds every frame)";
    static constexpr const char* buffers = "RGBE buffers";
    static CodedOut& coded(de_ctx* c) { return c->rg_coded; }
    static int source(const de_ctx* c) { return c->rg.source; }
    static RgbeGeometry geometry(const de_ctx* c) { const LinearFrame f = linear_frame(c); return rg_geometry(f.W, f.H, c->rg); }
    static int size_refusal(const de_ctx* c) { const LinearFrame f = linear_frame(c); return rg_shape_check(f.W, f.H); }
    static int refusal(const de_ctx* c) { int rc = linear_pano_refusal(c, "RGBE"); return rc ? rc : size_refusal(c); }
    static size_t first_prefix(const RgbeGeometry& g) { return g.header + 2 * (size_t)g.W * (size_t)g.H; }      // the front and half the flat bytes
    static int render(de_ctx* c, Dev<uint8_t>& dev, int) { return linear_render<RgbeOut>(c, dev); }
    static bool reads_panorama(const de_ctx* c) { return env_active(c); }
    static int length(const void* word, uint64_t* len) { return rg_length(word, len); }
    static int frame_prepare(de_ctx*) { return DE_OK; }
    static int work(de_ctx* c, const RgbeGeometry& g) { return rg_work_ensure(c->rg_work, g); }      // no table
    template <class After>
    static int launch(de_ctx* c, const RgbeGeometry& g, const DisplaySrc& src, uint8_t* out, After after) {
        return rg_launch(c->stream, c->rg_work, g, src, true, c->rg.rounding, out, after);
    }
};
}  // namespace

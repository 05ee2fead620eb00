// de_api.hip — the C ABI of libdigitalearth_hip.so (include/digital_earth.h): context life cycle, uploads, parameters, the frame loop, fetches.
// No CPU fallback exists: every entry point needs a HIP device.  The launches are in de_launch.h, the collectives in de_rccl.h, the display path's stages
// and their one chain in de_display.h, how an output leaves the GPU (staging, rings, the packed outputs' frame, the coded outputs' entry points over a format's descriptor and their debug frame) in de_fetch.h, the context in
// de_context.h, the owner of all its memory (Dev<T>, Pinned<T>: nothing here allocates or frees by hand) in de_memory.h; the kernel families the product no longer runs hang in under -DDE_LEGACY_VARIANTS (legacy/).  This file holds entry points only.
#include "de_rccl.h"
#include "de_display.h"

namespace {
// A launch slot's stream.  withhold > 0: the stream may use every CU but the LAST `withhold` of each XCD (hipExtStreamCreateWithCUMask; bit i of the mask is
// CU i / 8 of XCD i % 8 — the driver deals the mask's bits round robin over the XCDs — so the top 8 x withhold bits are `withhold` CUs of every XCD):
// persistent workgroups then leave those CUs to the small kernels of the context stream (collective, accumulate, display).
hipError_t create_slot_stream(de_ctx* c, hipStream_t* out) {
    if (c->cu_withhold <= 0) return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
    const int n = c->n_cus, keep = n - 8 * c->cu_withhold;
    if (keep < 8) return hipErrorInvalidValue;
    uint32_t mask[16];
    memset(mask, 0, sizeof(mask));
    for (int i = 0; i < keep && i < 512; ++i) mask[i >> 5] |= 1u << (i & 31);
    return hipExtStreamCreateWithCUMask(out, (uint32_t)((n + 31) / 32), mask);
}
// A launch slot: its stream and its three events.  de_create makes the first n_slots, de_set_launch_slots the ones that did not exist yet.
hipError_t create_slot(de_ctx* c, LaunchSlot& s) {
    if (s.stream) return hipSuccess;
    HIP_RET(create_slot_stream(c, &s.stream));
    HIP_RET(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    HIP_RET(hipEventCreate(&s.t0));
    return hipEventCreate(&s.t1);
}
// The context's own stream carries the small operations between frames and the collective: highest priority, so that wave slots freed by the draining
// render kernels of the launch slots go to them first.
hipError_t create_context_stream(hipStream_t* out) {
    int prio_lo = 0, prio_hi = 0;
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    return hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio_hi);
}
// What every context holds from de_create on: its stream, the launch slots, the frame's buffers and tables.  Everything else is allocated on first use.
hipError_t create_resources(de_ctx* c) {
    const size_t npx = (size_t)c->W * c->H;
    HIP_RET(create_context_stream(&c->stream));
    c->own_stream = true;
    for (int i = 0; i < c->n_slots; ++i) HIP_RET(create_slot(c, c->slot[i]));      // launches in flight per context (de_set_launch_slots; 1 = every launch waits for the previous one)
    HIP_RET(hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming));
    HIP_RET(c->d_hdr_own.ensure(npx * 3 * sizeof(float)));
    c->d_hdr = c->d_hdr_own;
    HIP_RET(c->d_image.ensure(npx * 3 * sizeof(float)));
    HIP_RET(c->d_scratch.ensure(npx * 4 * sizeof(float)));
    HIP_RET(c->d_fc.ensure(sizeof(FrameConsts)));
    HIP_RET(c->d_nodes.ensure(DE_N_NODES * sizeof(LambdaNode)));
    HIP_RET(c->d_node_val.ensure(256 * sizeof(float)));
    HIP_RET(c->d_counters.ensure(DE_N_COUNTERS * sizeof(unsigned long long)));
    HIP_RET(c->d_work_counter.ensure(16 * (DE_MAX_SLOTS + 1) * sizeof(uint32_t)));
    HIP_RET(c->d_dens_table.ensure((size_t)DE_DENS_TABLE_N * DE_DENS_STRIDE * sizeof(float)));
    HIP_RET(c->d_cie.ensure(441 * 2 * 3 * sizeof(float)));
    HIP_RET(c->d_srgb2spec.ensure(900 * sizeof(float)));
    HIP_RET(c->d_o3.ensure(441 * sizeof(float)));
    HIP_RET(hipMemsetAsync(c->d_hdr, 0, npx * 3 * sizeof(float), c->stream));
    HIP_RET(hipMemsetAsync(c->d_counters, 0, DE_N_COUNTERS * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(dens_table_kernel, dim3((DE_DENS_TABLE_N + 255) / 256), dim3(256), 0, c->stream, c->d_dens_table);
    return hipGetLastError();
}

}  // namespace

extern "C" {

const char* de_last_error(void) { return g_err.c_str(); }
int de_abi_version(void) { return DE_ABI_VERSION; }
int de_arithmetic_contract(void) { return DE_ARITHMETIC_CONTRACT; }

int de_create(int device, int width, int height, de_ctx** out) {
    if (!out) return fail(DE_ERR_INVALID, "out is null");
    if (width <= 0 || height <= 0 || width % 16 || height % 8)
        return fail(DE_ERR_INVALID, "image size must be a positive multiple of (16, 8) (renderer.py:46)");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(DE_ERR_NO_DEVICE, "no HIP device: libdigitalearth_hip has no CPU path");
    if (device < 0 || device >= n_dev) return fail(DE_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DE_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    de_ctx* c = new de_ctx();
    c->device = device; c->W = width; c->H = height;
    default_params(&c->p);
#ifdef DE_LEGACY_VARIANTS
    read_legacy_env(c);       // the legacy library keeps the experiment knobs of rounds 1-4 in the environment; the product reads none (de_set_tuning)
#endif
    memset(&c->counters, 0, sizeof(c->counters));
    c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const hipError_t e = create_resources(c);
    if (e != hipSuccess) {
        std::string msg = std::string("de_create: ") + hipGetErrorString(e);
        de_destroy(c);
        return fail(e == hipErrorOutOfMemory ? DE_ERR_NOMEM : DE_ERR_HIP, msg);
    }
    *out = c;
    return DE_OK;
}

int de_destroy(de_ctx* c) {
    if (!c) return DE_OK;
    if (c->loans > 0) return fail(DE_ERR_STATE, "this context lends its maps to another one (de_share_textures): destroy the borrowers first");
    hipSetDevice(c->device);
    for (int i = 0; i < DE_MAX_SLOTS; ++i) if (c->slot[i].stream) hipStreamSynchronize(c->slot[i].stream);
    hipStreamSynchronize(c->stream);
    if (c->comm && g_rccl.CommDestroy) { g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
    release_loan(c);
    // events and streams; the memory is the members' (de_memory.h): `delete c` frees what this context owns and leaves what it borrows
    for (FetchRing* r : {&c->img, &c->px_ring, &c->vd_ring, &c->jp_coded.ring, &c->pn_coded.ring, &c->ex_coded.ring, &c->rg_coded.ring}) ring_destroy_events(*r);
#ifdef DE_LEGACY_VARIANTS
    destroy_legacy_events(c);
#endif
    for (int i = 0; i < DE_MAX_SLOTS; ++i) {
        LaunchSlot& s = c->slot[i];
        if (s.done) hipEventDestroy(s.done);
        if (s.t0) hipEventDestroy(s.t0);
        if (s.t1) hipEventDestroy(s.t1);
        if (s.stream) hipStreamDestroy(s.stream);
    }
    if (c->ev_main) hipEventDestroy(c->ev_main);
    if (c->ev_r0) hipEventDestroy(c->ev_r0);
    if (c->ev_r1) hipEventDestroy(c->ev_r1);
    for (auto& pair : c->ev_standin) for (hipEvent_t ev : pair) if (ev) hipEventDestroy(ev);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;
    return DE_OK;
}

int de_upload_texture(de_ctx* c, int slot, const uint8_t* texels, int w, int h, int channels) {
    if (!c || slot < 0 || slot >= DE_TEX_COUNT || !texels || w <= 0 || h <= 0) return fail(DE_ERR_INVALID, "bad texture arguments");
    const bool colour = (slot == DE_TEX_ALBEDO || slot == DE_TEX_STARS);
    if (channels != (colour ? 3 : 1)) return fail(DE_ERR_INVALID, "albedo/stars take 3 channels, the grey maps 1");
    HIP_TRY(hipSetDevice(c->device));
    int rc = alloc_texture(c, slot, w, h, channels);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->tex[slot].linear, texels, (size_t)w * h * channels, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->tex[slot].set = true;
    c->dn_guides_valid = false;
    hs_drop(c);
    if (slot == DE_TEX_TOPOGRAPHY) c->params_dirty = true;
    return DE_OK;
}

int de_generate_texture(de_ctx* c, int slot, int w, int h, uint32_t seed, int variant) {
    if (!c || slot < 0 || slot >= DE_TEX_COUNT || w <= 0 || h <= 0) return fail(DE_ERR_INVALID, "bad texture arguments");
    HIP_TRY(hipSetDevice(c->device));
    const bool colour = (slot == DE_TEX_ALBEDO || slot == DE_TEX_STARS);
    int rc = alloc_texture(c, slot, w, h, colour ? 3 : 1);
    if (rc) return rc;
    dim3 grid((unsigned)((w + 255) / 256), (unsigned)h);
    hipLaunchKernelGGL(synth_kernel, grid, dim3(256), 0, c->stream, c->tex[slot].linear, slot, w, h, seed, variant);
    HIP_TRY(hipGetLastError());
    c->tex[slot].set = true;
    c->dn_guides_valid = false;
    hs_drop(c);
    if (slot == DE_TEX_TOPOGRAPHY) c->params_dirty = true;
    return DE_OK;
}

int de_share_textures(de_ctx* dst, de_ctx* src) {
    if (!dst || !src || dst == src) return fail(DE_ERR_INVALID, "two different contexts are needed");
    if (dst->device != src->device) return fail(DE_ERR_INVALID, "contexts on different devices cannot share maps");
    if (src->lender) return fail(DE_ERR_STATE, "the lending context borrows its maps itself: share from their owner");
    if (dst->loans > 0) return fail(DE_ERR_STATE, "the borrowing context lends its own maps to another one");
    for (int i = 0; i < DE_TEX_COUNT; ++i)
        if (!src->tex[i].set) return fail(DE_ERR_STATE, "the lending context must hold all 7 maps");
    if (!src->luts_set) return fail(DE_ERR_STATE, "the lending context must hold the LUTs");
    HIP_TRY(hipSetDevice(src->device));
    // bring the lender's packed copies up to date for ITS address mode, then wait: the borrower reads them from other streams
    const bool clamp = (src->p.flags & DE_FLAG_CLAMP_SAMPLER) != 0;
    for (int i = 0; i < DE_TEX_COUNT; ++i) { int rc = ensure_packed(src, i, clamp); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(src->stream));
    { int rc = sync_all(dst); if (rc) return rc; }
    release_loan(dst);
    for (int i = 0; i < DE_TEX_COUNT; ++i) {
        DevTexture& t = dst->tex[i];
        const DevTexture& s = src->tex[i];
        t.linear.release();       // the as-uploaded copy stays the lender's alone: de_download_texture on the borrower fails cleanly
        t.packed.borrow(s.packed); t.bound.borrow(s.bound);      // (the cloud map's occupancy bound with it)
        t.w = s.w; t.h = s.h; t.ch = s.ch; t.tiles_x = s.tiles_x; t.tiles_y = s.tiles_y; t.packed_clamp = s.packed_clamp; t.set = s.set;
    }
    dst->d_cie.borrow(src->d_cie); dst->d_srgb2spec.borrow(src->d_srgb2spec); dst->d_o3.borrow(src->d_o3); dst->d_crf.borrow(src->d_crf);
    dst->n_crf = src->n_crf; dst->luts_set = true;
    dst->params_dirty = true; dst->nodes_dirty = true;
    // the loan is on record: while it lasts the lender refuses to free, replace or repack its maps and LUTs, and to be destroyed
    dst->lender = src; src->loans++;
    dst->dn_guides_valid = false;
    hs_drop(dst);
    touched_render_inputs(dst);
    return DE_OK;
}

int de_trim_textures(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    const bool clamp = (c->p.flags & DE_FLAG_CLAMP_SAMPLER) != 0;
    for (int i = 0; i < DE_TEX_COUNT; ++i) {
        DevTexture& t = c->tex[i];
        if (!t.set || t.borrowed() || !t.linear) continue;
        int rc = ensure_packed(c, i, clamp);          // the packed copy must exist before its source goes (fails if that means repacking lent maps)
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < DE_TEX_COUNT; ++i) {
        DevTexture& t = c->tex[i];
        if (!t.set || t.borrowed() || !t.linear) continue;
        t.linear.release();
    }
    return DE_OK;
}

int de_download_texture(de_ctx* c, int slot, uint8_t* out, uint64_t out_bytes) {
    if (!c || slot < 0 || slot >= DE_TEX_COUNT || !out || !c->tex[slot].set) return fail(DE_ERR_INVALID, "texture not set");
    const DevTexture& t = c->tex[slot];
    if (t.borrowed()) return fail(DE_ERR_STATE, "this map is borrowed (de_share_textures): download it from the context that owns it");
    if (!t.linear) return fail(DE_ERR_STATE, "the as-uploaded copy of this map was released (de_trim_textures)");
    size_t n = (size_t)t.w * t.h * t.ch;
    if (out_bytes < n) return fail(DE_ERR_INVALID, "output buffer too small");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, t.linear, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DE_OK;
}

int de_texture_info(de_ctx* c, int slot, int* w, int* h, int* ch) {
    if (!c || slot < 0 || slot >= DE_TEX_COUNT) return fail(DE_ERR_INVALID, "bad slot");
    if (w) *w = c->tex[slot].w;
    if (h) *h = c->tex[slot].h;
    if (ch) *ch = c->tex[slot].ch;
    return DE_OK;
}

int de_upload_luts(de_ctx* c, const float* cie, const uint16_t* srgb2spec_f16, const float* o3, const float* crf, int n_crf) {
    if (!c || !cie || !srgb2spec_f16 || !o3 || !crf || n_crf <= 0) return fail(DE_ERR_INVALID, "bad LUT arguments");
    if (c->loans > 0) return fail(DE_ERR_STATE, "the LUTs are lent to another context (de_share_textures): destroy the borrowers first");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }
    touched_render_inputs(c);
    std::vector<float> q(441 * 2 * 3), s(900), r((size_t)1024 * n_crf * 3);
    for (int i = 0; i < 441 * 2 * 3; ++i) q[i] = quantize_f16(cie[i]);
    for (int i = 0; i < 900; ++i) s[i] = half_to_float(srgb2spec_f16[i]);
    for (int x = 0; x < 1024; ++x)
        for (int y = 0; y < n_crf; ++y)
            for (int ch = 0; ch < 3; ++ch) r[((size_t)y * 1024 + x) * 3 + ch] = crf[((size_t)x * n_crf + y) * 3 + ch];
    if (c->luts_borrowed()) {                // stop borrowing: own copies again
        c->d_cie.release(); c->d_srgb2spec.release(); c->d_o3.release();
        if (!borrows_anything(c)) release_loan(c);
    }
    HIP_TRY(c->d_cie.ensure(441 * 2 * 3 * sizeof(float)));      // (held since de_create unless they were borrowed)
    HIP_TRY(c->d_srgb2spec.ensure(900 * sizeof(float)));
    HIP_TRY(c->d_o3.ensure(441 * sizeof(float)));
    c->d_crf.release();                      // sized by n_crf
    HIP_TRY(c->d_crf.ensure(r.size() * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(c->d_cie, q.data(), q.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_srgb2spec, s.data(), s.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_o3, o3, 441 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_crf, r.data(), r.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->n_crf = n_crf; c->luts_set = true; c->params_dirty = true; c->nodes_dirty = true;
    hs_drop(c);
    return DE_OK;
}

int de_set_params(de_ctx* c, const de_params* p) {
    if (!c || !p) return fail(DE_ERR_INVALID, "null argument");
    if (p->flags != c->p.flags || memcmp(&p->fixed_wavelength, &c->p.fixed_wavelength, sizeof(float)) != 0) c->nodes_dirty = true;
    // the denoiser's guides depend on the camera, the terrain scale and the address mode; exposure, CRF, gamma and the vignette do not
    if (memcmp(p->camera_pos, c->p.camera_pos, 11 * sizeof(float)) != 0 || memcmp(&p->land_height_scale, &c->p.land_height_scale, sizeof(float)) != 0 ||
        ((p->flags ^ c->p.flags) & DE_FLAG_CLAMP_SAMPLER) != 0u || p->topo_res_override != c->p.topo_res_override) c->dn_guides_valid = false;
    if (hs_radiance_changed(c->p, *p)) hs_drop(c);      // the history shows another light: camera fields reproject, display-only fields keep it
    c->p = *p;
    c->params_dirty = true;
    return DE_OK;
}
int de_get_params(de_ctx* c, de_params* p) {
    if (!c || !p) return fail(DE_ERR_INVALID, "null argument");
    *p = c->p;
    return DE_OK;
}

int de_reset(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = join_slots(c); if (rc) return rc; }
    touched_hdr(c);
    HIP_TRY(hipMemsetAsync(c->d_hdr, 0, (size_t)c->W * c->H * 3 * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, DE_N_COUNTERS * sizeof(unsigned long long), c->stream));
    memset(&c->counters, 0, sizeof(c->counters));
    c->dn_guides_valid = false; c->dn_out_valid = false;
    c->dn_s2_complete = false;
    if (c->dn_on) {                        // the denoiser tracks S2 from the frame's first sample on (zeroed before the first accumulate: same stream, touched_hdr above)
        HIP_TRY(c->d_s2.ensure((size_t)c->W * c->H * 3 * sizeof(float)));
        HIP_TRY(hipMemsetAsync(c->d_s2, 0, (size_t)c->W * c->H * 3 * sizeof(float), c->stream));
        c->dn_s2_complete = true;
    }
    c->current_spp = 0;
    note_abort(c);                         // re-arm the abort words ...
    c->frame_invalid = false;              // ... a new frame starts
    if (c->display_src == c->d_assembled) c->display_src = nullptr;    // the assembled frame of a progressive reduce is history now
    c->frame_kind = DE_FRAME_NONE;         // the next de_accumulate or de_accumulate_adaptive starts the frame
    // history reprojection: what the frame's newest display showed becomes the history (a pointer swap: the launches that wrote it and the ones that will
    // read it are ordered by the context stream); without a display since the last swap the old history stays: it is still valid geometry
    if (c->hs_on && c->hs_cand_valid) { c->hs_cur ^= 1; c->hs_valid = true; c->hs_cand_valid = false; }
    return DE_OK;
}

int de_accumulate(de_ctx* c, int spp, uint64_t seed, int tile_rank, int tile_world) {
    if (!c || spp < 0 || tile_world < 1 || tile_rank < 0 || tile_rank >= tile_world) return fail(DE_ERR_INVALID, "bad accumulate arguments");
    if (c->frame_kind == DE_FRAME_ADAPTIVE) return fail(DE_ERR_STATE, "an adaptive frame is current (de_accumulate_adaptive): de_reset first");
    HIP_TRY(hipSetDevice(c->device));
    int rc = build_tiles(c, tile_rank, tile_world);
    if (rc) return rc;
    RenderArgs a;
    rc = fill_render_args(c, &a);
    if (rc) return rc;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    // Sample partition (renderer.py:371-380 dealt round robin): the call covers the frame's sample indices
    // [current_spp, current_spp + spp); this context renders those = sample_rank (mod sample_world) — first_index, first_index + world, ... —
    // and the frame's sample counter advances by the whole spp on every rank.
    const int frame_spp = spp;
    int first_index = c->current_spp;
    if (c->sample_world > 1) {
        const int rem = first_index % c->sample_world;
        first_index += (c->sample_rank - rem + c->sample_world) % c->sample_world;
        spp = first_index < c->current_spp + frame_spp ? (c->current_spp + frame_spp - first_index + c->sample_world - 1) / c->sample_world : 0;
    }
    a.spp_stride = c->sample_world;
    // S2 stays complete only while every sample goes through accumulate_moments_kernel (launch_accumulate): the denoiser on, no ray marcher, no per-lane loops
    if (!c->dn_on || (c->p.flags & DE_FLAG_RAY_MARCHER) || c->kernel_variant == 1) c->dn_s2_complete = false;
#ifdef DE_LEGACY_VARIANTS
    rc = accumulate_legacy(c, a, spp, first_index);
#else
    rc = accumulate_default(c, a, spp, first_index);
#endif
    if (rc) return rc;
    c->current_spp += frame_spp;
    c->frame_kind = DE_FRAME_UNIFORM;
    return DE_OK;
}

int de_set_sample_partition(de_ctx* c, int rank, int world) {
    if (!c || world < 1 || rank < 0 || rank >= world) return fail(DE_ERR_INVALID, "sample partition: 0 <= rank < world");
    c->sample_rank = rank; c->sample_world = world;      // read by the next de_accumulate; launches in flight keep what they were issued with
    return DE_OK;
}

int de_set_memory_budget(de_ctx* c, uint64_t bytes) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }
#ifdef DE_LEGACY_VARIANTS
    free_queue_memory(c);                 // what is held may exceed the new budget: the next large call allocates within it
#endif
    c->mem_budget = (size_t)bytes;        // the product's kernels need 37 MB per launch slot whatever the call: the budget binds the legacy pipeline's queues only
    return DE_OK;
}
int de_get_memory_use(de_ctx* c, uint64_t* queue_bytes) {
    if (!c || !queue_bytes) return fail(DE_ERR_INVALID, "null argument");
    uint64_t n = 0;
#ifdef DE_LEGACY_VARIANTS
    n += legacy_memory_use(c);
#endif
    for (auto& S : c->v6s) if (S.cold) n += (uint64_t)S.n_wg * DE_V6_P * sizeof(wf::Cold) + ((uint64_t)S.pool_cap[0] + S.pool_cap[1]) * DE_V6_POOL_ENTRY_BYTES;      // the per-CU scheduler: 37 MB per launch slot, whatever the call
    *queue_bytes = n;
    return DE_OK;
}

/* Phases of the LAST render_kernel_v6 launch of the last de_accumulate call, from the kernel's own clock (100 MHz): ms[0] = first workgroup start
 * to last wave exit, ms[1] = the DRAIN — from the first wave that found no work item left to the last wave's exit (the launch's last long
 * paths, which no scheduling shortens: what separates a rank's 1/N share of a frame from 1/N of the frame's time).  Waits for that launch.
 * DE_ERR_STATE when the last call did not run render_kernel_v6. */
int de_last_launch_phases(de_ctx* c, float* ms2) {
    if (!c || !ms2) return fail(DE_ERR_INVALID, "null argument");
    if (c->last_call[0] != 6 || c->last_slot < 0) return fail(DE_ERR_STATE, "the last de_accumulate did not run render_kernel_v6");
    HIP_TRY(hipSetDevice(c->device));
    de_ctx::V6State& S = c->v6s[c->last_slot];
    if (!S.ctl) return fail(DE_ERR_STATE, "no launch yet");
    HIP_TRY(hipStreamSynchronize(c->slot[c->last_slot].stream));
    unsigned long long t[3] = {0ull, 0ull, 0ull};
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemcpy(&t[k], S.ctl + (size_t)(bs::G_T_START + k) * DE_V6_CTL_STRIDE, 8, hipMemcpyDeviceToHost));
    ms2[0] = t[2] > t[0] ? (float)((double)(t[2] - t[0]) * 1e-5) : 0.f;
    ms2[1] = (t[2] > t[1] && t[1] != ~0ull) ? (float)((double)(t[2] - t[1]) * 1e-5) : 0.f;
    return DE_OK;
}

int de_last_call_info(de_ctx* c, int* variant, int* pipes, int* depths, int* launches) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (variant) *variant = c->last_call[0];
    if (pipes) *pipes = c->last_call[1];
    if (depths) *depths = c->last_call[2];
    if (launches) *launches = c->last_call[3];
    return DE_OK;
}

/* Make the context stream wait (on the device) for every launch issued so far.  Needed only by a host framework that enqueues
 * its OWN work on the stream it handed to de_set_stream — e.g. a torch.distributed reduce of the bound HDR tensor; the
 * library's own entry points (fetch, reduce, reset, display ...) do it themselves. */
int de_flush(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    int rc = join_slots(c);
    if (rc) return rc;
    touched_hdr(c);          // whatever the host enqueues next on the stream may touch the HDR buffer
    return frame_status(c);  // an abort already known (the words are host-visible): a host framework's own collective must not ship that frame
}

/* de_render_to_image (capture_face < 0), and de_panorama_capture's half of it (capture_face = 0 ... 5: the chain, the display launch and the look as
 * they stand, then the displayed image into that face's slot instead of the stage that makes the shown image; include/digital_earth_panorama.h). */
static int render_to_image_or_slot(de_ctx* c, const float** device_image, int capture_face);

int de_render_to_image(de_ctx* c, const float** device_image) { return render_to_image_or_slot(c, device_image, -1); }

static int render_to_image_or_slot(de_ctx* c, const float** device_image, int capture_face) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    const bool capture = capture_face >= 0;
    if (!capture && c->pano.on) {      // the shown image is made of the six captured faces alone: the frame as it stands is not displayed, nothing of it is read
        int rc = pano_refusal(c);      // ahead of everything: a refused call changes nothing
        if (rc) return rc;
        HIP_TRY(hipSetDevice(c->device));
        rc = run_panorama(c);
        if (rc) return rc;
        if (device_image) *device_image = shown_image(c);
        return DE_OK;
    }
    DisplayArgs d;
    bool per_tile;
    int rc = display_chain(c, STOP_IMAGE, &d, &per_tile);
    if (rc) return rc;
    const dim3 grid = tiles32(c);
    if (c->ho.on) {              // the HDR display output: the same launch over the same arguments, the settings' constants by value
        if (per_tile) hipLaunchKernelGGL(hdr_display_kernel<true>, grid, dim3(256), 0, c->stream, d, c->ho_consts);
        else hipLaunchKernelGGL(hdr_display_kernel<false>, grid, dim3(256), 0, c->stream, d, c->ho_consts);
    }
    else if (per_tile) hipLaunchKernelGGL(display_kernel<true>, grid, dim3(256), 0, c->stream, d);    // every tile divided by its own count
    else hipLaunchKernelGGL(display_kernel<false>, grid, dim3(256), 0, c->stream, d);
    HIP_TRY(hipGetLastError());
    // what the next accumulate_kernel must wait for ends HERE (the display has read the HDR buffer): recorded now, not lazily at the next de_accumulate, so that
    // a device-to-host copy of the image enqueued behind the display (de_fetch_image_begin) does not hold the next frame's sums back
    HIP_TRY(hipEventRecord(c->ev_main, c->stream));
    c->rec_render = c->gen_render; c->rec_hdr = c->gen_hdr;
    if (c->lk_on) {              // the look LUTs, in place on d_image; behind ev_main too: the stage reads nothing the next frame's sums write
        lk_launch(c->stream, c->d_image, (uint64_t)c->W * (uint64_t)c->H, c->lk, c->lk_dev);
        HIP_TRY(hipGetLastError());
    }
    if (capture) {               // behind the look, ahead of any pack: the displayed image into the face's slot
        const size_t n = (size_t)c->W * (size_t)c->W * 3;
        HIP_TRY(hipMemcpyAsync(c->pano_faces + (size_t)capture_face * n, c->d_image, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        c->pano_mask |= 1u << capture_face;
        return DE_OK;
    }
    if (os_active(c)) { rc = run_output_scale(c); if (rc) return rc; }      // behind ev_main: the next frame's sums do not wait for the resampling
    if (device_image) *device_image = shown_image(c);
    return DE_OK;
}

int de_fetch_image(de_ctx* c, float* out) {
    if (!out) return fail(DE_ERR_INVALID, "out is null");
    int rc = de_render_to_image(c, nullptr);
    if (rc) return rc;
    return copy_out(c, out, shown_image(c), out_image_bytes(c));
}

int de_fetch_image_view(de_ctx* c, const float** host_image) {
    if (!host_image) return fail(DE_ERR_INVALID, "host_image is null");
    if (!c) return fail(DE_ERR_INVALID, "null context");
    return fetch_staged(c, c->h_stage, c->img.noun, de_render_to_image, out_image_bytes(c), out_image_bytes(c), host_image);
}

/* The window loop pipelined (include/digital_earth.h; de_fetch.h: the lagged path), through the float image's ring. */
int de_fetch_image_begin(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    return ring_begin(c, c->img, de_render_to_image, out_image_bytes(c), out_image_bytes(c));
}
int de_fetch_image_end(de_ctx* c, const float** host_image) {
    if (!c || !host_image) return fail(DE_ERR_INVALID, "null argument");
    return ring_end(c, c->img, host_image);
}

int de_fetch_hdr(de_ctx* c, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = join_slots(c); if (rc) return rc; }
    touched_hdr(c);
    return fetch_transposed(c, c->display_src ? c->display_src : c->d_hdr, out);
}

int de_upload_hdr(de_ctx* c, const float* hdr, int spp) {
    if (!c || !hdr || spp < 0) return fail(DE_ERR_INVALID, "bad arguments");
    if (c->frame_kind == DE_FRAME_ADAPTIVE) return fail(DE_ERR_STATE, "an adaptive frame is current (de_accumulate_adaptive): de_reset first");
    HIP_TRY(hipSetDevice(c->device));
    size_t npx = (size_t)c->W * c->H;
    std::vector<float> t(npx * 3);
    to_device_layout(hdr, t.data(), c->W, c->H, 3);
    { int rc = join_slots(c); if (rc) return rc; }
    touched_hdr(c);
    HIP_TRY(hipMemcpyAsync(c->d_hdr, t.data(), npx * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->current_spp = spp;
    c->frame_kind = DE_FRAME_UNIFORM;
    c->dn_s2_complete = false;             // a checkpoint has no S2: the denoiser falls back on the spatial variance
    return DE_OK;
}
int de_current_spp(de_ctx* c, int* spp) { if (!c || !spp) return fail(DE_ERR_INVALID, "null argument"); *spp = c->current_spp; return DE_OK; }
int de_set_current_spp(de_ctx* c, int spp) {
    if (!c || spp < 0) return fail(DE_ERR_INVALID, "bad spp");
    if (c->frame_kind == DE_FRAME_ADAPTIVE) return fail(DE_ERR_STATE, "an adaptive frame keeps a sample count per tile: de_reset first");
    c->current_spp = spp;
    c->dn_s2_complete = false;
    return DE_OK;
}

/* One round of an adaptive frame (include/digital_earth.h).  The round is one accumulate_default call over the active list — sample indices
 * n .. n + r - 1, spp_stride 1, accumulate_moments_kernel instead of accumulate_kernel — then, on the context stream, the convergence test and the
 * compaction into the other list, and one host wait for the new number of active tiles (it sizes the next round's launch). */
int de_accumulate_adaptive(de_ctx* c, uint64_t seed, de_adaptive* io) {
    if (!c || !io) return fail(DE_ERR_INVALID, "null argument");
    if (io->struct_bytes != (uint32_t)sizeof(de_adaptive)) return fail(DE_ERR_INVALID, "de_adaptive.struct_bytes does not match this library's struct");
    if (io->min_spp < 2 || io->round_spp < 1 || io->min_spp > io->max_spp || !(io->threshold >= 0.0f) || !(io->floor >= 0.0f))
        return fail(DE_ERR_INVALID, "adaptive settings: 2 <= min_spp <= max_spp, round_spp >= 1, threshold >= 0, floor >= 0");
    if (c->frame_kind == DE_FRAME_UNIFORM) return fail(DE_ERR_STATE, "the current frame was started by de_accumulate / de_upload_hdr: de_reset first");
    if (c->sample_world > 1) return fail(DE_ERR_STATE, "an adaptive frame does not run under a sample partition");
    if (c->p.flags & DE_FLAG_RAY_MARCHER) return fail(DE_ERR_STATE, "the ray marcher writes the HDR buffer without per-sample records: no adaptive frame");
    const int n_tiles = (c->W / 8) * (c->H / 8);
    HIP_TRY(hipSetDevice(c->device));
    if (c->frame_kind != DE_FRAME_ADAPTIVE) {
        // frame start: S2 zeroed, every tile active with count 0
        HIP_TRY(c->d_s2.ensure((size_t)c->W * c->H * 3 * sizeof(float)));
        for (int k = 0; k < 2; ++k) HIP_TRY(c->d_alist[k].ensure((size_t)n_tiles * sizeof(uint32_t)));
        HIP_TRY(c->d_tile_spp.ensure((size_t)n_tiles * sizeof(int32_t)));
        HIP_TRY(c->d_keep.ensure((size_t)n_tiles * sizeof(uint32_t)));
        HIP_TRY(c->d_ad_count.ensure(sizeof(int32_t)));
        HIP_TRY(c->h_ad_count.ensure(sizeof(int32_t)));
        { int rc = join_slots(c); if (rc) return rc; }
        touched_hdr(c); touched_render_inputs(c);      // the launches read the list and read-modify-write S2 after this
        HIP_TRY(hipMemsetAsync(c->d_s2, 0, (size_t)c->W * c->H * 3 * sizeof(float), c->stream));
        hipLaunchKernelGGL(adaptive_start_kernel, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, c->stream, c->d_alist[0], c->d_tile_spp, n_tiles);
        HIP_TRY(hipGetLastError());
        c->ad_cur = 0; c->ad_active = n_tiles; c->ad_n = 0; c->ad_rounds = 0; c->ad_pixel_samples = 0;
        c->ad_seed = seed; c->ad_threshold = io->threshold; c->ad_floor = io->floor;
        c->ad_min = io->min_spp; c->ad_max = io->max_spp; c->ad_round = io->round_spp;
        c->current_spp = 0;
        c->frame_kind = DE_FRAME_ADAPTIVE;
        c->dn_s2_complete = true;          // every round runs accumulate_moments_kernel
    } else if (seed != c->ad_seed || memcmp(&io->threshold, &c->ad_threshold, sizeof(float)) != 0 || memcmp(&io->floor, &c->ad_floor, sizeof(float)) != 0 ||
               io->min_spp != c->ad_min || io->max_spp != c->ad_max || io->round_spp != c->ad_round) {
        return fail(DE_ERR_INVALID, "the seed and the settings of an adaptive frame are fixed until de_reset");
    }
    if (c->ad_active > 0) {
        const int r = std::min(c->ad_round, c->ad_max - c->ad_n);
        RenderArgs a;
        int rc = fill_render_args(c, &a);
        if (rc) return rc;
        a.tiles = c->d_alist[c->ad_cur]; a.n_tiles = c->ad_active;
        a.tiles_identity = c->ad_active == n_tiles ? 1 : 0;      // the list is stable and ascending: all tiles = the identity
        a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
        a.spp_stride = 1;
        rc = accumulate_default(c, a, r, c->ad_n);
        if (rc) return rc;
        // the test reads S1 / S2 and rewrites the counts; the compaction writes the list that no launch of this round reads
        rc = join_slots(c);
        if (rc) return rc;
        touched_hdr(c); touched_render_inputs(c);
        AdaptiveArgs t;
        t.hdr = c->d_hdr; t.s2 = c->d_s2; t.list = c->d_alist[c->ad_cur]; t.n_active = c->ad_active;
        t.tile_spp = c->d_tile_spp; t.keep = c->d_keep; t.W = c->W; t.tiles_x = c->W / 8;
        t.n = c->ad_n + r; t.round = r; t.stop = t.n >= c->ad_max ? 1 : 0;
        t.test = (t.n >= c->ad_min && c->ad_threshold > 0.0f) ? 1 : 0;      // threshold 0: no tile converges
        t.tau2 = c->ad_threshold * c->ad_threshold; t.floor2 = c->ad_floor * c->ad_floor;
        hipLaunchKernelGGL(adaptive_test_kernel, dim3((unsigned)(((size_t)c->ad_active * 64 + 255) / 256)), dim3(256), 0, c->stream, t);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(1024), 0, c->stream, c->d_alist[c->ad_cur], c->d_keep, c->ad_active, c->d_alist[c->ad_cur ^ 1], c->d_ad_count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->h_ad_count, c->d_ad_count, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));      // one wait per round: the next round's launch is sized by the count
        rc = frame_status(c);
        if (rc) return rc;
        c->ad_pixel_samples += 64ull * (unsigned long long)c->ad_active * (unsigned long long)r;
        c->ad_n += r; c->ad_rounds++;
        c->ad_active = *c->h_ad_count;
        c->ad_cur ^= 1;
        c->current_spp = c->ad_n;      // de_current_spp: the largest tile count (the active tiles always hold it)
    }
    if (io->tile_spp) {
        HIP_TRY(hipMemcpyAsync(io->tile_spp, c->d_tile_spp, (size_t)n_tiles * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    io->active_tiles = c->ad_active;
    io->rounds = c->ad_rounds;
    io->pixel_samples = (uint64_t)c->ad_pixel_samples;
    return DE_OK;
}

int de_debug_adaptive_moments(de_ctx* c, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (!c->d_s2) return fail(DE_ERR_STATE, "no adaptive frame has run on this context");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = join_slots(c); if (rc) return rc; }
    touched_hdr(c);
    return fetch_transposed(c, c->d_s2, out);
}

int de_hdr_device_ptr(de_ctx* c, void** ptr, uint64_t* n_floats) {
    if (!c || !ptr) return fail(DE_ERR_INVALID, "null argument");
    *ptr = c->d_hdr;
    if (n_floats) *n_floats = (uint64_t)c->W * c->H * 3;
    return DE_OK;
}
int de_bind_hdr(de_ctx* c, void* device_ptr, uint64_t n_floats) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }
    touched_hdr(c);
    c->dn_s2_complete = false;
    if (!device_ptr) { c->d_hdr = c->d_hdr_own; return DE_OK; }
    if (n_floats < (uint64_t)c->W * c->H * 3) return fail(DE_ERR_INVALID, "bound HDR buffer is smaller than W*H*3 floats");
    c->d_hdr = (float*)device_ptr;
    return DE_OK;
}
int de_set_stream(de_ctx* c, void* hip_stream) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    // NULL is HIP's null stream, as everywhere in HIP (a framework whose current stream IS the null stream — torch's default
    // stream — passes 0 here and must get exactly that stream, or its own work would not be ordered with the context's)
    c->stream = (hipStream_t)hip_stream; c->own_stream = false;
    touched_render_inputs(c); touched_hdr(c);      // whatever the new stream holds, the next launch is ordered after it
    return DE_OK;
}
int de_use_own_stream(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }
    if (c->own_stream) return DE_OK;
    hipStream_t s = nullptr;
    HIP_TRY(create_context_stream(&s));
    c->stream = s; c->own_stream = true;
    touched_render_inputs(c); touched_hdr(c);
    return DE_OK;
}
int de_synchronize(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }
    return frame_status(c);
}
int de_last_accumulate_ms(de_ctx* c, float* ms) {
    if (!c || !ms) return fail(DE_ERR_INVALID, "null argument");
    if (c->timing_empty) { *ms = 0.0f; return DE_OK; }      // the last call's share was empty: nothing was launched
    if (!c->timing_valid) return fail(DE_ERR_STATE, "no de_accumulate has been issued");
    HIP_TRY(hipSetDevice(c->device));
    // from the start of the call's first launch (after its waits) to the end of its last accumulate_kernel
    HIP_TRY(hipEventSynchronize(c->slot[c->t1_slot].t1));
    HIP_TRY(hipEventElapsedTime(ms, c->slot[c->t0_slot].t0, c->slot[c->t1_slot].t1));
    return DE_OK;
}
int de_set_kernel_variant(de_ctx* c, int variant) {
    if (!c || variant < 1 || variant > 6) return fail(DE_ERR_INVALID, "kernel variant must be 1 ... 6");
#ifndef DE_LEGACY_VARIANTS
    if (variant != 2 && variant != 4 && variant != 6)
        return fail(DE_ERR_INVALID, "kernel variants 1, 3 and 5 (per-lane loops, wavefront pipeline, HBM-queue scheduler) live in the legacy library: build with -DDE_LEGACY_VARIANTS (digital_earth_amd/build.py: build_legacy) and load it through DE_LIB_PATH");
#endif
    c->kernel_variant = variant; c->launch_variant = variant >= 4 ? 2 : variant;
    return DE_OK;
}

/* Every tuning knob of the product's kernels as ONE plain struct (include/digital_earth.h: de_tuning).  The library reads no environment
 * variable for them: a host that wants experiment overrides reads its own environment and calls this (the Python layer does: _native.py). */
int de_get_tuning(de_ctx* c, de_tuning* t) {
    if (!c || !t) return fail(DE_ERR_INVALID, "null argument");
    memset(t, 0, sizeof(*t));
    t->struct_bytes = (uint32_t)sizeof(de_tuning);
    t->kernel_variant = c->kernel_variant;
    t->launch_slots = c->n_slots; t->big_launch_slots = c->big_slots;
    t->v6_min_paths = (uint64_t)c->auto_v6_min_items;
    for (int k = 0; k < 3; ++k) { t->v6_service_area[k] = c->v6_svc_area[k]; t->v6_service_lanes[k] = c->v6_svc[k]; }
    t->v6_yield_max = c->v6_yield; t->v6_elsewhere_min = c->v6_elsewhere; t->v6_retry = c->v6_retry; t->v6_enter_min = c->v6_enter_min;
    t->v6_flat_min = c->v6_flat_min; t->v6_flat_again = c->v6_flat_again; t->v6_bands = c->v6_bands; t->v6_stats = c->v6_stats;
    t->v6_tail_levels = c->v6_tail_levels; t->v6_tail_min_paths = c->v6_tail_min_paths; t->v6_tail_when_alone = c->v6_tail_when_alone;
    for (int k = 0; k < 2; ++k) { t->v6_tail_export[k] = c->v6_tail_export[k]; t->v6_tail_grid[k] = c->v6_tail_grid[k]; }
    t->v2_pend = c->tune_pend; t->v2_heavy = c->tune_heavy; t->v2_b = c->tune_b; t->v2_gas = c->tune_gas; t->v2_chunk = c->tune_chunk;
    t->v2_waves_per_cu = c->tune_wpc; t->v2_max_spp = c->tune_max_spp;
    t->trace = c->trace ? 1 : 0;
    t->v6_cu_withhold = c->cu_withhold;
    return DE_OK;
}
int de_set_tuning(de_ctx* c, const de_tuning* t) {
    if (!c || !t) return fail(DE_ERR_INVALID, "null argument");
    if (t->struct_bytes != (uint32_t)sizeof(de_tuning)) return fail(DE_ERR_INVALID, "de_tuning.struct_bytes does not match this library's struct: fill it with de_get_tuning first");
    if (t->launch_slots < 1 || t->launch_slots > DE_MAX_SLOTS || t->big_launch_slots < 1 || t->big_launch_slots > DE_MAX_SLOTS) return fail(DE_ERR_INVALID, "launch slots must be 1..8");
    if (t->v2_chunk < 1 || t->v2_waves_per_cu < 1 || t->v2_waves_per_cu > 20 || t->v6_flat_again < 1 || t->v6_min_paths < 64) return fail(DE_ERR_INVALID, "tuning value out of range");
    for (int k = 0; k < 3; ++k) if (t->v6_service_lanes[k] < 1 || t->v6_service_lanes[k] > 64 || t->v6_service_area[k] < 0) return fail(DE_ERR_INVALID, "service thresholds out of range");
    if (t->v6_tail_levels < 0 || t->v6_tail_levels > 2) return fail(DE_ERR_INVALID, "v6_tail_levels must be 0..2");
    for (int k = 0; k < 2; ++k) if (t->v6_tail_export[k] < 1 || t->v6_tail_export[k] > 1024 || t->v6_tail_grid[k] < 1 || t->v6_tail_grid[k] > 4096) return fail(DE_ERR_INVALID, "tail settings out of range");
    if (t->v6_cu_withhold < 0 || 8 * t->v6_cu_withhold > c->n_cus - 8) return fail(DE_ERR_INVALID, "v6_cu_withhold: CUs per XCD withheld from the render streams, 0 .. (CUs / 8 - 1)");
    int rc = de_set_kernel_variant(c, t->kernel_variant);
    if (rc) return rc;
    if (t->v6_cu_withhold != c->cu_withhold) {
        // the launch slots' streams carry the mask: make them again (nothing may be in flight on them)
        HIP_TRY(hipSetDevice(c->device));
        rc = sync_all(c);
        if (rc) return rc;
        c->cu_withhold = t->v6_cu_withhold;
        for (int i = 0; i < DE_MAX_SLOTS; ++i) {
            LaunchSlot& sl = c->slot[i];
            if (!sl.stream) continue;
            HIP_TRY(hipStreamDestroy(sl.stream));
            sl.stream = nullptr;
            HIP_TRY(create_slot_stream(c, &sl.stream));
        }
    }
    if (t->launch_slots != c->n_slots || t->big_launch_slots != c->big_slots) { rc = de_set_launch_slots(c, t->launch_slots, t->big_launch_slots); if (rc) return rc; }
    c->auto_v6_min_items = (unsigned long long)t->v6_min_paths;
    for (int k = 0; k < 3; ++k) { c->v6_svc_area[k] = t->v6_service_area[k]; c->v6_svc[k] = t->v6_service_lanes[k]; }
    c->v6_yield = t->v6_yield_max; c->v6_elsewhere = t->v6_elsewhere_min; c->v6_retry = t->v6_retry; c->v6_enter_min = t->v6_enter_min;
    c->v6_flat_min = t->v6_flat_min; c->v6_flat_again = t->v6_flat_again; c->v6_bands = t->v6_bands == 8 ? 8 : 1; c->v6_stats = t->v6_stats;
    c->v6_tail_levels = t->v6_tail_levels; c->v6_tail_min_paths = t->v6_tail_min_paths; c->v6_tail_when_alone = t->v6_tail_when_alone != 0;
    for (int k = 0; k < 2; ++k) { c->v6_tail_export[k] = t->v6_tail_export[k]; c->v6_tail_grid[k] = t->v6_tail_grid[k]; }
    c->tune_pend = t->v2_pend; c->tune_heavy = t->v2_heavy; c->tune_b = t->v2_b; c->tune_gas = t->v2_gas; c->tune_chunk = t->v2_chunk;
    c->tune_wpc = t->v2_waves_per_cu; c->tune_max_spp = t->v2_max_spp;
    c->trace = t->trace != 0;
    return DE_OK;
}
int de_enable_counters(de_ctx* c, int enable) { if (!c) return fail(DE_ERR_INVALID, "null context"); c->count = enable != 0; return DE_OK; }
int de_get_counters(de_ctx* c, de_counters* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long h[16];
    { int rc = join_slots(c); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memset(out, 0, sizeof(*out));
    out->samples = h[0]; out->taps_r8 = h[1]; out->taps_rgb8 = h[2]; out->sphere_steps = h[3];
    out->tracking_steps = h[4]; out->vertices = h[5]; out->rng_draws = h[6];
    for (int i = 0; i < 9; ++i) out->reserved[i] = h[7 + i];   // scheduler statistics of render_kernel_v2 (see its MODE 1 epilogue)
    return DE_OK;
}


int de_set_display_source(de_ctx* c, const void* device_ptr) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    c->display_src = (const float*)device_ptr;
    return DE_OK;
}
int de_set_launch_slots(de_ctx* c, int n_slots, int n_big) {
    if (!c || n_slots < 1 || n_slots > DE_MAX_SLOTS || n_big < 1 || n_big > DE_MAX_SLOTS) return fail(DE_ERR_INVALID, "slot counts must be 1..8");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }
    for (int i = c->n_slots; i < n_slots; ++i) HIP_TRY(create_slot(c, c->slot[i]));          // slots that did not exist yet
    c->n_slots = n_slots; c->big_slots = n_big;
    c->next_slot = 0; c->last_slot = -1; c->last_v6_slot = -1;
    return DE_OK;
}
int de_set_wave_budget(de_ctx* c, int waves_per_cu) {
    if (!c || waves_per_cu < 1 || waves_per_cu > 20) return fail(DE_ERR_INVALID, "waves per CU must be 1..20");
    c->tune_wpc = waves_per_cu;
    return DE_OK;
}

/* the same for render_kernel_v6 (DE_V6_STATS=1): out[k] = word k of its ST_* list */
int de_debug_v6_stats(de_ctx* c, uint64_t* out, int n) {
    if (!c || !out || n < 0) return fail(DE_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }
    for (int k = 0; k < n; ++k) out[k] = 0;
    std::vector<uint32_t> h((size_t)bs::G_WORDS * DE_V6_CTL_STRIDE);
    for (auto& S : c->v6s) {
        if (!S.ctl) continue;
        HIP_TRY(hipMemcpy(h.data(), S.ctl, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int k = 0; k < n && k < bs::ST_N; ++k) { uint64_t v; memcpy(&v, &h[(size_t)(bs::G_STAT0 + k) * DE_V6_CTL_STRIDE], 8); out[k] += v; }
        for (int k = 64; k < n && k < 128; ++k) { uint64_t v; memcpy(&v, &h[(size_t)(bs::G_STAT2 + k - 64) * DE_V6_CTL_STRIDE], 8); out[k] += v; }      // region statistics
        for (int k = 128; k < n && k < 192; ++k) { uint64_t v; memcpy(&v, &h[(size_t)(bs::G_DRAIN + k - 128) * DE_V6_CTL_STRIDE], 8); out[k] += v; }      // the drain's population histogram
    }
    return DE_OK;
}

int de_debug_cloud_bound(de_ctx* c, uint8_t* out, uint64_t out_bytes, int* cells_per_edge, uint32_t* budget_m) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (cells_per_edge) *cells_per_edge = DE_CLOUD_BOUND_N;
    if (budget_m) *budget_m = DE_CLOUD_BOUND_R;
    if (!out) return DE_OK;
    if (out_bytes < DE_CLOUD_BOUND_BYTES) return fail(DE_ERR_INVALID, "output buffer too small");
    if (!c->tex[DE_TEX_CLOUDS].set) return fail(DE_ERR_STATE, "no cloud map");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = ensure_packed(c, DE_TEX_CLOUDS, (c->p.flags & DE_FLAG_CLAMP_SAMPLER) != 0); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(out, c->tex[DE_TEX_CLOUDS].bound, DE_CLOUD_BOUND_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DE_OK;
}

int de_debug_sched_stats(de_ctx* c, uint64_t* out, int n) {
    if (!c || !out || n < 0 || n > DE_N_COUNTERS - 16) return fail(DE_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long h[DE_N_COUNTERS];
    { int rc = join_slots(c); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) out[i] = h[16 + i];
    return DE_OK;
}

int de_debug_samples(de_ctx* c, uint64_t seed, int sample_index, float* out) {
    if (!c || !out || sample_index < 0) return fail(DE_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    int rc = build_tiles(c, 0, 1);
    if (rc) return rc;
    RenderArgs a;
    rc = fill_render_args(c, &a);
    if (rc) return rc;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.spp_begin = sample_index; a.spp_count = 1; a.spp_stride = 1;
    a.spp_magic = (1ull << 40) + 1ull;
    a.contrib = nullptr;
    a.work_counter = c->d_work_counter + 16 * DE_MAX_SLOTS;     // a counter of its own: launches in the slots keep theirs
    c->launch_variant = c->kernel_variant == 1 ? 1 : 2;         // (the pipeline has no single-sample trace mode: variants 3 and 4 trace with the state machine)
    rc = join_slots(c);
    if (rc) return rc;
    HIP_TRY(launch_render<2>(c, a, c->stream, []() -> hipError_t { return hipSuccess; }));
    HIP_TRY(hipMemcpyAsync(out, c->d_scratch, (size_t)c->W * c->H * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DE_OK;
}

static int debug_math(de_ctx* c, int fn, const float* a, const float* b, float* out, uint64_t n, bool fast) {
    if (!c || !a || !out || fn < 0 || fn > 31) return fail(DE_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes[3] = {n * sizeof(float), b ? n * sizeof(float) : 0, n * sizeof(float)};      // a, b (null without one), out
    const void* const in[3] = {a, b, nullptr};
    return debug_round_trip(c->stream, bytes, in, 2, out, [&](void* const* m) -> hipError_t {
        if (fast) return de_fast_launch_math(fn, (const float*)m[0], (const float*)m[1], (float*)m[2], (size_t)n, c->stream);
        hipLaunchKernelGGL(math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, fn, (const float*)m[0], (const float*)m[1], (float*)m[2], (size_t)n, (const float*)c->d_dens_table);
        return hipSuccess;
    });
}
int de_debug_math(de_ctx* c, int fn, const float* a, const float* b, float* out, uint64_t n) { return debug_math(c, fn, a, b, out, n, false); }
int de_debug_math_fast(de_ctx* c, int fn, const float* a, const float* b, float* out, uint64_t n) { return debug_math(c, fn, a, b, out, n, true); }


/* ---- the denoiser: include/digital_earth_denoise.h */
int de_set_denoise(de_ctx* c, const de_denoise* d) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (!d) { c->dn_on = false; c->dn_out_valid = false; return DE_OK; }
    if (d->struct_bytes != (uint32_t)sizeof(de_denoise)) return fail(DE_ERR_INVALID, "de_denoise.struct_bytes does not match this library's struct");
    if (d->levels < 1 || d->levels > 10 || !(d->sigma_luminance > 0.0f) || !(d->sigma_luminance < 1e30f))
        return fail(DE_ERR_INVALID, "denoiser settings: 1 <= levels <= 10, 0 < sigma_luminance < 1e30");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->dn_on) {
        { int rc = dn_alloc(c); if (rc) return rc; }
        if (c->frame_kind == DE_FRAME_NONE) {
            // no sample yet: S2 starts complete (zeroed on the context stream, ordered before the frame's first accumulate)
            HIP_TRY(c->d_s2.ensure((size_t)c->W * c->H * 3 * sizeof(float)));
            { int rc = join_slots(c); if (rc) return rc; }
            touched_hdr(c);
            HIP_TRY(hipMemsetAsync(c->d_s2, 0, (size_t)c->W * c->H * 3 * sizeof(float), c->stream));
            c->dn_s2_complete = true;
        } else if (c->frame_kind != DE_FRAME_ADAPTIVE) {
            c->dn_s2_complete = false;     // enabled mid-frame: the samples so far have no S2
        }
    }
    c->dn_on = true; c->dn_levels = d->levels; c->dn_sigma_l = d->sigma_luminance;
    c->dn_out_valid = false;
    return DE_OK;
}
int de_get_denoise(de_ctx* c, de_denoise* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    out->struct_bytes = (uint32_t)sizeof(de_denoise);
    out->levels = c->dn_on ? c->dn_levels : 0;
    out->sigma_luminance = c->dn_on ? c->dn_sigma_l : 0.0f;
    return DE_OK;
}
int de_fetch_denoised_hdr(de_ctx* c, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    DisplayArgs d;
    bool per_tile;
    int rc = display_chain(c, STOP_DENOISE, &d, &per_tile);
    if (rc) return rc;
    return fetch_transposed(c, d.hdr, out);
}
int de_fetch_guides(de_ctx* c, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = run_setup(c);
    if (rc) return rc;
    rc = dn_ensure_guides(c);
    if (rc) return rc;
    const size_t npx = (size_t)c->W * c->H;
    std::vector<float4> nc(npx), at(npx);
    std::vector<float> dist(npx);
    HIP_TRY(hipMemcpyAsync(nc.data(), c->d_dn_nc, npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(at.data(), c->d_dn_at, npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(dist.data(), c->d_dn_dist, npx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<float> g(npx * 9);      // the nine guides of a pixel side by side, still [H][W]
    for (size_t p = 0; p < npx; ++p) {
        float* o = &g[p * 9];
        o[0] = nc[p].w; o[1] = dist[p]; o[2] = nc[p].x; o[3] = nc[p].y; o[4] = nc[p].z;
        o[5] = at[p].x; o[6] = at[p].y; o[7] = at[p].z; o[8] = at[p].w;
    }
    to_host_layout(g.data(), out, c->W, c->H, 9);
    return DE_OK;
}
int de_debug_denoise(de_ctx* c, const float* mean, const float* var, const float* guides, int levels, float sigma_l, float* out) {
    if (!c || !mean || !var || !guides || !out || levels < 1 || levels > 10 || !(sigma_l > 0.0f)) return fail(DE_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    int rc = dn_alloc(c);
    if (rc) return rc;
    rc = sync_all(c);
    if (rc) return rc;
    const size_t npx = (size_t)c->W * c->H;
    std::vector<float4> col(npx), nc(npx), at(npx);
    std::vector<float> dist(npx), m3(npx * 3), v1(npx), g9(npx * 9);
    to_device_layout(mean, m3.data(), c->W, c->H, 3);
    to_device_layout(var, v1.data(), c->W, c->H, 1);
    to_device_layout(guides, g9.data(), c->W, c->H, 9);
    for (size_t p = 0; p < npx; ++p) {
        const float* m = &m3[p * 3];
        const float* g = &g9[p * 9];
        col[p] = make_float4(m[0], m[1], m[2], v1[p]);
        nc[p] = make_float4(g[2], g[3], g[4], g[0]);
        at[p] = make_float4(g[5], g[6], g[7], g[8]);
        dist[p] = g[1];
    }
    HIP_TRY(hipMemcpyAsync(c->d_dn_buf[1], col.data(), npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_dn_nc, nc.data(), npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_dn_at, at.data(), npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_dn_dist, dist.data(), npx * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));      // the host vectors are reused below
    c->dn_guides_valid = false; c->dn_out_valid = false;      // the context's guides were overwritten
    float4* res = nullptr;
    rc = dn_levels(c, levels, sigma_l, &res);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(col.data(), res, npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    to_host_layout(reinterpret_cast<const float*>(col.data()), out, c->W, c->H, 4);
    return DE_OK;
}

/* ---- auto-exposure: include/digital_earth_exposure.h */
int de_set_auto_exposure(de_ctx* c, const de_auto_exposure* s) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (!s) { c->ae_on = false; c->ae_displayed = false; return DE_OK; }
    if (s->struct_bytes != (uint32_t)sizeof(de_auto_exposure)) return fail(DE_ERR_INVALID, "de_auto_exposure.struct_bytes does not match this library's struct");
    if (!(s->key > 0.0f) || !(s->key < 1e30f) || !(fabsf(s->compensation) < 1e30f) || !(fabsf(s->ev_min) < 1e30f) || !(fabsf(s->ev_max) < 1e30f) || !(s->ev_min <= s->ev_max))
        return fail(DE_ERR_INVALID, "auto-exposure settings: 0 < key, finite compensation, finite ev_min <= ev_max");
    if (!(s->low_fraction >= 0.0f) || !(s->low_fraction < s->high_fraction) || !(s->high_fraction <= 1.0f) || !(s->low_fraction < 1.0f))
        return fail(DE_ERR_INVALID, "auto-exposure settings: 0 <= low_fraction < high_fraction <= 1");
    if (!(s->adapt > 0.0f) || !(s->adapt <= 1.0f)) return fail(DE_ERR_INVALID, "auto-exposure settings: 0 < adapt <= 1");
    const int32_t* r = s->region;
    if ((r[0] | r[1] | r[2] | r[3]) != 0 && (r[0] < 0 || r[1] < 0 || r[2] > c->W || r[3] > c->H || r[0] >= r[2] || r[1] >= r[3]))
        return fail(DE_ERR_INVALID, "auto-exposure region: 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height (all 0 = the whole image)");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = ae_alloc(c); if (rc) return rc; }
    // every call clears the adaptation state, ordered on the context stream behind the displays already enqueued
    HIP_TRY(hipMemsetAsync(c->d_ae_state, 0, sizeof(MeterState), c->stream));
    c->ae = *s;
    c->ae_on = true; c->ae_displayed = false;
    return DE_OK;
}
int de_get_auto_exposure(de_ctx* c, de_auto_exposure* out) { return get_settings(c, &de_ctx::ae_on, &de_ctx::ae, out); }
int de_get_metering(de_ctx* c, de_metering* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (out->struct_bytes != (uint32_t)sizeof(de_metering)) return fail(DE_ERR_INVALID, "de_metering.struct_bytes does not match this library's struct");
    if (!c->ae_on) return fail(DE_ERR_STATE, "auto-exposure is off (de_set_auto_exposure)");
    if (!c->ae_displayed) return fail(DE_ERR_STATE, "nothing has been displayed since auto-exposure was turned on");
    HIP_TRY(hipSetDevice(c->device));
    MeterResult r;
    HIP_TRY(hipMemcpyAsync(&r, c->d_ae_result, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out->ev = r.ev; out->ev_target = r.target; out->mean_log2 = r.mean; out->valid = r.valid;
    out->metered = r.n; out->below = r.below; out->clipped = r.clipped;
    memcpy(out->histogram, r.h, sizeof(out->histogram));
    return DE_OK;
}

/* ---- bloom: include/digital_earth_bloom.h */
int de_set_bloom(de_ctx* c, const de_bloom* s) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (!s) { c->bl_on = false; return DE_OK; }
    if (s->struct_bytes != (uint32_t)sizeof(de_bloom)) return fail(DE_ERR_INVALID, "de_bloom.struct_bytes does not match this library's struct");
    if (!(s->intensity >= 0.0f) || !(s->intensity <= 1.0f) || !(s->knee >= 0.0f) || !(s->knee <= 1.0f) || !(s->spread >= 0.0f) || !(s->spread <= 1.0f))
        return fail(DE_ERR_INVALID, "bloom settings: intensity, knee and spread in [0, 1]");
    if (!(s->threshold >= 0.0f) || !(s->threshold < 1e30f) || !(s->clamp >= 0.0f) || !(s->clamp < 1e30f))
        return fail(DE_ERR_INVALID, "bloom settings: finite threshold >= 0, finite clamp >= 0 (0 = none)");
    if (s->levels < 1 || s->levels > BL_MAX_LEVELS) return fail(DE_ERR_INVALID, "bloom settings: levels in 1 .. 10");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = bl_alloc(c); if (rc) return rc; }
    c->bl = *s;
    c->bl_on = true;
    return DE_OK;
}
int de_get_bloom(de_ctx* c, de_bloom* out) { return get_settings(c, &de_ctx::bl_on, &de_ctx::bl, out); }
int de_fetch_bloom_hdr(de_ctx* c, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    DisplayArgs d;
    bool per_tile;
    int rc = display_chain(c, STOP_BLOOM, &d, &per_tile);
    if (rc) return rc;
    return fetch_transposed(c, d.hdr, out);
}

/* ---- history reprojection: include/digital_earth_history.h */
int de_set_history(de_ctx* c, const de_history* s) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (!s) { c->hs_on = false; hs_drop(c); return DE_OK; }
    if (s->struct_bytes != (uint32_t)sizeof(de_history)) return fail(DE_ERR_INVALID, "de_history.struct_bytes does not match this library's struct");
    if (!(s->max_history > 0.0f) || !(s->max_history < 1e30f) || !(s->depth_tolerance > 0.0f) || !(s->depth_tolerance <= 1.0f))
        return fail(DE_ERR_INVALID, "history settings: 0 < max_history < 1e30, 0 < depth_tolerance <= 1");
    HIP_TRY(hipSetDevice(c->device));
    { int rc = hs_alloc(c); if (rc) return rc; }
    c->hs = *s;
    c->hs_on = true;
    hs_drop(c);      // every call drops the history
    return DE_OK;
}
int de_get_history(de_ctx* c, de_history* out) { return get_settings(c, &de_ctx::hs_on, &de_ctx::hs, out); }
int de_fetch_history_hdr(de_ctx* c, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    DisplayArgs d;
    bool per_tile;
    int rc = display_chain(c, STOP_HISTORY, &d, &per_tile);
    if (rc) return rc;
    // the candidate the blend just wrote: the mean the display reads and its weight in samples
    const size_t npx = (size_t)c->W * c->H;
    std::vector<float4> px(npx);
    HIP_TRY(hipMemcpyAsync(px.data(), c->d_hs_c[c->hs_cur ^ 1], npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    to_host_layout(reinterpret_cast<const float*>(px.data()), out, c->W, c->H, 4);
    return frame_status(c);
}
/* include/digital_earth_debug.h: the blend on host-given arrays.  Buffers of its own; the context's history is not touched. */
int de_debug_history(de_ctx* c, const float* mean, const int32_t* n, const float* dist, const de_params* cur, const float* hist_c, const float* hist_d,
                     const de_params* hist, float max_history, float depth_tolerance, float* out) {
    if (!c || !mean || !n || !dist || !cur || !out || (hist_c && (!hist_d || !hist)) || !(max_history > 0.0f) || !(depth_tolerance > 0.0f) || !(depth_tolerance <= 1.0f))
        return fail(DE_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * H;
    Dev<void> own[10];
    void* b[10] = {};
    const size_t bytes[10] = {npx * 3 * sizeof(float), npx * sizeof(int32_t), npx * sizeof(float), npx * sizeof(float4), npx * sizeof(float),
                              sizeof(FrameConsts), 2 * sizeof(HistoryCam), npx * 3 * sizeof(float), npx * sizeof(float4), npx * sizeof(float)};
    for (int k = 0; k < 10; ++k) { HIP_TRY(own[k].ensure(bytes[k])); b[k] = own[k]; }
    std::vector<float> m(npx * 3), t(npx), hd(npx);
    std::vector<int32_t> nn(npx);
    std::vector<float4> hcol(npx);
    to_device_layout(mean, m.data(), W, H, 3);
    to_device_layout(n, nn.data(), W, H, 1);
    to_device_layout(dist, t.data(), W, H, 1);
    if (hist_c) {
        to_device_layout(hist_c, reinterpret_cast<float*>(hcol.data()), W, H, 4);
        to_device_layout(hist_d, hd.data(), W, H, 1);
    }
    HIP_TRY(hipMemcpyAsync(b[0], m.data(), bytes[0], hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b[1], nn.data(), bytes[1], hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b[2], t.data(), bytes[2], hipMemcpyHostToDevice, c->stream));
    if (hist_c) {
        HIP_TRY(hipMemcpyAsync(b[3], hcol.data(), bytes[3], hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(b[4], hd.data(), bytes[4], hipMemcpyHostToDevice, c->stream));
    }
    HistoryCam* cams = (HistoryCam*)b[6];
    hipLaunchKernelGGL(history_camera_kernel, dim3(1), dim3(1), 0, c->stream, *cur, W, H, (FrameConsts*)b[5], (HistoryCam*)nullptr);
    HIP_TRY(hipGetLastError());
    if (hist_c) {
        hipLaunchKernelGGL(history_camera_kernel, dim3(1), dim3(1), 0, c->stream, *hist, W, H, (FrameConsts*)nullptr, cams);
        HIP_TRY(hipGetLastError());
    }
    HistoryArgs a;
    a.s.hdr = (const float*)b[0]; a.s.tile_spp = nullptr; a.s.samples = 1; a.s.W = W; a.s.H = H;
    a.n_tile = nullptr; a.n_pixel = (const int32_t*)b[1]; a.n_frame = 0;
    a.dist = (const float*)b[2]; a.fc = (const FrameConsts*)b[5];
    a.hist_c = hist_c ? (const float4*)b[3] : nullptr; a.hist_d = (const float*)b[4]; a.hist_cam = cams;
    a.out = (float*)b[7]; a.cand_c = (float4*)b[8]; a.cand_d = (float*)b[9]; a.cand_cam = cams + 1;
    a.max_history = max_history; a.depth_tolerance = depth_tolerance;
    hipLaunchKernelGGL(history_blend_kernel, dn_grid(c), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hcol.data(), b[8], bytes[8], hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(m.data(), b[7], bytes[7], hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t p = 0; p < npx; ++p) {
        const float4 v = hcol[p];
        // the mean the display would read and the candidate's colour are the same three stores
        if (memcmp(&m[p * 3], &v.x, sizeof(float)) != 0 || memcmp(&m[p * 3 + 1], &v.y, sizeof(float)) != 0 || memcmp(&m[p * 3 + 2], &v.z, sizeof(float)) != 0)
            return fail(DE_ERR_HIP, "history_blend_kernel: the display's mean and the candidate differ");
    }
    to_host_layout(reinterpret_cast<const float*>(hcol.data()), out, W, H, 4);
    return DE_OK;
}

/* ---- local exposure: include/digital_earth_local_exposure.h */
int de_set_local_exposure(de_ctx* c, const de_local_exposure* s) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (!s) { c->lx_on = false; return DE_OK; }
    if (s->struct_bytes != (uint32_t)sizeof(de_local_exposure)) return fail(DE_ERR_INVALID, "de_local_exposure.struct_bytes does not match this library's struct");
    if (!s->on) { c->lx_on = false; return DE_OK; }
    { int rc = lx_settings_check(s); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    { int rc = lx_alloc(c); if (rc) return rc; }
    c->lx = *s;
    c->lx.on = 1;
    c->lx_on = true;
    return DE_OK;
}
int de_get_local_exposure(de_ctx* c, de_local_exposure* out) { return get_settings(c, &de_ctx::lx_on, &de_ctx::lx, out); }
int de_fetch_local_exposure_hdr(de_ctx* c, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    DisplayArgs d;
    bool per_tile;
    int rc = display_chain(c, STOP_LOCAL_EXPOSURE, &d, &per_tile);
    if (rc) return rc;
    return fetch_transposed(c, d.hdr, out);
}
/* The stage once on a host-given mean.  A source and a FrameConsts of its own; the pyramid and the output are the context's (nothing between displays
 * lives in them). */
int de_debug_local_exposure(de_ctx* c, const float* mean, float exposure_scale, const de_local_exposure* s, float* out) {
    if (!c || !mean || !s || !out) return fail(DE_ERR_INVALID, "null argument");
    { int rc = lx_settings_check(s); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    { int rc = lx_alloc(c); if (rc) return rc; }
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * H;
    Dev<float> d_mean;
    Dev<FrameConsts> d_fc;
    HIP_TRY(d_mean.ensure(npx * 3 * sizeof(float)));
    HIP_TRY(d_fc.ensure(sizeof(FrameConsts)));
    std::vector<float> m(npx * 3);
    to_device_layout(mean, m.data(), W, H, 3);
    FrameConsts fc;
    memset(&fc, 0, sizeof(fc));
    fc.exposure_scale = exposure_scale;      // the only field the stage reads
    HIP_TRY(hipMemcpyAsync(d_mean, m.data(), npx * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_fc, &fc, sizeof(fc), hipMemcpyHostToDevice, c->stream));
    DisplayArgs d;
    memset(&d, 0, sizeof(d));
    d.fc = d_fc; d.hdr = d_mean; d.W = W; d.H = H; d.samples = 1;
    bool per_tile = false;
    int rc = lx_run(c, *s, d, per_tile);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(m.data(), c->d_lx_out, npx * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    to_host_layout(m.data(), out, W, H, 3);
    return DE_OK;
}

/* ---- 8-bit pixel output: include/digital_earth_pixels.h (pixels_kernels.hip) */
int de_set_pixels(de_ctx* c, const de_pixels* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = px_settings_check(s); if (rc) return rc; }
    { int rc = refuse_in_flight(c->px_ring); if (rc) return rc; }
    c->px = *s;
    packed_reset(c->px_out);
    return DE_OK;
}
int de_get_pixels(de_ctx* c, de_pixels* out, uint32_t* last_phase) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->px;
    if (last_phase) *last_phase = c->px_out.last_phase;
    return DE_OK;
}
int de_render_to_pixels(de_ctx* c, const uint8_t** device_pixels) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    int rc = render_packed(c, c->px_out, px_capacity(c), c->px.animate != 0, [c](uint32_t phase) {
        px_launch(c->stream, shown_image(c), c->px_out.dev, out_w(c), out_h(c), c->px, phase);
    });
    if (rc) return rc;
    if (device_pixels) *device_pixels = c->px_out.dev;
    return DE_OK;
}
int de_fetch_pixels_view(de_ctx* c, const uint8_t** host) {
    if (!c || !host) return fail(DE_ERR_INVALID, "null argument");
    return fetch_staged(c, c->px_out.stage, c->px_out.noun, de_render_to_pixels, px_capacity(c), px_size(c), host);
}
int de_fetch_pixels(de_ctx* c, uint8_t* out, uint64_t out_bytes) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (out_bytes < (uint64_t)px_size(c)) return fail(DE_ERR_INVALID, "out_bytes is smaller than W * H * channels");
    const uint8_t* host = nullptr;
    int rc = de_fetch_pixels_view(c, &host);
    if (rc) return rc;
    memcpy(out, host, px_size(c));
    return DE_OK;
}
int de_fetch_pixels_begin(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    return ring_begin(c, c->px_ring, de_render_to_pixels, px_capacity(c), px_size(c));
}
int de_fetch_pixels_end(de_ctx* c, const uint8_t** host) {
    if (!c || !host) return fail(DE_ERR_INVALID, "null argument");
    return ring_end(c, c->px_ring, host);
}
/* include/digital_earth_debug.h: the conversion once on a host-given image.  Buffers of its own; the context's pixels and phase counter are not touched. */
int de_debug_pixels(de_ctx* c, const float* image, int W, int H, const de_pixels* s, uint32_t phase, uint8_t* out) {
    if (!c || !image || !s || !out || W <= 0 || H <= 0 || (W % 16) != 0 || (H % 8) != 0 || (long long)W * H > (1ll << 28))
        return fail(DE_ERR_INVALID, "bad arguments (W a multiple of 16, H a multiple of 8, as de_create asks)");
    { int rc = px_settings_check(s); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes[2] = {(size_t)W * H * 3 * sizeof(float), (size_t)W * H * (size_t)s->channels};
    const void* const in[2] = {image, nullptr};
    return debug_round_trip(c->stream, bytes, in, 1, out, [&](void* const* b) { px_launch(c->stream, (const float*)b[0], (uint8_t*)b[1], W, H, *s, phase); return hipSuccess; });
}

/* ---- output scaling: include/digital_earth_output_scale.h (output_scale_kernels.hip) */
int de_set_output_scale(de_ctx* c, const de_output_scale* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    int ow = 0, oh = 0;
    { int rc = os_settings_check(s, c->W, c->H, &ow, &oh); if (rc) return rc; }
    if (s->enabled && c->pano.on) return fail(DE_ERR_STATE, "the panorama is on (de_set_panorama): it makes the shown image, and a context has one");
    for (const FetchRing* r : {&c->img, &c->px_ring, &c->vd_ring, &c->jp_coded.ring, &c->pn_coded.ring}) { int rc = refuse_in_flight(*r); if (rc) return rc; }
    c->os = *s;
    c->os.enabled = s->enabled ? 1 : 0; c->os.width = ow; c->os.height = oh;
    return DE_OK;
}
int de_get_output_scale(de_ctx* c, de_output_scale* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->os;
    if (out->width == 0 && out->height == 0) { out->width = c->W; out->height = c->H; }
    return DE_OK;
}
int de_output_size(de_ctx* c, int* width, int* height) {
    if (!c || !width || !height) return fail(DE_ERR_INVALID, "null argument");
    *width = out_w(c); *height = out_h(c);
    return DE_OK;
}
/* ---- the panorama output: include/digital_earth_panorama.h (panorama_kernels.hip, panorama_body.h) */
int de_set_panorama(de_ctx* c, const de_panorama* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    if (c->W != c->H) return fail(DE_ERR_INVALID, "a panorama's face camera is square: the context needs W == H");
    { int rc = pano_settings_check(s, c->W); if (rc) return rc; }
    if (s->on && c->os.enabled) return fail(DE_ERR_STATE, "output scaling is on (de_set_output_scale): it makes the shown image, and a context has one");
    for (const FetchRing* r : {&c->img, &c->px_ring, &c->vd_ring}) { int rc = refuse_in_flight(*r); if (rc) return rc; }
    // an EXR or RGBE fetch of the scene-linear panorama reads the linear slots and the tables (include/digital_earth_environment.h); one of the pinhole frame reads nothing of this stage
    for (const CodedOut* o : {&c->jp_coded, &c->pn_coded, &c->ex_coded, &c->rg_coded}) { int rc = refuse_panorama_readers(*o); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    { int rc = c->pano_faces.ensure((size_t)DE_PANO_FACES * (size_t)c->W * (size_t)c->W * 3 * sizeof(float), "the panorama's buffers"); if (rc) return rc; }
    { int rc = c->pano_out.ensure((size_t)s->width * (size_t)s->height * 3 * sizeof(float), "the panorama's buffers"); if (rc) return rc; }
    c->pano = *s;
    c->pano.on = s->on ? 1 : 0;
    c->pano_mask = 0u; c->env_mask = 0u;
    pano_make_consts(c->pano, c->W, &c->pano_consts);
    return DE_OK;
}
int de_get_panorama(de_ctx* c, de_panorama* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->pano;
    return DE_OK;
}
int de_panorama_face_camera(de_ctx* c, int face, const float* pos, float* look_at, float* up, float* fov) {
    if (!c || !pos || !look_at || !up || !fov) return fail(DE_ERR_INVALID, "null argument");
    if (face < 0 || face >= DE_PANO_FACES) return fail(DE_ERR_INVALID, "face must lie in 0 ... 5");
    if (c->W != c->H) return fail(DE_ERR_INVALID, "a panorama's face camera is square: the context needs W == H");
    double look[3], u[3];
    pano_face_frame(c->pano.basis, face, look, u);
    const double len = sqrt((double)pos[0] * pos[0] + (double)pos[1] * pos[1] + (double)pos[2] * pos[2]), L = len > 1.0 ? len : 1.0;
    for (int k = 0; k < 3; ++k) { look_at[k] = (float)((double)pos[k] + L * look[k]); up[k] = (float)u[k]; }
    *fov = (float)((double)c->W / (double)(c->W - 2 * c->pano.apron));
    return DE_OK;
}
int de_panorama_capture(de_ctx* c, int face) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (face < 0 || face >= DE_PANO_FACES) return fail(DE_ERR_INVALID, "face must lie in 0 ... 5");
    if (!c->pano.on) return fail(DE_ERR_STATE, "the panorama is off (de_set_panorama)");
    // what would print the face's border into the picture: a seam along every cube edge
    if (c->p.vignette_strength != 0.0f) return fail(DE_ERR_STATE, "a panorama face cannot be captured with a vignette (vignette_strength != 0): it darkens every face's border");
    if (c->ae_on) return fail(DE_ERR_STATE, "a panorama face cannot be captured under auto-exposure: every face would be metered on its own");
    if (c->bl_on) return fail(DE_ERR_STATE, "a panorama face cannot be captured under bloom: the glare ends at the face's border");
    if (c->lx_on) return fail(DE_ERR_STATE, "a panorama face cannot be captured under local exposure: its pyramid ends at the face's border");
    if (c->hs_on) return fail(DE_ERR_STATE, "a panorama face cannot be captured under history reprojection: the history belongs to another face's camera");
    return render_to_image_or_slot(c, nullptr, face);
}
int de_panorama_captured(de_ctx* c, uint32_t* mask) {
    if (!c || !mask) return fail(DE_ERR_INVALID, "null argument");
    *mask = c->pano_mask;
    return DE_OK;
}
/* include/digital_earth_debug.h: the kernel once on host-given faces.  Buffers and tables of its own; the context's setting and slots are not touched.
 * The arguments and the settings are checked before the context is read. */
int de_debug_panorama(de_ctx* c, const float* faces, int n, const de_panorama* s, float* out) {
    if (!c || !faces || !s || !out || n < 4 || n > 16384) return fail(DE_ERR_INVALID, "bad arguments (faces of 4 ... 16384 pixels a side)");
    { int rc = pano_settings_check(s, n); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    Dev<float> d_faces, d_out;
    de_ctx::PanoTab tab;
    PanoArgs k = {};
    pano_make_consts(*s, n, &k);
    const size_t in_bytes = (size_t)DE_PANO_FACES * (size_t)n * (size_t)n * 3 * sizeof(float), out_bytes = (size_t)s->width * (size_t)s->height * 3 * sizeof(float);
    HIP_TRY(d_faces.ensure(in_bytes));
    HIP_TRY(d_out.ensure(out_bytes));
    if (s->projection == DE_PANO_EQUIRECT) { int rc = pano_tables_ensure(c->stream, tab, s->width, s->height, s->supersample); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(d_faces, faces, in_bytes, hipMemcpyHostToDevice, c->stream));
    int rc = pano_launch(c->stream, *s, k, n, d_faces, tab, d_out);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DE_OK;
}

/* ---- the scene-linear panorama: include/digital_earth_environment.h (environment_kernels.hip, environment_body.h) */
int de_environment_capture(de_ctx* c, int face) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (face < 0 || face >= DE_PANO_FACES) return fail(DE_ERR_INVALID, "face must lie in 0 ... 5");
    if (!c->pano.on) return fail(DE_ERR_STATE, "the panorama is off (de_set_panorama)");
    const int source = c->ex.source;
    // what would print the face's border or another face's camera into the environment; a vignette and auto-exposure live behind the display and do not
    if (source == DE_EXR_SOURCE_HISTORY) return fail(DE_ERR_STATE, "a linear panorama face cannot be captured from the history (de_exr.source): the history belongs to another face's camera");
    if (source == DE_EXR_SOURCE_BLOOM) return fail(DE_ERR_STATE, "a linear panorama face cannot be captured from the bloom (de_exr.source): its pyramid ends at the face's border");
    if (source == DE_EXR_SOURCE_LOCAL_EXPOSURE) return fail(DE_ERR_STATE, "a linear panorama face cannot be captured from local exposure (de_exr.source): its pyramid ends at the face's border");
    if (source != DE_EXR_SOURCE_MEAN) { int rc = display_chain_refusal(c, linear_stop_of[source]); if (rc) return rc; }      // ahead of every allocation: a refused call changes nothing
    HIP_TRY(hipSetDevice(c->device));
    { int rc = c->env_faces.ensure((size_t)DE_PANO_FACES * env_face_floats(c) * sizeof(float), "the environment's buffers"); if (rc) return rc; }
    DisplayArgs d;
    bool per_tile;
    int rc = linear_source(c, source, &d, &per_tile);
    if (rc) return rc;
    rc = env_capture_launch(c->stream, display_src(d, per_tile), c->env_faces + (size_t)face * env_face_floats(c));
    if (rc) return rc;
    rc = linear_sums_read(c);      // behind the capture: it has read the sums
    if (rc) return rc;
    c->env_mask |= 1u << face;
    return DE_OK;
}
int de_environment_captured(de_ctx* c, uint32_t* mask) {
    if (!c || !mask) return fail(DE_ERR_INVALID, "null argument");
    *mask = c->env_mask;
    return DE_OK;
}
int de_fetch_environment_face(de_ctx* c, int face, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (face < 0 || face >= DE_PANO_FACES) return fail(DE_ERR_INVALID, "face must lie in 0 ... 5");
    if (!(c->env_mask >> face & 1u)) return fail(DE_ERR_STATE, "that linear face is not held (de_environment_capture)");
    HIP_TRY(hipSetDevice(c->device));
    return copy_out(c, out, c->env_faces + (size_t)face * env_face_floats(c), env_face_floats(c) * sizeof(float));
}
/* The resampling and the conversion once on host-given linear faces.  Buffers and tables of its own; the context's settings and slots are not touched.
 * The arguments and both settings are checked before the context is read. */
int de_debug_environment_exr(de_ctx* c, const float* faces, int n, const de_panorama* p, const de_exr* s, void* out, uint64_t out_bytes, uint64_t* len) {
    if (!c || !faces || !p || !s || !out || !len || n < 4 || n > 16384) return fail(DE_ERR_INVALID, "bad arguments (faces of 4 ... 16384 pixels a side)");
    { int rc = pano_settings_check(p, n); if (rc) return rc; }
    { int rc = ex_settings_check(s); if (rc) return rc; }
    { int rc = ex_shape_check(p->width, p->height, s->pixel_type); if (rc) return rc; }
    const ExrGeometry g = ex_geometry(p->width, p->height, *s);
    EnvDebug env;
    de_ctx::ExrWork work;
    return coded_debug(c, g.capacity, ex_length, out, out_bytes, len, "out_bytes is smaller than the file (*len)", [&](hipStream_t stream, uint8_t* d_out) -> int {
        DisplaySrc src;
        int rc = ex_work_ensure(work, g);
        if (!rc) rc = env_debug_source(stream, env, faces, n, *p, &src);
        if (rc) return rc;
        HIP_TRY(ex_tables_upload(stream, work));
        return ex_launch(stream, work, g, src, true, s->scale, d_out, no_hook);
    });
}

/* include/digital_earth_debug.h: the stage once on a host-given image.  Buffers and tables of its own; the context's setting is not touched. */
int de_debug_output_scale(de_ctx* c, const float* image, int W, int H, const de_output_scale* s, float* out) {
    if (!c || !image || !s || !out || W <= 0 || H <= 0 || (W % 16) != 0 || (H % 8) != 0 || (long long)W * H > (1ll << 28))
        return fail(DE_ERR_INVALID, "bad arguments (W a multiple of 16, H a multiple of 8, as de_create asks)");
    int ow = 0, oh = 0;
    { int rc = os_settings_check(s, W, H, &ow, &oh); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    Dev<float> d_in, d_mid, d_out;
    de_ctx::ScaleDev t[2];          // and the two axes' tables
    const size_t in_bytes = (size_t)W * H * 3 * sizeof(float), mid_bytes = (size_t)W * oh * 3 * sizeof(float), out_bytes = (size_t)ow * oh * 3 * sizeof(float);
    HIP_TRY(d_in.ensure(in_bytes));
    HIP_TRY(d_mid.ensure(mid_bytes));
    HIP_TRY(d_out.ensure(out_bytes));
    int rc = DE_OK;
    if (oh != H) { rc = os_table_ensure(c->stream, t[0], H, oh, s->filter); if (rc) return rc; }
    if (ow != W) { rc = os_table_ensure(c->stream, t[1], W, ow, s->filter); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(d_in, image, in_bytes, hipMemcpyHostToDevice, c->stream));
    const float* result = d_in;      // both axes copies: the identity, nothing runs
    if (ow != W || oh != H) {
        rc = os_launch(c->stream, d_in, W, H, ow, oh, t[0], t[1], d_mid, d_out);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        result = d_out;
    }
    HIP_TRY(hipMemcpyAsync(out, result, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DE_OK;
}
int de_debug_output_scale_weights(de_ctx* c, int n_src, int n_dst, int filter, int32_t* first, float* weights, int* taps) {
    if (!c || !taps) return fail(DE_ERR_INVALID, "null argument");
    ScaleTable T;
    if (!os_build_table(n_src, n_dst, filter, &T)) return fail(DE_ERR_INVALID, "de_debug_output_scale_weights: sizes must be positive with n_dst / n_src in [1/8, 8], the filter DE_SCALE_*");
    *taps = T.taps;
    if (first) memcpy(first, T.first.data(), T.first.size() * sizeof(int32_t));
    if (weights)
        for (int j = 0; j < n_dst; ++j)
            for (int t = 0; t < T.taps; ++t) weights[(size_t)j * (size_t)T.taps + (size_t)t] = T.w[(size_t)t * (size_t)n_dst + (size_t)j];      // the kernels' [tap][j], transposed
    return DE_OK;
}

/* ---- HDR display output: include/digital_earth_hdr_output.h (hdr_output_kernels.hip) */

int de_set_hdr_output(de_ctx* c, const de_hdr_output* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = ho_settings_check(s); if (rc) return rc; }
    c->ho = *s;
    c->ho.on = s->on ? 1 : 0;
    hdr_output_consts((double)s->peak_nits, s->gamut, s->transfer, &c->ho_consts);
    packed_reset(c->hpx_out);
    return DE_OK;
}
int de_get_hdr_output(de_ctx* c, de_hdr_output* out, uint32_t* last_phase) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->ho;
    if (last_phase) *last_phase = c->hpx_out.last_phase;
    return DE_OK;
}
int de_render_to_hdr_pixels(de_ctx* c, const void** device_pixels) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (!c->ho.on) return fail(DE_ERR_STATE, "the HDR display output is off: de_set_hdr_output first");
    int rc = render_packed(c, c->hpx_out, hpx_capacity(c), c->ho.animate != 0, [c](uint32_t phase) {
        hpx_launch(c->stream, shown_image(c), c->hpx_out.dev, out_w(c), out_h(c), c->ho, phase);
    });
    if (rc) return rc;
    if (device_pixels) *device_pixels = c->hpx_out.dev;
    return DE_OK;
}
int de_fetch_hdr_pixels(de_ctx* c, void* out, uint64_t out_bytes) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (!c->ho.on) return fail(DE_ERR_STATE, "the HDR display output is off: de_set_hdr_output first");
    if (out_bytes < (uint64_t)hpx_size(c)) return fail(DE_ERR_INVALID, "out_bytes is smaller than width * height * 4 (RGB10A2) or * 6 (RGB16)");
    const void* host = nullptr;
    int rc = fetch_staged(c, c->hpx_out.stage, c->hpx_out.noun, de_render_to_hdr_pixels, hpx_capacity(c), hpx_size(c), &host);
    if (rc) return rc;
    memcpy(out, host, hpx_size(c));
    return DE_OK;
}
/* ---- video frame output: include/digital_earth_video.h (videoframe_kernels.hip) */
int de_set_video(de_ctx* c, const de_video* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = vd_settings_check(s); if (rc) return rc; }
    { int rc = refuse_in_flight(c->vd_ring); if (rc) return rc; }
    c->vd = *s;
    c->vd.animate = s->animate ? 1 : 0;
    c->vd_consts = vd_make_consts(s->format, s->matrix, s->range);
    packed_reset(c->vd_out);
    return DE_OK;
}
int de_get_video(de_ctx* c, de_video* out, uint32_t* last_phase) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->vd;
    if (last_phase) *last_phase = c->vd_out.last_phase;
    return DE_OK;
}
int de_videoframe_bytes(de_ctx* c, uint64_t* bytes, uint64_t* plane_offsets, uint64_t* plane_strides) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    { int rc = vd_even_check(c); if (rc) return rc; }
    const uint64_t W = (uint64_t)out_w(c), H = (uint64_t)out_h(c), B = (uint64_t)vd_sample_bytes(c->vd);
    const bool interleaved = c->vd.format == DE_VIDEO_NV12 || c->vd.format == DE_VIDEO_P010;
    if (bytes) *bytes = (uint64_t)vd_size(c);
    if (plane_offsets) { plane_offsets[0] = 0; plane_offsets[1] = W * H * B; plane_offsets[2] = interleaved ? W * H * B + B : (W * H + (W / 2) * (H / 2)) * B; }
    if (plane_strides) { plane_strides[0] = W * B; plane_strides[1] = plane_strides[2] = (interleaved ? W : W / 2) * B; }
    return DE_OK;
}
int de_render_to_video(de_ctx* c, const void** device_frame) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    { int rc = vd_even_check(c); if (rc) return rc; }
    int rc = render_packed(c, c->vd_out, vd_capacity(c), c->vd.animate != 0, [c](uint32_t phase) {
        vd_launch(c->stream, shown_image(c), c->vd_out.dev, out_w(c), out_h(c), c->vd, c->vd_consts, phase);
    });
    if (rc) return rc;
    if (device_frame) *device_frame = c->vd_out.dev;
    return DE_OK;
}
int de_fetch_videoframe_view(de_ctx* c, const void** host) {
    if (!c || !host) return fail(DE_ERR_INVALID, "null argument");
    { int rc = vd_even_check(c); if (rc) return rc; }
    return fetch_staged(c, c->vd_out.stage, c->vd_out.noun, de_render_to_video, vd_capacity(c), vd_size(c), host);
}
int de_fetch_video(de_ctx* c, void* out, uint64_t out_bytes) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    { int rc = vd_even_check(c); if (rc) return rc; }
    if (out_bytes < (uint64_t)vd_size(c)) return fail(DE_ERR_INVALID, "out_bytes is smaller than the frame (de_videoframe_bytes)");
    const void* host = nullptr;
    int rc = de_fetch_videoframe_view(c, &host);
    if (rc) return rc;
    memcpy(out, host, vd_size(c));
    return DE_OK;
}
int de_fetch_videoframe_begin(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    { int rc = vd_even_check(c); if (rc) return rc; }
    return ring_begin(c, c->vd_ring, de_render_to_video, vd_capacity(c), vd_size(c));
}
int de_fetch_videoframe_end(de_ctx* c, const void** host) {
    if (!c || !host) return fail(DE_ERR_INVALID, "null argument");
    return ring_end(c, c->vd_ring, host);
}
/* the conversion once on a host-given image of any even size.  Buffers of its own; the context's frame and phase counter are not touched. */
int de_debug_video(de_ctx* c, const float* image, int W, int H, const de_video* s, uint32_t phase, void* out) {
    if (!c || !image || !s || !out || W <= 0 || H <= 0 || (W & 1) || (H & 1) || (long long)W * H > (1ll << 28))
        return fail(DE_ERR_INVALID, "bad arguments (W and H positive and even, W * H at most 2^28)");
    { int rc = vd_settings_check(s); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes[2] = {(size_t)W * H * 3 * sizeof(float), vd_frame_bytes(W, H, *s)};
    const void* const in[2] = {image, nullptr};
    return debug_round_trip(c->stream, bytes, in, 1, out, [&](void* const* b) { vd_launch(c->stream, (const float*)b[0], (uint8_t*)b[1], W, H, *s, vd_make_consts(s->format, s->matrix, s->range), phase); return hipSuccess; });
}

/* ---- JPEG output: include/digital_earth_jpeg.h (jpeg_kernels.hip, jpeg_tables.h) */
int de_set_jpeg(de_ctx* c, const de_jpeg* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = jp_settings_check(s); if (rc) return rc; }
    { int rc = refuse_in_flight(c->jp_coded.ring); if (rc) return rc; }
    c->jp = *s;
    jp_make_tables(s->quality, &c->jp_tab);
    c->jp_gen++; c->jp_tab_gen = c->jp_gen;
    c->jp_w = out_w(c); c->jp_h = out_h(c);
    jp_write_framing(c->jp_tab, c->jp_w, c->jp_h, s->restart_mcus, c->jp_framing);
    packed_reset(c->jp_coded.out);
    return DE_OK;
}
int de_get_jpeg(de_ctx* c, de_jpeg* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->jp;
    return DE_OK;
}
int de_jpeg_capacity(de_ctx* c, uint64_t* bytes) { return coded_capacity<JpegOut>(c, bytes); }
int de_render_to_jpeg(de_ctx* c, const void** device_stream, const uint64_t** device_len) { return coded_render_to<JpegOut>(c, device_stream, device_len); }
int de_fetch_jpeg_view(de_ctx* c, const void** host, uint64_t* len) { return coded_fetch_view<JpegOut>(c, host, len); }
int de_fetch_jpeg(de_ctx* c, void* out, uint64_t out_bytes, uint64_t* len) { return coded_fetch<JpegOut>(c, out, out_bytes, len); }
int de_fetch_jpeg_begin(de_ctx* c) { return coded_fetch_begin<JpegOut>(c); }
int de_fetch_jpeg_end(de_ctx* c, const void** host, uint64_t* len) { return coded_fetch_end<JpegOut>(c, host, len); }
/* the conversion once on a host-given image of any even size.  Buffers of its own; the context's settings and streams are not touched. */
int de_debug_jpeg(de_ctx* c, const float* image, int W, int H, const de_jpeg* s, void* out, uint64_t out_bytes, uint64_t* len) {
    if (!c || !image || !s || !out || !len || W <= 0 || H <= 0 || (W & 1) || (H & 1) || (long long)W * H > (1ll << 24))
        return fail(DE_ERR_INVALID, "bad arguments (W and H positive and even, W * H at most 2^24)");
    { int rc = jp_settings_check(s); if (rc) return rc; }
    const JpegGeometry g = jp_geometry(W, H, s->restart_mcus);
    { int rc = jp_geometry_check(g); if (rc) return rc; }
    JpegTables tab;
    jp_make_tables(s->quality, &tab);
    uint8_t framing[JP_FRAMING_BYTES];
    jp_write_framing(tab, W, H, s->restart_mcus, framing);
    de_ctx::JpegWork work;
    Dev<float> d_image;
    return coded_debug(c, g.capacity, jp_length, out, out_bytes, len, "out_bytes is smaller than the frame (*len)", [&](hipStream_t stream, uint8_t* d_out) -> int {
        int rc = jp_work_ensure(work, g);
        if (!rc) rc = debug_upload(stream, d_image, image, (size_t)W * H * 3 * sizeof(float));
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(work.tab, &tab, sizeof(tab), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_out + CS_WORD_BYTES, framing, sizeof(framing), hipMemcpyHostToDevice, stream));
        jp_launch(stream, d_image, work, g, d_out);
        return DE_OK;
    });
}
/* the host's part alone: no device, no context */
int de_debug_jpeg_framing(const de_jpeg* s, int W, int H, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity) {
    if (!s || W <= 0 || H <= 0 || (W & 1) || (H & 1) || W > 65534 || H > 65534) return fail(DE_ERR_INVALID, "bad arguments (W and H positive, even and below 65535)");
    { int rc = jp_settings_check(s); if (rc) return rc; }
    if (len) *len = JP_FRAMING_BYTES;
    if (capacity) *capacity = (uint64_t)jp_geometry(W, H, s->restart_mcus).capacity;
    if (out || out_bytes) {
        if (!out || out_bytes < JP_FRAMING_BYTES) return fail(DE_ERR_INVALID, "out_bytes is smaller than the framing (*len)");
        JpegTables tab;
        jp_make_tables(s->quality, &tab);
        jp_write_framing(tab, W, H, s->restart_mcus, (uint8_t*)out);
    }
    return DE_OK;
}

/* ---- PNG output: include/digital_earth_png.h (png_kernels.hip, png_tables.h) */
int de_set_png(de_ctx* c, const de_png* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = pn_settings_check(s); if (rc) return rc; }
    { int rc = refuse_in_flight(c->pn_coded.ring); if (rc) return rc; }
    c->pn = *s;
    coded_reset(c->pn_coded);
    return DE_OK;
}
int de_get_png(de_ctx* c, de_png* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->pn;
    return DE_OK;
}
int de_png_capacity(de_ctx* c, uint64_t* bytes) { return coded_capacity<PngOut>(c, bytes); }
int de_render_to_png(de_ctx* c, const void** device_stream, const uint64_t** device_len) { return coded_render_to<PngOut>(c, device_stream, device_len); }
int de_fetch_png_view(de_ctx* c, const void** host, uint64_t* len) { return coded_fetch_view<PngOut>(c, host, len); }
int de_fetch_png(de_ctx* c, void* out, uint64_t out_bytes, uint64_t* len) { return coded_fetch<PngOut>(c, out, out_bytes, len); }
int de_fetch_png_begin(de_ctx* c) { return coded_fetch_begin<PngOut>(c); }
int de_fetch_png_end(de_ctx* c, const void** host, uint64_t* len) { return coded_fetch_end<PngOut>(c, host, len); }
/* the conversion once on host-given packed pixels of any size.  Buffers of its own; the context's settings and streams are not touched. */
int de_debug_png(de_ctx* c, const void* pixels, int W, int H, int channels, int depth, const de_png* s, void* out, uint64_t out_bytes, uint64_t* len) {
    if (!c || !pixels || !s || !out || !len) return fail(DE_ERR_INVALID, "null argument");
    { int rc = pn_shape_check(W, H, channels, depth); if (rc) return rc; }
    { int rc = pn_settings_check(s); if (rc) return rc; }
    const PngGeometry g = png_geometry(W, H, channels, depth, s->chunk_bytes);
    de_ctx::PngWork work;
    return coded_debug(c, g.capacity, pn_length, out, out_bytes, len, "out_bytes is smaller than the file (*len)", [&](hipStream_t stream, uint8_t* d_out) -> int {
        int rc = pn_work_ensure(work, g);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(work.pixels, pixels, (size_t)g.H * g.row_bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(pn_tables_upload(stream, work));
        const uint8_t cicp[4] = {1, 8, 0, 1};
        pn_launch(stream, work, g, s->filter, cicp, d_out);
        return DE_OK;
    });
}
/* the host's part alone: no device, no context */
int de_debug_png_framing(const de_png* s, int W, int H, int channels, int depth, const uint8_t* cicp, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity) {
    if (!s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = pn_shape_check(W, H, channels, depth); if (rc) return rc; }
    { int rc = pn_settings_check(s); if (rc) return rc; }
    const PngGeometry g = png_geometry(W, H, channels, depth, s->chunk_bytes);
    if (len) *len = g.front;
    if (capacity) *capacity = (uint64_t)g.capacity;
    if (out || out_bytes) {
        if (!out || out_bytes < g.front) return fail(DE_ERR_INVALID, "out_bytes is smaller than the front (*len)");
        static const uint8_t linear709[4] = {1, 8, 0, 1};
        uint8_t front[PNG_FRONT_MAX];
        png_write_front(pn_host_tables(), g, cicp ? cicp : linear709, front);
        memcpy(out, front, g.front);
    }
    return DE_OK;
}

/* ---- OpenEXR output: include/digital_earth_exr.h (exr_kernels.hip, exr_tables.h) */
int de_set_exr(de_ctx* c, const de_exr* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = ex_settings_check(s); if (rc) return rc; }
    if (c->ex_aovs) { int rc = ex_shape_check(c->W, c->H, s->pixel_type, c->ex_aovs); if (rc) return rc; }      // the AOV channels in force count at the new pixel type
    { int rc = refuse_in_flight(c->ex_coded.ring); if (rc) return rc; }
    c->ex = *s;
    coded_reset(c->ex_coded);
    return DE_OK;
}
int de_get_exr(de_ctx* c, de_exr* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->ex;
    return DE_OK;
}
int de_exr_capacity(de_ctx* c, uint64_t* bytes) { return coded_capacity<ExrOut>(c, bytes); }
int de_render_to_exr(de_ctx* c, const void** device_stream, const uint64_t** device_len) { return coded_render_to<ExrOut>(c, device_stream, device_len); }
int de_fetch_exr_view(de_ctx* c, const void** host, uint64_t* len) { return coded_fetch_view<ExrOut>(c, host, len); }
int de_fetch_exr(de_ctx* c, void* out, uint64_t out_bytes, uint64_t* len) { return coded_fetch<ExrOut>(c, out, out_bytes, len); }
int de_fetch_exr_begin(de_ctx* c) { return coded_fetch_begin<ExrOut>(c); }
int de_fetch_exr_end(de_ctx* c, const void** host, uint64_t* len) { return coded_fetch_end<ExrOut>(c, host, len); }
/* the conversion once on a host-given image of any size, rows top-down.  Buffers of its own; the context's settings and streams are not touched. */
int de_debug_exr(de_ctx* c, const float* image, int W, int H, const de_exr* s, void* out, uint64_t out_bytes, uint64_t* len) {
    if (!c || !image || !s || !out || !len) return fail(DE_ERR_INVALID, "null argument");
    { int rc = ex_settings_check(s); if (rc) return rc; }
    { int rc = ex_shape_check(W, H, s->pixel_type); if (rc) return rc; }
    const ExrGeometry g = ex_geometry(W, H, *s);
    de_ctx::ExrWork work;
    Dev<float> d_image;
    return coded_debug(c, g.capacity, ex_length, out, out_bytes, len, "out_bytes is smaller than the file (*len)", [&](hipStream_t stream, uint8_t* d_out) -> int {
        int rc = ex_work_ensure(work, g);
        if (!rc) rc = debug_upload(stream, d_image, image, (size_t)W * H * 3 * sizeof(float));
        if (rc) return rc;
        HIP_TRY(ex_tables_upload(stream, work));
        return ex_launch(stream, work, g, linear_src(d_image, W, H), false, s->scale, d_out, no_hook);
    });
}
/* the host's part alone: no device, no context */
int de_debug_exr_framing(const de_exr* s, int W, int H, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity) {
    if (!s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = ex_settings_check(s); if (rc) return rc; }
    { int rc = ex_shape_check(W, H, s->pixel_type); if (rc) return rc; }
    const ExrGeometry g = ex_geometry(W, H, *s);
    if (len) *len = g.front;
    if (capacity) *capacity = (uint64_t)g.capacity;
    if (out || out_bytes) {
        if (!out || out_bytes < g.front) return fail(DE_ERR_INVALID, "out_bytes is smaller than the front (*len)");
        uint8_t front[EXR_FRONT_MAX];
        exr_write_front(g, front);
        memcpy(out, front, EXR_FRONT_FIXED);
        memset((uint8_t*)out + EXR_FRONT_FIXED, 0, g.front - EXR_FRONT_FIXED);
    }
    return DE_OK;
}

/* ---- EXR AOV channels: include/digital_earth_exr_aovs.h (exr_kernels.hip: exr_aov_layout_kernel, exr_tables.h) */
int de_set_exr_aovs(de_ctx* c, uint32_t mask) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    { int rc = ex_mask_check(mask); if (rc) return rc; }
    { int rc = ex_shape_check(c->W, c->H, c->ex.pixel_type, mask); if (rc) return rc; }
    { int rc = refuse_in_flight(c->ex_coded.ring); if (rc) return rc; }
    c->ex_aovs = mask;
    c->ex_coded.guess = 0;
    return DE_OK;
}
int de_get_exr_aovs(de_ctx* c, uint32_t* mask) {
    if (!c || !mask) return fail(DE_ERR_INVALID, "null argument");
    *mask = c->ex_aovs;
    return DE_OK;
}
/* the conversion with AOV channels once on host-given arrays of any size, rows top-down.  Buffers of its own; the context's settings are not touched. */
int de_debug_exr_aovs(de_ctx* c, const float* image, const float* guides, const float* s2, const float* counts, int W, int H, const de_exr* s, uint32_t mask,
                      void* out, uint64_t out_bytes, uint64_t* len) {
    if (!c || !image || !s || !out || !len) return fail(DE_ERR_INVALID, "null argument");
    { int rc = ex_settings_check(s); if (rc) return rc; }
    { int rc = ex_mask_check(mask); if (rc) return rc; }
    { int rc = ex_shape_check(W, H, s->pixel_type, mask); if (rc) return rc; }
    const ExrGeometry g = ex_geometry(W, H, *s, mask);
    uint32_t need = 0u;
    for (int k = 0; k < g.channels; ++k) need |= exr_slot_need(g.ch[k].slot);
    const bool need_guides = (need & (EXR_NEED_NC | EXR_NEED_AT | EXR_NEED_DIST)) != 0u;
    if (need_guides && !guides) return fail(DE_ERR_INVALID, "the mask selects guide channels: `guides` is null");
    if ((need & EXR_NEED_MOMENTS) && !s2) return fail(DE_ERR_INVALID, "the mask selects the variance: `s2` is null");
    if ((need & EXR_NEED_DIVISOR) && !counts) return fail(DE_ERR_INVALID, "the mask selects the variance or the samples: `counts` is null");
    const size_t npx = (size_t)W * H, image_bytes = npx * 3 * sizeof(float);
    std::vector<float4> nc, at;      // the uploads read them: alive until coded_debug has waited
    std::vector<float> dist;
    if (need_guides) {      // the nine guides of a pixel side by side, in de_fetch_guides' order, into the device's three buffers
        nc.resize(npx); at.resize(npx); dist.resize(npx);
        for (size_t p = 0; p < npx; ++p) {
            const float* q = guides + p * 9;
            nc[p] = make_float4(q[2], q[3], q[4], q[0]); at[p] = make_float4(q[5], q[6], q[7], q[8]); dist[p] = q[1];
        }
    }
    de_ctx::ExrWork work;
    Dev<float> d_image, d_s2, d_counts, d_dist;
    Dev<float4> d_nc, d_at;
    return coded_debug(c, g.capacity, ex_length, out, out_bytes, len, "out_bytes is smaller than the file (*len)", [&](hipStream_t stream, uint8_t* d_out) -> int {
        ExrAovSrc av;
        int rc = ex_work_ensure(work, g);
        if (!rc) rc = debug_upload(stream, d_image, image, image_bytes);
        if (!rc && need_guides) {
            rc = debug_upload(stream, d_nc, nc.data(), npx * sizeof(float4));
            if (!rc) rc = debug_upload(stream, d_at, at.data(), npx * sizeof(float4));
            if (!rc) rc = debug_upload(stream, d_dist, dist.data(), npx * sizeof(float));
            av.nc = d_nc; av.at = d_at; av.dist = d_dist;
        }
        if (!rc && (need & EXR_NEED_MOMENTS)) {
            rc = debug_upload(stream, d_s2, s2, image_bytes);
            av.s1 = d_image; av.s2 = d_s2;
        }
        if (!rc && counts) {      // the divisor of B, G, R too: `image` is read as the sums
            rc = debug_upload(stream, d_counts, counts, npx * sizeof(float));
            av.counts = d_counts;
        }
        if (rc) return rc;
        HIP_TRY(ex_tables_upload(stream, work));
        return ex_launch(stream, work, g, linear_src(d_image, W, H), false, s->scale, d_out, no_hook, av);      // without counts: x / 1.0f == x
    });
}
/* the host's part alone: no device, no context */
int de_debug_exr_aov_framing(const de_exr* s, uint32_t mask, int W, int H, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity) {
    if (!s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = ex_settings_check(s); if (rc) return rc; }
    { int rc = ex_mask_check(mask); if (rc) return rc; }
    { int rc = ex_shape_check(W, H, s->pixel_type, mask); if (rc) return rc; }
    const ExrGeometry g = ex_geometry(W, H, *s, mask);
    if (len) *len = g.front;
    if (capacity) *capacity = (uint64_t)g.capacity;
    if (out || out_bytes) {
        if (!out || out_bytes < g.front) return fail(DE_ERR_INVALID, "out_bytes is smaller than the front (*len)");
        uint8_t front[EXR_FRONT_MAX];
        const size_t n = exr_write_front(g, front);
        if (n != g.front_fixed) return fail(DE_ERR_INTERNAL, "the EXR front's length is not the geometry's");
        memcpy(out, front, n);
        memset((uint8_t*)out + n, 0, g.front - n);
    }
    return DE_OK;
}

/* ---- Radiance HDR output: include/digital_earth_rgbe.h (rgbe_kernels.hip, rgbe_tables.h) */
int de_set_rgbe(de_ctx* c, const de_rgbe* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = rg_settings_check(s); if (rc) return rc; }
    { int rc = refuse_in_flight(c->rg_coded.ring); if (rc) return rc; }
    c->rg = *s;
    coded_reset(c->rg_coded);
    return DE_OK;
}
int de_get_rgbe(de_ctx* c, de_rgbe* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->rg;
    return DE_OK;
}
int de_rgbe_capacity(de_ctx* c, uint64_t* bytes) { return coded_capacity<RgbeOut>(c, bytes); }
int de_render_to_rgbe(de_ctx* c, const void** device_stream, const uint64_t** device_len) { return coded_render_to<RgbeOut>(c, device_stream, device_len); }
int de_fetch_rgbe_view(de_ctx* c, const void** host, uint64_t* len) { return coded_fetch_view<RgbeOut>(c, host, len); }
int de_fetch_rgbe(de_ctx* c, void* out, uint64_t out_bytes, uint64_t* len) { return coded_fetch<RgbeOut>(c, out, out_bytes, len); }
int de_fetch_rgbe_begin(de_ctx* c) { return coded_fetch_begin<RgbeOut>(c); }
int de_fetch_rgbe_end(de_ctx* c, const void** host, uint64_t* len) { return coded_fetch_end<RgbeOut>(c, host, len); }
/* the conversion once on a host-given image of any size, rows top-down.  Buffers of its own; the context's settings and streams are not touched. */
int de_debug_rgbe(de_ctx* c, const float* image, int W, int H, const de_rgbe* s, void* out, uint64_t out_bytes, uint64_t* len) {
    if (!c || !image || !s || !out || !len) return fail(DE_ERR_INVALID, "null argument");
    { int rc = rg_settings_check(s); if (rc) return rc; }
    { int rc = rg_shape_check(W, H); if (rc) return rc; }
    const RgbeGeometry g = rg_geometry(W, H, *s);
    de_ctx::RgbeWork work;
    Dev<float> d_image;
    return coded_debug(c, g.capacity, rg_length, out, out_bytes, len, "out_bytes is smaller than the file (*len)", [&](hipStream_t stream, uint8_t* d_out) -> int {
        int rc = rg_work_ensure(work, g);
        if (!rc) rc = debug_upload(stream, d_image, image, (size_t)W * H * 3 * sizeof(float));
        if (rc) return rc;
        return rg_launch(stream, work, g, linear_src(d_image, W, H), false, s->rounding, d_out, no_hook);
    });
}
/* the host's part alone: no device, no context */
int de_debug_rgbe_framing(const de_rgbe* s, int W, int H, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity) {
    if (!s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = rg_settings_check(s); if (rc) return rc; }
    { int rc = rg_shape_check(W, H); if (rc) return rc; }
    const RgbeGeometry g = rg_geometry(W, H, *s);
    if (len) *len = g.header;
    if (capacity) *capacity = (uint64_t)g.capacity;
    if (out || out_bytes) {
        if (!out || out_bytes < g.header) return fail(DE_ERR_INVALID, "out_bytes is smaller than the front (*len)");
        memcpy(out, g.text, g.header);
    }
    return DE_OK;
}
/* The resampling and the conversion once on host-given linear faces, as de_debug_environment_exr.  Buffers and tables of its own; the context's
 * settings and slots are not touched.  The arguments and both settings are checked before the context is read. */
int de_debug_environment_rgbe(de_ctx* c, const float* faces, int n, const de_panorama* p, const de_rgbe* s, void* out, uint64_t out_bytes, uint64_t* len) {
    if (!c || !faces || !p || !s || !out || !len || n < 4 || n > 16384) return fail(DE_ERR_INVALID, "bad arguments (faces of 4 ... 16384 pixels a side)");
    { int rc = pano_settings_check(p, n); if (rc) return rc; }
    { int rc = rg_settings_check(s); if (rc) return rc; }
    { int rc = rg_shape_check(p->width, p->height); if (rc) return rc; }
    const RgbeGeometry g = rg_geometry(p->width, p->height, *s);
    EnvDebug env;
    de_ctx::RgbeWork work;
    return coded_debug(c, g.capacity, rg_length, out, out_bytes, len, "out_bytes is smaller than the file (*len)", [&](hipStream_t stream, uint8_t* d_out) -> int {
        DisplaySrc src;
        int rc = rg_work_ensure(work, g);
        if (!rc) rc = env_debug_source(stream, env, faces, n, *p, &src);
        if (rc) return rc;
        return rg_launch(stream, work, g, src, true, s->rounding, d_out, no_hook);
    });
}

/* ---- the IBL output: include/digital_earth_ibl.h (ibl_kernels.hip, ibl_body.h, ibl_tables.h) */
namespace {
int ibl_settings_check(const de_ibl* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_ibl)) return fail(DE_ERR_INVALID, "de_ibl.struct_bytes does not match this library's struct");
    if (const char* fault = ibl_settings_fault(s->edge, s->levels, s->samples, s->supersample, s->lod_bias, s->pixel_type)) return fail(DE_ERR_INVALID, fault);
    return DE_OK;
}
unsigned ibl_blocks(int e) { const unsigned tiles = (unsigned)((e + IBL_TILE - 1) / IBL_TILE); return 6u * tiles * tiles; }
size_t ibl_spec_offset(int E, int l) { return ibl_level_offset(E, l) - ibl_level_offset(E, 1); }      // floats in front of specular level l >= 1
// The whole bake on `stream`, waited for: faces [6][N][N][3] with the constants of their panorama in `k` -> everything in `w`.
int ibl_run(hipStream_t stream, de_ctx::IblWork& w, const PanoArgs& k, int N, const float* faces, const de_ibl& s) {
    const int E = s.edge, L = s.levels, M = ibl_log2(E) + 1, es = E < IBL_SH_EDGE ? E : IBL_SH_EDGE, groups = (6 * es * es + IBL_THREADS - 1) / IBL_THREADS;
    // the tables, in double on the host, rounded once; they outlive their uploads: this call waits for the stream before it returns
    std::vector<IblSample> tab, level_tab;
    std::vector<float> omega;
    int first[IBL_MAX_LEVELS] = {}, kept[IBL_MAX_LEVELS] = {};
    for (int l = 1; l < L; ++l) {
        ibl_build_samples(E, L, s.samples, l, s.lod_bias, &level_tab);
        first[l] = (int)tab.size(); kept[l] = (int)level_tab.size();
        tab.insert(tab.end(), level_tab.begin(), level_tab.end());
    }
    ibl_build_omega(es, &omega);
    int rc = w.mips.ensure(ibl_level_offset(E, M) * sizeof(float), "the IBL buffers");
    if (!rc) rc = w.spec.ensure(ibl_spec_offset(E, L) * sizeof(float), "the IBL buffers");
    if (!rc) rc = w.tab.ensure((tab.size() + 1) * sizeof(IblSample), "the IBL buffers");
    if (!rc) rc = w.omega.ensure(omega.size() * sizeof(float), "the IBL buffers");
    if (!rc) rc = w.partial.ensure((size_t)groups * 27 * sizeof(float), "the IBL buffers");
    if (!rc) rc = w.sh.ensure(27 * sizeof(float), "the IBL buffers");
    if (!rc) rc = w.payload.ensure(ibl_payload_bytes(E, L, s.pixel_type), "the IBL buffers");
    if (rc) return rc;
    StreamWait wait{stream};
    if (!tab.empty()) HIP_TRY(hipMemcpyAsync(w.tab, tab.data(), tab.size() * sizeof(IblSample), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(w.omega, omega.data(), omega.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    PanoArgs p = k;
    p.faces = faces; p.out = nullptr; p.N = N; p.width = 0; p.height = 0; p.S = s.supersample; p.fisheye = 0;
    p.sin_lon = p.cos_lon = p.sin_lat = p.cos_lat = nullptr;
    hipLaunchKernelGGL(ibl_base_kernel, dim3(ibl_blocks(E)), dim3(IBL_THREADS), 0, stream, p, w.mips.get(), E, s.supersample);
    for (int m = 1; m < M; ++m)
        hipLaunchKernelGGL(ibl_mip_kernel, dim3(ibl_blocks(E >> m)), dim3(IBL_THREADS), 0, stream, w.mips + ibl_level_offset(E, m - 1), w.mips + ibl_level_offset(E, m), E >> m);
    IblLevelArgs a = {};
    a.mips = w.mips; a.omega = w.omega; a.E = E; a.M = M;
    for (int m = 0; m < M; ++m) a.off[m] = (uint32_t)ibl_level_offset(E, m);
    for (int l = 1; l < L; ++l) {
        a.out = w.spec + ibl_spec_offset(E, l); a.tab = w.tab + first[l]; a.n = kept[l]; a.e = E >> l;
        hipLaunchKernelGGL(ibl_spec_kernel, dim3(ibl_blocks(a.e)), dim3(IBL_THREADS), 0, stream, a);
    }
    hipLaunchKernelGGL(ibl_sh_kernel, dim3((unsigned)groups), dim3(IBL_THREADS), 0, stream, w.mips + ibl_level_offset(E, ibl_log2(E / es)), w.omega.get(), es, w.partial.get());
    hipLaunchKernelGGL(ibl_sh_final_kernel, dim3(1), dim3(64), 0, stream, w.partial.get(), groups, w.sh.get());
    IblPackArgs q = {};
    q.mips = w.mips; q.spec = w.spec; q.out = w.payload; q.E = E; q.L = L; q.half = s.pixel_type == DE_EXR_PIXEL_HALF ? 1 : 0;
    q.texels_per_face = (uint32_t)ibl_texels_before(E, L);
    for (int l = 1; l < L; ++l) q.spec_off[l] = (uint32_t)ibl_spec_offset(E, l);
    hipLaunchKernelGGL(ibl_pack_kernel, dim3((6u * q.texels_per_face + IBL_THREADS - 1) / IBL_THREADS), dim3(IBL_THREADS), 0, stream, q);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return DE_OK;
}
// device -> the caller's memory on `stream`, waited for
int ibl_copy_out(hipStream_t stream, void* out, const void* d_src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(out, d_src, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return DE_OK;
}
const float* ibl_level_block(const de_ctx::IblWork& w, int E, int level) { return level == 0 ? w.mips.get() : w.spec + ibl_spec_offset(E, level); }
int ibl_dds_out(hipStream_t stream, const de_ctx::IblWork& w, const de_ibl& s, void* out) {
    ibl_dds_header(s.edge, s.levels, s.pixel_type, (uint8_t*)out);
    return ibl_copy_out(stream, (uint8_t*)out + IBL_DDS_HEADER, w.payload, ibl_payload_bytes(s.edge, s.levels, s.pixel_type));
}
}  // namespace
int de_set_ibl(de_ctx* c, const de_ibl* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = ibl_settings_check(s); if (rc) return rc; }
    c->ibl = *s;
    c->ibl_built = false;
    c->ibl_bc6h_made = false;
    return DE_OK;
}
int de_get_ibl(de_ctx* c, de_ibl* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->ibl;
    return DE_OK;
}
int de_ibl_build(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    if (!c->pano.on) return fail(DE_ERR_STATE, "the panorama is off (de_set_panorama): the IBL bake reads its six linear faces");
    if (c->env_mask != 63u) return fail(DE_ERR_STATE, "fewer than six linear faces are captured (de_environment_capture)");
    HIP_TRY(hipSetDevice(c->device));
    c->ibl_built = false;
    c->ibl_bc6h_made = false;
    int rc = ibl_run(c->stream, c->ibl_work, c->pano_consts, c->W, c->env_faces, c->ibl);
    if (rc) return rc;
    c->ibl_built = true;
    return DE_OK;
}
int de_fetch_ibl_sh(de_ctx* c, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (!c->ibl_built) return fail(DE_ERR_STATE, "no IBL product is held (de_ibl_build)");
    HIP_TRY(hipSetDevice(c->device));
    return ibl_copy_out(c->stream, out, c->ibl_work.sh, 27 * sizeof(float));
}
int de_fetch_ibl_face(de_ctx* c, int level, int face, float* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (level < 0 || level >= c->ibl.levels) return fail(DE_ERR_INVALID, "level must lie in 0 ... de_ibl.levels - 1");
    if (face < 0 || face >= DE_PANO_FACES) return fail(DE_ERR_INVALID, "face must lie in 0 ... 5");
    if (!c->ibl_built) return fail(DE_ERR_STATE, "no IBL product is held (de_ibl_build)");
    HIP_TRY(hipSetDevice(c->device));
    const size_t e = (size_t)(c->ibl.edge >> level), floats = e * e * 3;
    return ibl_copy_out(c->stream, out, ibl_level_block(c->ibl_work, c->ibl.edge, level) + (size_t)face * floats, floats * sizeof(float));
}
int de_ibl_file_bytes(de_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return fail(DE_ERR_INVALID, "null argument");
    *bytes = (uint64_t)IBL_DDS_HEADER + (uint64_t)ibl_payload_bytes(c->ibl.edge, c->ibl.levels, c->ibl.pixel_type);
    return DE_OK;
}
int de_fetch_ibl_dds(de_ctx* c, void* out, uint64_t out_bytes) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (out_bytes < (uint64_t)IBL_DDS_HEADER + (uint64_t)ibl_payload_bytes(c->ibl.edge, c->ibl.levels, c->ibl.pixel_type)) return fail(DE_ERR_INVALID, "out_bytes is smaller than the file (de_ibl_file_bytes)");
    if (!c->ibl_built) return fail(DE_ERR_STATE, "no IBL product is held (de_ibl_build)");
    HIP_TRY(hipSetDevice(c->device));
    return ibl_dds_out(c->stream, c->ibl_work, c->ibl, out);
}
/* The bake once on host-given linear faces.  Buffers and tables of its own; the context's settings, slots and product are not touched.  The arguments
 * and both settings are checked before the context is read. */
int de_debug_ibl(de_ctx* c, const float* faces, int n, const de_panorama* p, const de_ibl* s, float* sh, float* levels, void* dds, uint64_t dds_bytes) {
    if (!c || !faces || !p || !s || n < 4 || n > 16384) return fail(DE_ERR_INVALID, "bad arguments (faces of 4 ... 16384 pixels a side)");
    { int rc = pano_settings_check(p, n); if (rc) return rc; }
    { int rc = ibl_settings_check(s); if (rc) return rc; }
    if (dds && dds_bytes < (uint64_t)IBL_DDS_HEADER + (uint64_t)ibl_payload_bytes(s->edge, s->levels, s->pixel_type)) return fail(DE_ERR_INVALID, "dds_bytes is smaller than the file");
    HIP_TRY(hipSetDevice(c->device));
    Dev<float> d_faces;
    de_ctx::IblWork work;
    PanoArgs k = {};
    pano_make_consts(*p, n, &k);
    StreamWait wait{c->stream};
    int rc = debug_upload(c->stream, d_faces, faces, (size_t)DE_PANO_FACES * (size_t)n * (size_t)n * 3 * sizeof(float));
    if (!rc) rc = ibl_run(c->stream, work, k, n, d_faces, *s);
    if (!rc && sh) rc = ibl_copy_out(c->stream, sh, work.sh, 27 * sizeof(float));
    for (int l = 0; !rc && levels && l < s->levels; ++l) {
        const size_t floats = (size_t)(s->edge >> l) * (size_t)(s->edge >> l) * 18;
        rc = ibl_copy_out(c->stream, levels + ibl_level_offset(s->edge, l), ibl_level_block(work, s->edge, l), floats * sizeof(float));
    }
    if (!rc && dds) rc = ibl_dds_out(c->stream, work, *s, dds);
    return rc;
}

/* ---- the IBL output, compressed: include/digital_earth_ibl_bc6h.h (bc6h_kernels.hip, bc6h_body.h, bc6h_tables.h) */
namespace {
int bc6h_settings_check(const de_ibl_bc6h* s) {
    if (s->struct_bytes != (uint32_t)sizeof(de_ibl_bc6h)) return fail(DE_ERR_INVALID, "de_ibl_bc6h.struct_bytes does not match this library's struct");
    if (const char* fault = bc6h_settings_fault(s->on, s->quality)) return fail(DE_ERR_INVALID, fault);
    return DE_OK;
}
// the launch's offset table: `images` images per face, `faces` faces
void bc6h_args_finish(Bc6hArgs* a, uint32_t images, uint32_t faces, uint8_t* out) {
    a->images = images; a->first[0] = 0u;
    for (uint32_t m = 0; m < images; ++m) a->first[m + 1] = a->first[m] + ((a->w[m] + 3u) / 4u) * ((a->h[m] + 3u) / 4u);
    a->per_face = a->first[images]; a->total = a->per_face * faces; a->out = out;
}
// every block of the launch, one launch
void bc6h_launch(hipStream_t stream, const Bc6hArgs& a, int quality) {
    if (quality == 0) hipLaunchKernelGGL(bc6h_q0_kernel, dim3((a.total + BC6H_Q0_GROUP_BLOCKS - 1u) / BC6H_Q0_GROUP_BLOCKS), dim3(BC6H_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(bc6h_q1_kernel, dim3((a.total + BC6H_Q1_GROUP_BLOCKS - 1u) / BC6H_Q1_GROUP_BLOCKS), dim3(BC6H_THREADS), 0, stream, a);
}
// the chain held in `w` (after ibl_run) -> w.bc6h, waited for
int bc6h_run(hipStream_t stream, de_ctx::IblWork& w, const de_ibl& s, int quality) {
    int rc = w.bc6h.ensure(bc6h_payload_bytes(s.edge, s.levels), "the BC6H blocks");
    if (rc) return rc;
    Bc6hArgs a = {};
    for (int l = 0; l < s.levels; ++l) { a.src[l] = ibl_level_block(w, s.edge, l); a.w[l] = a.h[l] = (uint32_t)(s.edge >> l); }
    bc6h_args_finish(&a, (uint32_t)s.levels, 6u, w.bc6h.get());
    bc6h_launch(stream, a, quality);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return DE_OK;
}
int bc6h_dds_out(hipStream_t stream, const de_ctx::IblWork& w, const de_ibl& s, void* out) {
    bc6h_dds_header(s.edge, s.levels, (uint8_t*)out);
    return ibl_copy_out(stream, (uint8_t*)out + IBL_DDS_HEADER, w.bc6h, bc6h_payload_bytes(s.edge, s.levels));
}
}  // namespace
int de_set_ibl_bc6h(de_ctx* c, const de_ibl_bc6h* s) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = bc6h_settings_check(s); if (rc) return rc; }
    c->ibl_bc6h = *s;
    c->ibl_bc6h_made = false;
    return DE_OK;
}
int de_get_ibl_bc6h(de_ctx* c, de_ibl_bc6h* out) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    *out = c->ibl_bc6h;
    return DE_OK;
}
int de_ibl_bc6h_file_bytes(de_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return fail(DE_ERR_INVALID, "null argument");
    *bytes = (uint64_t)IBL_DDS_HEADER + (uint64_t)bc6h_payload_bytes(c->ibl.edge, c->ibl.levels);
    return DE_OK;
}
int de_fetch_ibl_bc6h_dds(de_ctx* c, void* out, uint64_t out_bytes) {
    if (!c || !out) return fail(DE_ERR_INVALID, "null argument");
    if (out_bytes < (uint64_t)IBL_DDS_HEADER + (uint64_t)bc6h_payload_bytes(c->ibl.edge, c->ibl.levels)) return fail(DE_ERR_INVALID, "out_bytes is smaller than the file (de_ibl_bc6h_file_bytes)");
    if (!c->ibl_bc6h.on) return fail(DE_ERR_STATE, "the BC6H stage is off (de_set_ibl_bc6h)");
    if (!c->ibl_built) return fail(DE_ERR_STATE, "no IBL product is held (de_ibl_build)");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->ibl_bc6h_made) {
        int rc = bc6h_run(c->stream, c->ibl_work, c->ibl, c->ibl_bc6h.quality);
        if (rc) return rc;
        c->ibl_bc6h_made = true;
    }
    return bc6h_dds_out(c->stream, c->ibl_work, c->ibl, out);
}
/* The encoder alone on a host-given image.  Buffers of its own; the arguments and the settings are checked before the context is read. */
int de_debug_bc6h_encode(de_ctx* c, const float* rgb, int w, int h, const de_ibl_bc6h* s, void* blocks, uint64_t bytes) {
    if (!c || !rgb || !s || !blocks || w < 1 || h < 1 || w > 16384 || h > 16384) return fail(DE_ERR_INVALID, "bad arguments (an image of 1 ... 16384 texels a side)");
    { int rc = bc6h_settings_check(s); if (rc) return rc; }
    const size_t need = (size_t)((w + 3) / 4) * (size_t)((h + 3) / 4) * 16;
    if (bytes < (uint64_t)need) return fail(DE_ERR_INVALID, "bytes is smaller than the blocks (16 ceil(w / 4) ceil(h / 4))");
    HIP_TRY(hipSetDevice(c->device));
    Dev<float> d_image;
    Dev<uint8_t> d_blocks;
    StreamWait wait{c->stream};
    int rc = debug_upload(c->stream, d_image, rgb, (size_t)w * (size_t)h * 3 * sizeof(float));
    if (!rc) rc = d_blocks.ensure(need, "the BC6H blocks");
    if (rc) return rc;
    Bc6hArgs a = {};
    a.src[0] = d_image; a.w[0] = (uint32_t)w; a.h[0] = (uint32_t)h;
    bc6h_args_finish(&a, 1u, 1u, d_blocks.get());
    bc6h_launch(c->stream, a, s->quality);
    HIP_TRY(hipGetLastError());
    return ibl_copy_out(c->stream, blocks, d_blocks, need);
}
/* de_debug_ibl with the compressed file out, and the half integers the blocks encode. */
int de_debug_ibl_bc6h(de_ctx* c, const float* faces, int n, const de_panorama* p, const de_ibl* s, const de_ibl_bc6h* b, float* sh, float* levels, uint16_t* half_levels, void* dds, uint64_t dds_bytes) {
    if (!c || !faces || !p || !s || !b || n < 4 || n > 16384) return fail(DE_ERR_INVALID, "bad arguments (faces of 4 ... 16384 pixels a side)");
    { int rc = pano_settings_check(p, n); if (rc) return rc; }
    { int rc = ibl_settings_check(s); if (rc) return rc; }
    { int rc = bc6h_settings_check(b); if (rc) return rc; }
    if (dds && dds_bytes < (uint64_t)IBL_DDS_HEADER + (uint64_t)bc6h_payload_bytes(s->edge, s->levels)) return fail(DE_ERR_INVALID, "dds_bytes is smaller than the file");
    HIP_TRY(hipSetDevice(c->device));
    Dev<float> d_faces;
    de_ctx::IblWork work;
    PanoArgs k = {};
    pano_make_consts(*p, n, &k);
    StreamWait wait{c->stream};
    int rc = debug_upload(c->stream, d_faces, faces, (size_t)DE_PANO_FACES * (size_t)n * (size_t)n * 3 * sizeof(float));
    if (!rc) rc = ibl_run(c->stream, work, k, n, d_faces, *s);
    if (!rc && sh) rc = ibl_copy_out(c->stream, sh, work.sh, 27 * sizeof(float));
    const size_t all = ibl_level_offset(s->edge, s->levels);
    std::vector<float> held;
    if (!rc && (levels || half_levels)) {
        float* to = levels;
        if (!to) { held.resize(all); to = held.data(); }
        for (int l = 0; !rc && l < s->levels; ++l) {
            const size_t floats = (size_t)(s->edge >> l) * (size_t)(s->edge >> l) * 18;
            rc = ibl_copy_out(c->stream, to + ibl_level_offset(s->edge, l), ibl_level_block(work, s->edge, l), floats * sizeof(float));
        }
        for (size_t i = 0; !rc && half_levels && i < all; ++i) {      // TEXEL TO HALF, on the host: the same two functions the kernel calls
            const uint32_t h = exr_half_bits(exr_sample_bits(to[i], 1.0f));
            half_levels[i] = (uint16_t)((h & 0x8000u) ? 0u : h);
        }
    }
    if (!rc && dds) rc = bc6h_run(c->stream, work, *s, b->quality);
    if (!rc && dds) rc = bc6h_dds_out(c->stream, work, *s, dds);
    return rc;
}

/* ---- look LUTs: include/digital_earth_look.h (look_kernels.hip) */
int de_set_look(de_ctx* c, const de_look* s, const float* table_1d, const float* table_3d) {
    if (!c || !s) return fail(DE_ERR_INVALID, "null argument");
    { int rc = lk_settings_check(s, table_1d, table_3d); if (rc) return rc; }
    HIP_TRY(hipSetDevice(c->device));
    de_ctx::LookDev fresh;
    { int rc = lk_upload(c->stream, *s, table_1d, table_3d, fresh); if (rc) return rc; }
    c->lk_dev = std::move(fresh);      // the previous tables go: hipFree waits for a display in flight that still reads them (a lagged fetch)
    c->lk = *s;
    c->lk.enabled = s->enabled ? 1 : 0;
    c->lk_on = s->enabled != 0;
    return DE_OK;
}
int de_get_look(de_ctx* c, de_look* out) { return get_settings(c, &de_ctx::lk_on, &de_ctx::lk, out); }
/* the kernel once on n host-given pixels.  Buffers of its own; the context's look is not touched. */
int de_debug_look(de_ctx* c, const float* rgb, uint64_t n, const de_look* s, const float* table_1d, const float* table_3d, float* out) {
    if (!c || !rgb || !s || !out || n == 0 || n > (1ull << 28)) return fail(DE_ERR_INVALID, "bad arguments (1 <= n_pixels <= 2^28)");
    { int rc = lk_settings_check(s, table_1d, table_3d); if (rc) return rc; }
    if (!s->size_1d && !s->size_3d) return fail(DE_ERR_INVALID, "de_look: no table");
    HIP_TRY(hipSetDevice(c->device));
    de_ctx::LookDev t;
    { int rc = lk_upload(c->stream, *s, table_1d, table_3d, t); if (rc) return rc; }
    const size_t bytes[1] = {(size_t)n * 3 * sizeof(float)};      // in place
    const void* const in[1] = {rgb};
    return debug_round_trip(c->stream, bytes, in, 0, out, [&](void* const* b) { lk_launch(c->stream, (float*)b[0], n, *s, t); return hipSuccess; });
}

/* the transform alone on n colours.  Buffers of its own; the context's setting is not touched. */
int de_debug_hdr_transform(de_ctx* c, const float* rgb, uint64_t n, const de_hdr_output* s, float* out) {
    if (!c || !rgb || !s || !out || n == 0 || n > (1ull << 28)) return fail(DE_ERR_INVALID, "bad arguments (1 <= n <= 2^28)");
    { int rc = ho_settings_check(s); if (rc) return rc; }
    HdrConsts h;
    hdr_output_consts((double)s->peak_nits, s->gamut, s->transfer, &h);
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes[2] = {(size_t)n * 3 * sizeof(float), (size_t)n * 3 * sizeof(float)};
    const void* const in[2] = {rgb, nullptr};
    return debug_round_trip(c->stream, bytes, in, 1, out, [&](void* const* b) { hipLaunchKernelGGL(hdr_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const float*)b[0], (float*)b[1], (size_t)n, h); return hipSuccess; });
}
/* include/digital_earth_debug.h: the constants alone, on the host.  settings = NULL: the six constants setup_kernel is handed for the SDR display
 * (opendrt_consts), the other thirteen 0 — so that a test can put the two host functions side by side. */
int de_debug_hdr_consts(de_ctx* c, const de_hdr_output* s, float* out19) {
    (void)c;      // host only: the context is not read and may be NULL
    if (!out19) return fail(DE_ERR_INVALID, "null argument");
    if (!s) {
        memset(out19, 0, 19 * sizeof(float));
        opendrt_consts(&out19[0], &out19[1], &out19[2], &out19[3], &out19[4], &out19[5]);
        return DE_OK;
    }
    { int rc = ho_settings_check(s); if (rc) return rc; }
    HdrConsts h;
    hdr_output_consts((double)s->peak_nits, s->gamut, s->transfer, &h);
    const float first[6] = {h.m, h.s, h.fl, h.ds, h.clamp_max, h.dch_s}, last[4] = {h.h_a, h.h_b, h.h_c, h.h_e};
    memcpy(out19, first, sizeof(first)); memcpy(out19 + 6, h.xyz_to_display, sizeof(h.xyz_to_display)); memcpy(out19 + 15, last, sizeof(last));
    return DE_OK;
}

}  // extern "C"

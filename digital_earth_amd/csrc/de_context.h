// de_context.h — the context behind the C ABI (include/digital_earth.h): device memory, streams, launch slots, what the launches need to know.
#pragma once
#include "de_kernels.h"
#include "../../include/digital_earth_exposure.h"
#include "../../include/digital_earth_bloom.h"
#include "../../include/digital_earth_history.h"
#include "../../include/digital_earth_pixels.h"
#include "../../include/digital_earth_local_exposure.h"
#include "../../include/digital_earth_output_scale.h"
#include "../../include/digital_earth_panorama.h"
#include "../../include/digital_earth_hdr_output.h"
#include "../../include/digital_earth_video.h"
#include "../../include/digital_earth_look.h"
#include "../../include/digital_earth_jpeg.h"
#include "../../include/digital_earth_png.h"
#include "../../include/digital_earth_exr.h"
#include "../../include/digital_earth_exr_aovs.h"
#include "../../include/digital_earth_environment.h"
#include "../../include/digital_earth_rgbe.h"
#include "../../include/digital_earth_ibl.h"
#include "../../include/digital_earth_ibl_bc6h.h"

#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>

// single translation unit: the kernels are compiled together with the host API.  pt_leaves.h (the integrator's leaves) comes in through each of
// the first three; the per-lane path tracer is in the legacy library only.
#include "render_kernel.hip"          // the ray marcher, the per-lane pieces (Tracer) and kernel body
#include "render_kernel_v2.hip"       // path_tracer as a wave-level state machine
#include "de_stages.h"                // path_tracer in stage form, under render_kernel_v6.hip
#ifdef DE_LEGACY_VARIANTS
#include "legacy/render_kernel_v1.hip"
#include "legacy/render_kernel_v3.hip"
#include "legacy/render_kernel_v5.hip"
#endif
#include "render_kernel_v6.hip"
#include "aux_kernels.hip"
#include "adaptive_kernels.hip"
#include "denoise_kernels.hip"
#include "exposure_kernels.hip"
#include "bloom_kernels.hip"
#include "history_kernels.hip"
#include "pixels_kernels.hip"
#include "output_scale_kernels.hip"
#include "panorama_kernels.hip"
#include "environment_kernels.hip"
#include "local_exposure_kernels.hip"
#include "hdr_output_kernels.hip"
#include "videoframe_kernels.hip"
#include "look_kernels.hip"
#include "jpeg_kernels.hip"
#include "png_kernels.hip"
#include "exr_kernels.hip"
#include "rgbe_kernels.hip"
#include "ibl_kernels.hip"
#include "bc6h_kernels.hip"

namespace {

#define DE_N_COUNTERS 64   // 0-6 work counters, 7-8 trips / passes, 16-47 scheduler statistics, 48-59 section timers (render_kernel_v2 MODE 1)
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(DE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define HIP_RET(expr)       /* in a function that answers a hipError_t: hand a failure on */ \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return e_;                                                    \
    } while (0)

}  // namespace
#include "de_memory.h"      // Dev<T>, Pinned<T>: what owns every allocation below
namespace {

enum { DE_FRAME_NONE = 0, DE_FRAME_UNIFORM = 1, DE_FRAME_ADAPTIVE = 2 };   // de_ctx::frame_kind

#define DE_MAX_SLOTS 8
#define DE_FETCH_RING 4      // de_fetch_image_begin / _end: fetches in flight (a lone one-sample launch takes ~10 ms, its longest path: 2 / 3 / 4 frames in flight run at 5.1 / 4.1 / ~3.5 ms per frame)
struct LaunchSlot {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;           // recorded after the slot's latest accumulate_kernel
    hipEvent_t t0 = nullptr, t1 = nullptr;
    Dev<uint2> contrib;                  // per-sample (radiance, wavelength node) records of the launch in this slot
    size_t contrib_items = 0;
    bool pending = false;                // `done` has not been waited for by the context stream yet
    bool launched = false;               // `done` has been recorded at least once (an event never recorded reads as complete)
    uint64_t seen_render = 0, seen_hdr = 0;
};

// What a fetch leaves the GPU through.  de_fetch.h holds every operation on it (begin, end, the synchronous path), once.
struct FetchRing {                       // the lagged fetches of one output: begun - ended = fetches in flight, at most DE_FETCH_RING
    const char* noun;                    // for messages: "pixel", and the entry points' stem, "de_fetch_pixels" (+ "_begin" / "_end")
    const char* entry;
    Pinned<void> cell[DE_FETCH_RING];     // fetch n is copied into cell n % DE_FETCH_RING ...
    hipEvent_t ev[DE_FETCH_RING] = {};   // ... and its event recorded behind the copy
    unsigned begun = 0, ended = 0;       // calls of _begin and of _end
};
struct PackedOut {                       // an output converted from the displayed image: 8-bit pixels, HDR pixels, video frames
    const char* noun;
    Dev<uint8_t> dev;                    // the packed output; sized for the largest format at the output size, so that a change of format frees nothing
    Pinned<void> stage;                  // where a synchronous fetch lands
    uint32_t count = 0, last_phase = 0;  // conversions since the settings were set; the dither phase of the newest
};
struct CodedOut {                        // an output whose length the device decides (the JPEG stream, the PNG, OpenEXR and Radiance files): on the device, the 16-byte word, then the stream
    PackedOut out;                       // the stream of the synchronous fetches; its staging buffer grows to the longest frame fetched, not to the capacity
    FetchRing ring;                      // the lagged ones: a fetch copies a prefix at _begin and, should the frame be longer, the whole of it at _end ...
    Dev<uint8_t> cell[DE_FETCH_RING];    // ... from a device stream of its own per ring cell, which the next _begin does not touch
    size_t copied[DE_FETCH_RING] = {};   // bytes of cell k that _begin copied into the pinned cell
    size_t guess = 0;                    // the prefix _begin copies: a quarter more than the newest frame ended; 0: the output's first estimate
    bool reads_pano[DE_FETCH_RING] = {}; // the lagged fetch in ring cell k reads what de_set_panorama replaces: a displayed output always, a scene-linear
                                         // one (EXR, RGBE) where it was begun on the scene-linear panorama (env_faces, env_out, the tables)
};

struct DevTexture {
    int w = 0, h = 0, ch = 0;
    Dev<uint8_t> linear;          // as uploaded: [h][w][ch]; a borrower holds none
    Dev<uint32_t> packed;         // footprint tiles (ch == 1) or rgbx dwords (ch == 3)
    int tiles_x = 0, tiles_y = 0;
    int packed_clamp = -1;        // address mode the packed copy was built with
    Dev<uint8_t> bound;           // the cloud map only: its occupancy bound (DE_CLOUD_BOUND_BYTES), rebuilt with the packed copy
    bool set = false;
    bool borrowed() const { return packed.borrowed(); }      // the packed copy and the bound are views of another context's (de_share_textures)
};

}  // namespace

struct de_ctx {
    int device = 0;
    int W = 0, H = 0;
    de_params p;
    bool params_dirty = true;     // FrameConsts must be rebuilt (any scalar parameter, the topography width)
    bool nodes_dirty = true;      // the wavelength table must be rebuilt (LUTs, address mode, fixed wavelength)
    int tune_pend = 18, tune_heavy = 13, tune_b = 24, tune_gas = 6, tune_chunk = 128, tune_wpc = 20, tune_max_spp = 0;   // DE_V2_* overrides, read once in de_create
    hipStream_t stream = nullptr;   // the context stream: everything except the render launches (reset, display, fetch, reduce, uploads)
    bool own_stream = false;
    // Launch slots (round 3): de_accumulate does not launch on the context stream.  Launch k goes to slot k % n_slots, which has
    // its own stream, work counter and contribution buffer, so that consecutive launches overlap — the next render kernel
    // fills the machine while the last long paths of the previous one drain (the reference's interactive loop is
    // accumulate() x 1 per frame, earth_viewer.py:241-243).  The accumulate_kernels, which read-modify-write the HDR buffer,
    // are chained with events in launch order, so the per-pixel sums keep their association.  The context stream waits for
    // the slots lazily (join_slots) before anything that reads or writes the HDR buffer or rewrites what a launch reads.
    LaunchSlot slot[DE_MAX_SLOTS];
    int n_slots = 8, big_slots = 3, next_slot = 0, last_slot = -1;   // launches with > 96 MB of records cycle through the first big_slots only
    int last_v6_slot = -1;          // the slot of the newest render_kernel_v6 launch (the tail's "has a successor on another slot" word is about v6 launches only)
    int cu_withhold = 0;            // de_tuning.v6_cu_withhold: CUs per XCD the launch slots' streams may NOT use (hipExtStreamCreateWithCUMask), so that small kernels of
                                    // the context stream (collective, accumulate, display) find a free CU while persistent workgroups own the others; 0 = plain streams
    Dev<float> d_standin;     // de_debug_standin_reduce: its second operand (zeros), its output and its copy target, [3][H][W][3]
    hipEvent_t ev_standin[16][2] = {};   // the last 16 stand-in collectives: de_last_reduce_ms answers their MEAN queue-to-finish time (frames in flight: no host wait per frame)
    unsigned standin_count = 0;
    bool last_reduce_standin = false;
    hipEvent_t ev_main = nullptr;   // last state of the context stream the slots may have to wait for
    uint64_t gen_render = 1, gen_hdr = 1, rec_render = 0, rec_hdr = 0;   // generations of context-stream work that launches depend on
    int t0_slot = -1, t1_slot = -1;
    bool timing_valid = false;
    bool timing_empty = false;      // the last de_accumulate launched nothing (an empty share): its duration is 0, not the previous call's
    DevTexture tex[DE_TEX_COUNT];
    Dev<float> d_cie;      // 441 x 2 x 3 (f16-quantised)
    Dev<float> d_srgb2spec;
    Dev<float> d_o3;
    Dev<float> d_crf;      // [n][1024][3]
    int n_crf = 0;
    bool luts_set = false;
    bool luts_borrowed() const { return d_cie.borrowed(); }      // the four tables are views of another context's (de_share_textures)
    Dev<FrameConsts> d_fc;
    Dev<LambdaNode> d_nodes;
    Dev<float> d_node_val;
    float* d_hdr = nullptr;      // a view: [H][W][3], d_hdr_own or the buffer bound by de_bind_hdr
    Dev<float> d_hdr_own;
    Dev<float> d_image;    // (W, H, 3)
    Dev<float> d_scratch;  // (W, H, 3) / debug [H][W][4]
    Pinned<void> h_stage;          // copy_out's and de_fetch_image_view's staging (a pageable destination copies at a fraction of the link rate): W * H * 3 floats, or the output size's when that is larger
    // de_fetch_image_begin / _end: the window loop pipelined — display + device-to-host copy of frame k run on the context stream while launch k + 1 renders (de_fetch.h).
    FetchRing img = {"image", "de_fetch_image"};
    Dev<uint32_t> d_tiles;
    int n_tiles = 0, tiles_rank = -1, tiles_world = -1;
    Dev<unsigned long long> d_counters;
    Dev<uint32_t> d_work_counter;   // 16 dwords per launch slot
    Dev<float> d_dens_table;   // get_density by altitude index (DE_DENS_TABLE_N x 3)
    int n_cus = 256;
    bool count = false;
    de_counters counters;
    int current_spp = 0;
    int sample_rank = 0, sample_world = 1;   // de_set_sample_partition: of the frame's sample indices this context renders those = rank (mod world)
    Dev<float> d_assembled;   // root's receive buffer of de_reduce_progressive ([H][W][3])
    Dev<float> d_gather;      // root of de_reduce_ordered: the other ranks' buffers, [world][H][W][3]
    int gather_world = 0;
    const float* display_src = nullptr;   // a view: what the display transform / de_fetch_hdr read instead of d_hdr (de_set_display_source)
    hipEvent_t ev_r0 = nullptr, ev_r1 = nullptr;   // around the last collective
    bool reduce_timing_valid = false;
    void* comm = nullptr;        // the context's own RCCL communicator (de_comm_init)
    int comm_rank = 0, comm_world = 1;
    bool trace = false;          // env DE_AUTO_TRACE, read once in de_create: print what the launch policy measured and chose
    int kernel_variant = 4;      // 4 = automatic (default): large launches run the first vertex rounds in the wavefront pipeline and finish in the state machine, small ones run the state machine alone; 1 = per-lane loops (legacy/render_kernel_v1.hip), 2 = wave-level state machine (render_kernel_v2.hip), 3 = wavefront pipeline through HBM queues (render_kernel_v3.hip)
    // render_kernel_v6 (kernel variant 6): one persistent launch per call, one workgroup per CU, stage queues in LDS.  Per launch slot:
    // the control words, one cold record per record slot of every workgroup, the launch's RenderArgs.
    struct V6State {
        Dev<wf::Cold> cold;
        Dev<uint32_t> ctl;
        Dev<RenderArgs> d_args;
        Pinned<uint32_t> h_status;     // pinned, device-visible: the kernel's abort code
        uint32_t n_wg = 0;
        Dev<uint4> pool[2];      // the tail's pools (render_kernel_v6.hip: "The tail"): level k exports to pool[k & 1]
        uint32_t pool_cap[2] = {0, 0};            // entries
    } v6s[DE_MAX_SLOTS];
    int v6_tail_levels = 1, v6_tail_export[2] = {128, 96}, v6_tail_grid[2] = {64, 8};
    uint32_t v6_tail_min_paths = 4u << 20;
    int v6_tail_when_alone = 0;      // 1: export even when no launch is queued behind (tests; default: only then, see render_kernel_v6.hip schedule())
    Pinned<uint32_t> h_issued;    // pinned, device-visible: the number of the newest render_kernel_v6 launch with a successor on another launch slot (read once per workgroup)
    uint32_t v6_launch_seq = 0;
    int v6_bands = 8;                // work counters of a launch: 8 = one band of the image per XCD, 1 = one for the whole launch (render_kernel_v6.hip: run_primary)
    int v6_stats = 0;                // 1: the instrumented kernel (env DE_V6_STATS; de_debug_v6_stats)
    int v6_svc[3] = {24, 24, 20};    // idle lanes at which a loop stage services (env DE_V6_SVC_ST / _GAS / _CLOUD)
    int v6_svc_area[3] = {100, 72, 90};  // idle lane-trips since its last service at which a loop stage services (sphere trace, gas, cloud; 0 = the idle-lane threshold above): render_kernel_v6.hip run_loop
    int v6_yield = 56, v6_elsewhere = 48, v6_retry = 6, v6_enter_min = 0, v6_flat_min = 0, v6_flat_again = 32;      // render_kernel_v6.hip: bs::Args (env DE_V6_YIELD / _ELSEWHERE / _RETRY / _ENTER_MIN)
    int launch_variant = 2;          // variant of the sub-launch being issued
    int launch_pipe = 0;             // v3 pipe of the sub-launch being issued
    int launch_slot = 0;             // launch slot of the sub-launch being issued
    bool launch_one_batch = false;   // the call being issued is one batch on one pipe (calls in flight)
    int last_call[4] = {0, 0, 0, 0}; // what the last de_accumulate ran: variant, pipes, pipeline rounds, launches (de_last_call_info)
    int launch_pipes = 1;            // pipes the call being issued runs side by side
    int launch_depths = 25, launch_wpc = 14;   // pipeline settings of the call being issued
    int auto_v6 = 1;                 // 1: the automatic variant runs calls of at least auto_v6_min_items paths on the per-CU stage scheduler (env DE_AUTO_V6)
    unsigned long long auto_v6_min_items = 1ull << 12;      // (env DE_AUTO_V6_MIN_ITEMS; 32 768 paths per call: 4.9 against 8.4 ms per frame of the window loop, 0.74 against 1.21 ms per call back to back — tools/small_calls.py)
    size_t mem_budget = 0;           // de_set_memory_budget (binds the legacy pipeline's queues; the product's kernels hold 37 MB per launch slot)
#ifdef DE_LEGACY_VARIANTS
#include "legacy/de_ctx_legacy_members.inc"
#endif
    // What started the current frame (cleared by de_reset): de_accumulate / de_upload_hdr, or de_accumulate_adaptive — the two do not mix.
    int frame_kind = 0;          // DE_FRAME_*
    // Adaptive frame (de_accumulate_adaptive).  Allocated on first use: S2 12 B per pixel, two active lists, the tile counts and the keep flags 4 B per tile.
    Dev<float> d_s2;           // [H][W][3] per-pixel sums of squares, accumulated by accumulate_moments_kernel
    Dev<uint32_t> d_alist[2];   // active tile lists, ascending; a round's launches read alist[ad_cur], its compaction writes the other one
    Dev<int32_t> d_tile_spp;   // [H/8][W/8] samples per tile (the per-tile display reads it)
    Dev<uint32_t> d_keep;      // [active] flags of the convergence test
    Dev<int32_t> d_ad_count;   // tiles still active after the compaction ...
    Pinned<int32_t> h_ad_count;   // ... and its pinned host copy: the host sizes the next round's launch with it
    int ad_cur = 0, ad_active = 0, ad_n = 0, ad_rounds = 0;      // list in use, tiles active, samples of every active tile, rounds so far
    unsigned long long ad_pixel_samples = 0;
    uint64_t ad_seed = 0;
    float ad_threshold = 0.f, ad_floor = 0.f;
    int ad_min = 0, ad_max = 0, ad_round = 0;
    // Denoiser (include/digital_earth_denoise.h).  Allocated on first use: guides 36 B per pixel, two (colour, variance) buffers 32 B, the
    // filtered mean 12 B.  S2 (d_s2 above) doubles as the temporal variance source of uniform frames.
    bool dn_on = false;
    int dn_levels = 5;
    float dn_sigma_l = 4.0f;
    bool dn_s2_complete = false;    // every sample of the current frame went through accumulate_moments_kernel since the denoiser was on at its start
    bool dn_guides_valid = false;   // the guides belong to the current camera, maps and address mode (cleared by de_reset, map changes, camera changes)
    bool dn_out_valid = false;      // d_dn_out holds the filtered mean of the frame as last displayed
    Dev<float4> d_dn_nc;      // [H][W] (normal, coverage)
    Dev<float4> d_dn_at;      // [H][W] (albedo, cloud transmittance)
    Dev<float> d_dn_dist;     // [H][W]
    Dev<float4> d_dn_buf[2];   // [H][W] (colour, variance): the levels alternate
    Dev<float> d_dn_out;      // [H][W][3] the filtered mean: what the display reads with samples = 1
    // Auto-exposure (include/digital_earth_exposure.h).  Allocated on first use: the workgroups' partial histograms (528 KB), the bins' centres,
    // the adaptation state, the second FrameConsts and the result block.  Per context: a context that borrows its maps meters for itself.
    bool ae_on = false;
    bool ae_displayed = false;      // a display has been enqueued since the feature was turned on (de_get_metering answers)
    de_auto_exposure ae;            // the settings
    Dev<uint32_t> d_ae_partial;   // [AE_MAX_WG][AE_ROW]
    Dev<double> d_ae_centre;      // [AE_BINS]
    Dev<MeterState> d_ae_state;   // previous EV: survives de_reset, cleared by de_set_auto_exposure
    Dev<FrameConsts> d_fc_ae;     // *d_fc with the metered exposure_scale: what the display reads (d_fc itself is never written: render launches in flight read it)
    Dev<MeterResult> d_ae_result;
    // Bloom (include/digital_earth_bloom.h).  Allocated on first use: the pyramid (the levels D_1 .. D_L and U_1 .. U_{L-1} of the largest L the
    // image admits, float4: 22 MB at 1080p) and the composited mean that the display reads with samples = 1 (25 MB at 1080p).  Per context.
    bool bl_on = false;
    de_bloom bl;                    // the settings
    Dev<float4> d_bl_pyr;
    Dev<float> d_bl_out;      // [H][W][3]
    // History reprojection (include/digital_earth_history.h).  Allocated on first use: the history and the candidate (a float4 and an f32 per
    // pixel each, and a camera) and the blended mean that the display reads with samples = 1: 2 x (16 + 4) + 12 bytes per pixel (108 MB at 1080p).  Per context.
    bool hs_on = false;
    bool hs_valid = false;          // the history holds a displayed picture (cleared by everything that drops it)
    bool hs_cand_valid = false;     // the candidate was written by a display since the last swap: the next de_reset makes it the history
    de_history hs;                  // the settings
    Dev<float4> d_hs_c[2];       // [H][W] (rgb, weight): [hs_cur] the history, [hs_cur ^ 1] the candidate
    Dev<float> d_hs_d[2];        // [H][W] land distance
    Dev<HistoryCam> d_hs_cam[2];
    int hs_cur = 0;
    Dev<float> d_hs_out;      // [H][W][3]
    // 8-bit pixel output (include/digital_earth_pixels.h).  Allocated on first use, each for 4 channels so that de_set_pixels never frees a
    // buffer a caller may still read: W * H * 4 bytes on the device, and as much pinned for the staging buffer and per ring cell (W * H * channels of each
    // in use).  The ring is independent of the float image's.
    de_pixels px = {(uint32_t)sizeof(de_pixels), 4, DE_PIXELS_TRUNCATE, 0u, 0};      // the settings
    PackedOut px_out = {"pixel"};   // [H][W][channels]
    FetchRing px_ring = {"pixel", "de_fetch_pixels"};
    // Local exposure (include/digital_earth_local_exposure.h).  Allocated on first use: the float2 pyramid D_1 .. D_L (l w, w) and the f32
    // bases B_1 .. B_{L-1} of the largest L the image admits (5.5 + 2.8 MB at 1080p) and the dodged mean that the display reads with samples = 1 (25 MB
    // at 1080p).  Per context.
    bool lx_on = false;
    de_local_exposure lx;           // the settings
    Dev<float2> d_lx_pyr;
    Dev<float> d_lx_base;
    Dev<float> d_lx_out;      // [H][W][3]
    // Output scaling (include/digital_earth_output_scale.h).  Allocated on first use: the tables of the two axes (first[n_dst] and
    // w[taps][n_dst] each), the intermediate (W, oh, 3) and the output (ow, oh, 3); re-allocated when a new size needs more.  Per context.
    de_output_scale os = {(uint32_t)sizeof(de_output_scale), 0, 0, 0, DE_SCALE_LANCZOS3};      // the settings; width = height = 0 until the first set: W, H
    struct ScaleDev {               // one axis' table on the device, and what it was built for
        Dev<int32_t> first; Dev<float> w;   // first[n_dst], w[taps][n_dst]
        int n_src = 0, n_dst = 0, filter = -1, taps = 0;
    } os_tab[2];                    // [0] along v, [1] along u
    Dev<float> os_mid, os_out;
    // Panorama output (include/digital_earth_panorama.h).  Allocated by the first de_set_panorama that succeeds: six face slots of N x N x 3
    // floats in one buffer and the output (width, height, 3); the equirect's four tables on first use, rebuilt when the size or S changes.  Per context.
    de_panorama pano = {(uint32_t)sizeof(de_panorama), 0, DE_PANO_EQUIRECT, 0, 0, 180.0f, 1, 2, {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}};
    uint32_t pano_mask = 0;         // bit k: slot k holds a face (cleared by de_set_panorama alone)
    PanoArgs pano_consts = {};      // of `pano`: fov, scale, half_aperture, m — once per de_set_panorama; the pointers are filled at the launch
    Dev<float> pano_faces, pano_out;
    struct PanoTab { Dev<float> t[4]; int width = 0, height = 0, S = 0; } pano_tab;      // sin lon, cos lon, sin lat, cos lat
    // Scene-linear panorama (include/digital_earth_environment.h).  Allocated by the first de_environment_capture that succeeds: six
    // linear face slots of N x N x 3 floats in one buffer; the row-major image [height][width][3] by the first EXR conversion of the panorama.  The
    // settings are `pano` and `ex`; the equirect's tables are pano_tab.
    uint32_t env_mask = 0;          // bit k: linear slot k holds a face (cleared by de_set_panorama alone)
    Dev<float> env_faces, env_out;
    // IBL output (include/digital_earth_ibl.h).  Everything reaches the device by the first de_ibl_build that succeeds: the mip chain
    // (level 0 is the base level), the specular levels 1 ... L - 1, the levels' sample tables, the solid angles, the SH partials and result, the DDS payload.
    struct IblWork {
        Dev<float> mips, spec, omega, partial, sh; Dev<IblSample> tab; Dev<uint8_t> payload;
        Dev<uint8_t> bc6h;      // the BC6H blocks of the chain (digital_earth_ibl_bc6h.h): empty until the first de_fetch_ibl_bc6h_dds after a build
    };
    de_ibl ibl = {(uint32_t)sizeof(de_ibl), 128, 6, 256, 2, 0.0f, DE_EXR_PIXEL_HALF};
    bool ibl_built = false;         // ibl_work holds the product of `ibl` (dropped by de_set_ibl)
    IblWork ibl_work;
    de_ibl_bc6h ibl_bc6h = {(uint32_t)sizeof(de_ibl_bc6h), 0, 0};      // include/digital_earth_ibl_bc6h.h, DESIGN.md §29
    bool ibl_bc6h_made = false;     // ibl_work.bc6h holds the blocks of the product and of `ibl_bc6h` (dropped by de_ibl_build, de_set_ibl, de_set_ibl_bc6h)
    // HDR display output (include/digital_earth_hdr_output.h).  The constants of the settings are computed by de_set_hdr_output and travel in
    // the kernel's arguments.  Allocated on first use: the packed pixels on the device and one pinned staging buffer, each out_w * out_h * 6 bytes (either
    // format fits: de_set_hdr_output frees nothing); re-allocated when a new output size needs more.  No ring.
    de_hdr_output ho = {(uint32_t)sizeof(de_hdr_output), 0, 1000.0f, DE_HDR_GAMUT_REC2020, DE_HDR_TRANSFER_PQ, DE_HDR_PIXELS_RGB10A2, DE_PIXELS_TRUNCATE, 0u, 0};
    HdrConsts ho_consts = {};       // of `ho`; valid while ho.on
    PackedOut hpx_out = {"HDR pixel"};
    // Video frame output (include/digital_earth_video.h).  The constants of the settings are computed by de_set_video and travel in the
    // kernel's arguments.  Allocated on first use, each for the 10-bit formats (out_w * out_h * 3 bytes) so that de_set_video never frees a buffer a caller
    // may still read: the frame on the device, one pinned staging buffer and four pinned ring cells.  The ring is independent of the other two.
    de_video vd = {(uint32_t)sizeof(de_video), DE_VIDEO_NV12, DE_VIDEO_MATRIX_BT709, DE_VIDEO_RANGE_LIMITED, DE_VIDEO_SITING_LEFT, DE_PIXELS_ROUND, 0u, 0};
    VideoConsts vd_consts = vd_make_consts(DE_VIDEO_NV12, DE_VIDEO_MATRIX_BT709, DE_VIDEO_RANGE_LIMITED);      // of `vd`: once per de_set_video
    PackedOut vd_out = {"video"};
    FetchRing vd_ring = {"video", "de_fetch_videoframe"};
    // Look LUTs (include/digital_earth_look.h): the settings as de_set_look took them (lk_on = lk.enabled) and their tables on the
    // device.  de_set_look uploads into fresh buffers and swaps: a refused or failed call leaves these as they were.
    struct LookDev {              // the tables of one look and the constants of their axes
        Dev<float> t1;      // [size_1d][3]
        Dev<float4> t3;     // [size_3d]^3, one float4 per lattice point
        LookAxis a1[3] = {}, a3[3] = {};
    };
    bool lk_on = false;
    de_look lk = {};
    LookDev lk_dev;
    // JPEG output (include/digital_earth_jpeg.h).  The tables of the settings are computed by de_set_jpeg on the host; they, the framing and
    // every buffer reach the device on first use: the planes, coefficients, masks and interval slots of one conversion (JpegWork) and the streams of
    // jp_coded, each with the generation of the framing in it beside it (jp_gen when it was written: jp_out_framed, jp_cell_framed).
    struct JpegWork {             // what one conversion passes through; re-allocated when a frame needs more
        Dev<uint8_t> planes; Dev<int16_t> coef; Dev<unsigned long long> mask; Dev<uint8_t> slots; Dev<uint32_t> words; Dev<JpegTables> tab;
    };
    de_jpeg jp = {(uint32_t)sizeof(de_jpeg), 90, DE_JPEG_DEFAULT_RESTART};
    JpegTables jp_tab = {};         // of jp.quality: once per de_set_jpeg (and in de_create's stead on first use: jp_tab_gen = 0)
    uint64_t jp_gen = 1, jp_tab_gen = 0, jp_tab_uploaded = 0;      // jp_gen: counts de_set_jpeg and changes of the output size
    int jp_w = 0, jp_h = 0;         // the size the framing was written for
    uint8_t jp_framing[JP_FRAMING_BYTES] = {};
    JpegWork jp_work;
    CodedOut jp_coded = {{"JPEG"}, {"JPEG", "de_fetch_jpeg"}};
    uint64_t jp_out_framed = 0, jp_cell_framed[DE_FETCH_RING] = {};
    // PNG output (include/digital_earth_png.h).  Everything reaches the device on first use: the packed pixels, the filtered stream, the
    // chunks' slots and words of one conversion (PngWork) and the files of pn_coded.  The front travels in the kernels' arguments: no copy of it is tracked.
    struct PngWork {              // what one conversion passes through; re-allocated when a frame needs more
        Dev<uint8_t> pixels, filtered, slots; Dev<uint32_t> words; Dev<PngTables> tab;
        bool tab_uploaded = false;
    };
    de_png pn = {(uint32_t)sizeof(de_png), DE_PNG_SOURCE_PIXELS, DE_PNG_FILTER_ADAPTIVE, DE_PNG_DEFAULT_CHUNK};
    PngWork pn_work;
    CodedOut pn_coded = {{"PNG"}, {"PNG", "de_fetch_png"}};
    // OpenEXR output (include/digital_earth_exr.h).  Everything reaches the device on first use: the framed raw blocks, the predicted
    // bytes, the chunks' slots and words of one conversion (ExrWork) and the files of ex_coded.  The front travels in the kernels' arguments.
    struct ExrWork {              // what one conversion passes through; re-allocated when a frame needs more
        Dev<uint8_t> raw, pred, slots; Dev<uint32_t> words; Dev<PngTables> tab;
        bool tab_uploaded = false;
    };
    de_exr ex = {(uint32_t)sizeof(de_exr), DE_EXR_SOURCE_MEAN, DE_EXR_PIXEL_HALF, DE_EXR_COMPRESSION_ZIP, DE_EXR_DEFAULT_CHUNK, 1.0f};
    uint32_t ex_aovs = 0;         // DE_EXR_AOV_* (include/digital_earth_exr_aovs.h): the channels beside B, G, R; 0: none, the file of §23
    ExrWork ex_work;
    CodedOut ex_coded = {{"EXR"}, {"EXR", "de_fetch_exr"}};
    // Radiance HDR output (include/digital_earth_rgbe.h).  Everything reaches the device on first use: the planar bytes, the planes'
    // slots and words of one conversion (RgbeWork) and the files of rg_coded.  The front travels in the kernels' arguments.
    struct RgbeWork {             // what one conversion passes through; re-allocated when a frame needs more
        Dev<uint8_t> planes, slots; Dev<uint32_t> words;
    };
    de_rgbe rg = {(uint32_t)sizeof(de_rgbe), DE_EXR_SOURCE_MEAN, 1, DE_RGBE_ROUND_TRUNC, 1.0f};
    RgbeWork rg_work;
    CodedOut rg_coded = {{"RGBE"}, {"RGBE", "de_fetch_rgbe"}};
    bool frame_invalid = false;  // a persistent launch left on its abort word since the last de_reset: every fetch / reduce / synchronize reports it until then
    std::string invalid_msg;
    de_ctx* lender = nullptr;    // the context whose maps and LUTs this one reads (de_share_textures)
    int loans = 0;               // contexts currently reading THIS context's maps: while > 0 they may not be freed or repacked
};

/* digital_earth_history.h — opt-in history reprojection of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * Every camera move ends in de_reset, which throws the picture away; the next frames start again at one sample per pixel.  With the feature on,
 * every display entry point (de_fetch_image, de_fetch_image_view, de_fetch_image_begin, de_render_to_image) keeps what it showed — the HDR mean, a
 * weight in samples, the first-hit land distance and the camera — and after a de_reset the next displays find, for every pixel, where its world
 * point was in that picture (four bilinear taps, refused across depth edges) and blend it with the new frame's mean by sample count:
 * out = (mean n + history w) / (n + w).  As n grows the history fades on its own; `max_history` bounds w.  The result goes through the unchanged
 * display transform.  Everything runs on the GPU and on the context stream: no host round trip, and de_fetch_image_begin / _end keep their overlap.
 *
 * The stage reads exactly what the display reads — the accumulation buffer with the frame's or the tiles' sample counts, the denoiser's filtered
 * mean, or a display source — and runs after the denoiser and before the meter and the bloom, which then see the stabilised image.  The HDR sums,
 * the sample counts and the sample indices are never modified; while the feature is off every entry point behaves exactly as without this header.
 *
 * The history is dropped by de_set_history, by a map or LUT upload and by a change of any de_params field that changes radiance (sun_angle,
 * sun_path_rot, land_height_scale, fixed_wavelength, topo_res_override, the flags other than DE_FLAG_AGX).  Camera fields reproject; display-only
 * fields (exposure, gamma, CRF, vignette, DE_FLAG_AGX) keep it.  It needs the maps and the LUTs (the distance comes from the denoiser's guide
 * kernel; the denoiser need not be on): DE_ERR_STATE before they are set.
 */
#ifndef DIGITAL_EARTH_HISTORY_H
#define DIGITAL_EARTH_HISTORY_H
#include "digital_earth.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct de_history {
    uint32_t struct_bytes;               /* sizeof(de_history) of the caller; checked like de_tuning */
    float max_history;                   /* > 0, samples; the largest weight a reprojected pixel may carry; default 32 */
    float depth_tolerance;               /* (0, 1]; a tap is refused when its land distance differs from the reprojected one by more than this fraction; default 0.02 */
} de_history;

/* Turn history reprojection on with these settings, or off with NULL.  Every call drops the history.  DE_ERR_INVALID: a bad value, a NaN, or a
 * mismatched struct_bytes. */
int de_set_history(de_ctx* ctx, const de_history* settings);
/* The current settings; max_history = 0 while the feature is off. */
int de_get_history(de_ctx* ctx, de_history* out);
/* The blended HDR mean (what the display transform is given) and its weight in samples, (W, H, 4) floats in de_fetch_hdr's layout; a mean, not a
 * sum.  Runs the denoiser first when it is on.  Counts as a display: the picture it fetches is what the next de_reset keeps.  DE_ERR_STATE while
 * the feature is off, before the maps and LUTs are set, and wherever the denoiser refuses. */
int de_fetch_history_hdr(de_ctx* ctx, float* out);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_HISTORY_H */

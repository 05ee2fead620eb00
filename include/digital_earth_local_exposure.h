/* digital_earth_local_exposure.h — opt-in local exposure of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * The sunlit limb, the ocean glint and the cloud tops of a frame from orbit sit several stops above the twilight side of the same picture: no single
 * exposure is right for both.  A person printing such a negative would dodge and burn.  With the feature on, every display entry point
 * (de_fetch_image, de_fetch_image_view, de_fetch_image_begin, de_render_to_image, and the pixel fetches behind them) first multiplies every pixel of
 * the HDR mean by a gain 2^ev, ev = -strength (B - mid) clamped to +-max_ev: B is a smooth BASE of log2 luminance that stops at edges (an image
 * pyramid brought back up by joint-bilateral upsampling, `sigma` stops wide in range), mid is the scene luminance that the display about to run maps
 * to `key`, and strength is `highlights` where the base is above mid and `shadows` below.  The gain depends on the base only, so the detail inside a
 * region keeps its contrast and all three channels get the same gain.  Pixels whose luminance is not in [2^-24, FLT_MAX] — black space, negatives,
 * NaN, Inf — weigh nothing and pass unchanged.  The result goes through the unchanged display transform.  Everything runs on the GPU and on the
 * context stream: there is no host round trip, and de_fetch_image_begin / _end keep their overlap.
 *
 * The stage is the last one before the display: the scene is metered, the lens glares, the print is dodged.  It reads exactly what the display
 * reads at that point — the accumulation buffer with the frame's or the tiles' sample counts, the denoiser's filtered mean, a display source, the
 * blended history, the bloom's composite — and the exposure the display is about to use (the metered one while auto-exposure is on), so it works
 * under every partition on the rank that displays; a rank's partial frame is dodged as the partial frame it is.  The HDR sums are never modified;
 * while the feature is off every entry point behaves exactly as without this header.
 */
#ifndef DIGITAL_EARTH_LOCAL_EXPOSURE_H
#define DIGITAL_EARTH_LOCAL_EXPOSURE_H
#include "digital_earth.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct de_local_exposure {
    uint32_t struct_bytes;               /* sizeof(de_local_exposure) of the caller; checked like de_tuning */
    int32_t on;                          /* 0: turn the feature off (the other fields are not read); de_get_local_exposure answers 0 while it is off */
    float highlights;                    /* [0, 1]; the fraction of the base's distance above the anchor that is taken back; default 0.5 */
    float shadows;                       /* [0, 1]; the same below the anchor; default 0.25 */
    float sigma;                         /* > 0; range width of the edge-stopping weights in stops; very large: not edge-aware; default 1.0 */
    float max_ev;                        /* >= 0; bound of the correction in stops; default 2.0 */
    float key;                           /* > 0; the displayed value of the anchor, as auto-exposure's key; default 0.18 */
    int32_t levels;                      /* 1 .. 10; pyramid levels, reduced so that no level's smaller side is below 2; default 6 */
} de_local_exposure;

/* Turn local exposure on with these settings, or off with NULL (or on = 0).  DE_ERR_INVALID: a bad value, a NaN, or a mismatched struct_bytes. */
int de_set_local_exposure(de_ctx* ctx, const de_local_exposure* settings);
/* The current settings; on = 0 (and every setting 0) while the feature is off. */
int de_get_local_exposure(de_ctx* ctx, de_local_exposure* out);
/* The dodged HDR mean (what the display transform is given), (W, H, 3) floats in de_fetch_hdr's layout; a mean, not a sum.  Runs the display chain up
 * to and including this stage — the denoiser, the history blend, the meter (it counts as a display for the meter's adaptation) and the bloom, each
 * when it is on.  DE_ERR_STATE while local exposure is off, before the LUTs are uploaded, and wherever a stage ahead refuses. */
int de_fetch_local_exposure_hdr(de_ctx* ctx, float* out);
/* A test hook: the stage once on a host-given mean, (W, H, 3) floats in de_fetch_hdr's layout and of the context's size, with the anchor taken from
 * `exposure_scale` (the display's 2^exposure) and the given settings (`on` is not read); `out` receives the dodged mean in the same layout.  The
 * context's settings, frame and exposure are not touched. */
int de_debug_local_exposure(de_ctx* ctx, const float* mean, float exposure_scale, const de_local_exposure* settings, float* out);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_LOCAL_EXPOSURE_H */

/* digital_earth_exposure.h — opt-in auto-exposure of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * A headless sequence has nobody at the exposure slider.  With the feature on, every display entry point (de_fetch_image, de_fetch_image_view,
 * de_fetch_image_begin, de_render_to_image) first METERS what it is about to show, on the GPU and on the context stream: a 256-bin histogram of
 * the log2 luminance of the HDR mean (8 bins per octave over [2^-24, 2^8)), a trimmed mean of it between two percentiles, and from that an
 * exposure in EV that maps the retained mean to `key`.  The exposure is handed to the unchanged display transform through a second,
 * device-resident copy of the frame constants: there is no host round trip, and de_fetch_image_begin / _end keep their overlap.
 *
 * The meter reads exactly what the display reads — the accumulation buffer with the frame's or the tiles' sample counts, the denoiser's filtered
 * mean, or a display source — so it works under every partition on the rank that displays.  de_params.exposure is never modified; while the
 * feature is off every entry point behaves exactly as without this header, and turning it off restores the manual exposure's image.
 */
#ifndef DIGITAL_EARTH_EXPOSURE_H
#define DIGITAL_EARTH_EXPOSURE_H
#include "digital_earth.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct de_auto_exposure {
    uint32_t struct_bytes;               /* sizeof(de_auto_exposure) of the caller; checked like de_tuning */
    float key;                           /* > 0; luminance that the retained mean is mapped to; default 0.18 */
    float compensation;                  /* EV added to the target; default 0 */
    float ev_min, ev_max;                /* ev_min <= ev_max; defaults -8, 16 */
    float low_fraction, high_fraction;   /* 0 <= low < high <= 1, low < 1; defaults 0.10, 0.95: the metered pixels between these percentiles are retained */
    float adapt;                         /* (0, 1]; ev = prev + adapt (target - prev); 1 = jump to the target (default) */
    int32_t region[4];                   /* x0, y0, x1, y1, half-open, in the display's pixel (i, j); all 0 = the whole image */
} de_auto_exposure;

/* Turn auto-exposure on with these settings, or off with NULL.  Every call clears the adaptation state: the first display after it jumps to its
 * target.  de_reset does NOT clear it (adaptation across camera moves is the point).  DE_ERR_INVALID: a bad value, a region outside the image,
 * an empty region, or a mismatched struct_bytes. */
int de_set_auto_exposure(de_ctx* ctx, const de_auto_exposure* settings);
/* The current settings; key = 0 while the feature is off. */
int de_get_auto_exposure(de_ctx* ctx, de_auto_exposure* out);

typedef struct de_metering {
    uint32_t struct_bytes;               /* sizeof(de_metering) of the caller */
    float ev, ev_target, mean_log2;      /* the exposure used, its target before adaptation, the trimmed mean of log2 luminance */
    uint32_t valid;                      /* 0: no pixel was metered (an all-black frame): ev kept its previous value (the manual exposure when there is none) */
    uint64_t metered, below, clipped;    /* pixels of the region in the histogram; below 2^-24 (or negative, or NaN: not metered); at or above 2^8 (in bin 255) */
    uint32_t histogram[256];
} de_metering;

/* The metering of the newest display enqueued; waits for the context stream.  DE_ERR_STATE while the feature is off or before the first display
 * since it was turned on. */
int de_get_metering(de_ctx* ctx, de_metering* out);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_EXPOSURE_H */

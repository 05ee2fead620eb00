/* digital_earth_bloom.h — opt-in bloom of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * The sun disk, the ocean glint and the sunlit limb sit several stops above the rest of a frame from orbit; a lens spreads a little of that light
 * over its surroundings.  With the feature on, every display entry point (de_fetch_image, de_fetch_image_view, de_fetch_image_begin,
 * de_render_to_image) first takes a fraction `intensity` of the light above `threshold` from every pixel of the HDR mean and gives it back through
 * a wide, normalised point-spread function built as an image pyramid.  Every output's weights sum to 1, so a constant image stays constant.  Energy
 * (every input's total weight over all outputs) is conserved exactly while every pyramid level that is halved has even sides; a level of odd size
 * counts its last row or column twice, so light near the right and bottom borders is returned in excess and the rest of the frame loses a little
 * (measured at 1920x1080, whose rows halve to 135, with the default six levels and spread 0.7: up to +18 % for the bottom row, at most -4 % anywhere;
 * DESIGN.md §12 has the figures).  With threshold = 0 this is plain veiling glare:
 * out = (1 - intensity) mean + intensity PSF * mean.  The result goes through the unchanged display transform.  Everything runs on the GPU and on
 * the context stream: there is no host round trip, and de_fetch_image_begin / _end keep their overlap.
 *
 * The bloom reads exactly what the display reads — the accumulation buffer with the frame's or the tiles' sample counts, the denoiser's filtered
 * mean, or a display source — so it works under every partition on the rank that displays.  Auto-exposure (digital_earth_exposure.h) meters the
 * image before the bloom: the scene is metered, not the lens.  The HDR sums are never modified; while the feature is off every entry point behaves
 * exactly as without this header.
 */
#ifndef DIGITAL_EARTH_BLOOM_H
#define DIGITAL_EARTH_BLOOM_H
#include "digital_earth.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct de_bloom {
    uint32_t struct_bytes;               /* sizeof(de_bloom) of the caller; checked like de_tuning */
    float intensity;                     /* [0, 1]; the fraction of the bright part that is spread; default 0.05 */
    float threshold;                     /* >= 0; luminance of the HDR mean above which light is spread; 0 (default): all of it, veiling glare */
    float knee;                          /* [0, 1]; soft knee around the threshold, as a fraction of it; default 0.5 */
    float clamp;                         /* >= 0; upper bound of the luminance a pixel may give; 0 (default): none */
    float spread;                        /* [0, 1]; weight of the next coarser level at every step up: larger is wider; default 0.7 */
    int32_t levels;                      /* 1 .. 10; pyramid levels, reduced so that no level's smaller side is below 2; default 6 */
} de_bloom;

/* Turn bloom on with these settings, or off with NULL.  DE_ERR_INVALID: a bad value, a NaN, or a mismatched struct_bytes. */
int de_set_bloom(de_ctx* ctx, const de_bloom* settings);
/* The current settings; levels = 0 while the feature is off. */
int de_get_bloom(de_ctx* ctx, de_bloom* out);
/* The composited HDR mean (what the display transform is given), (W, H, 3) floats in de_fetch_hdr's layout; a mean, not a sum.  Runs the denoiser
 * first when it is on.  DE_ERR_STATE while bloom is off, and wherever the denoiser refuses. */
int de_fetch_bloom_hdr(de_ctx* ctx, float* out);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_BLOOM_H */

/* digital_earth_denoise.h — the opt-in denoiser of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * An SVGF-style edge-avoiding a-trous wavelet filter runs on the GPU between the accumulation buffer and the display transform.  It filters the HDR
 * MEAN (S1 / n per pixel), guided by noise-free first-hit features ("guides") of four fixed sub-pixel primary rays per pixel, with a per-pixel
 * variance: from the sums of squares S2 when every sample of the frame was accumulated with them and the pixel has at least 4 samples, else the
 * 7x7 spatial variance of the luminance.  The display then runs the unchanged transform over the filtered mean with a sample count of 1.
 * While the denoiser is off every other entry point behaves exactly as without this header.
 *
 * With the denoiser on, every display entry point (de_fetch_image, de_fetch_image_view, de_fetch_image_begin, de_render_to_image) shows the
 * denoised image; they answer DE_ERR_STATE under a tile partition (tile_world > 1), a sample partition, a display source (de_set_display_source)
 * or after de_reduce_progressive.  The HDR sums (de_fetch_hdr) never change.
 */
#ifndef DIGITAL_EARTH_DENOISE_H
#define DIGITAL_EARTH_DENOISE_H
#include "digital_earth.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct de_denoise {
    uint32_t struct_bytes;     /* sizeof(de_denoise) of the caller; checked like de_tuning */
    int32_t levels;            /* a-trous levels, steps 1, 2, 4, ...: 1 .. 10 (default 5) */
    float sigma_luminance;     /* luminance edge-stopping scale, in standard deviations: > 0 (default 4) */
} de_denoise;

/* Turn the denoiser on with these settings, or off with NULL.  Turned on before the frame's first sample (right after de_reset), it makes
 * de_accumulate track S2 too; turned on mid-frame, the frame uses the spatial variance until the next de_reset.  DE_ERR_INVALID: a bad value or a
 * mismatched struct_bytes. */
int de_set_denoise(de_ctx* ctx, const de_denoise* settings);
/* The current settings; levels = 0 while the denoiser is off. */
int de_get_denoise(de_ctx* ctx, de_denoise* out);
/* The filtered mean as (W, H, 3) f32, de_fetch_hdr's layout.  DE_ERR_STATE while the denoiser is off (and where the display refuses). */
int de_fetch_denoised_hdr(de_ctx* ctx, float* out);
/* The guides as (W, H, 9) f32: coverage (fraction of the four rays that hit land), distance to the land hit in metres (mean over the hitting rays,
 * 0 when none hits), normal xyz (renormalised mean), surface albedo rgb (0 for a ray that misses), cloud transmittance.  Computed once per frame:
 * after de_reset, a map change or a camera / terrain-scale / address-mode change.  Also useful as AOVs for an external denoiser; the
 * denoiser need not be on.  DE_ERR_STATE before the maps and LUTs are set. */
int de_fetch_guides(de_ctx* ctx, float* out);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_DENOISE_H */

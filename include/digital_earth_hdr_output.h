/* digital_earth_hdr_output.h — opt-in HDR display output of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * The display transform the library runs by default is OpenDRT in the one configuration the reference runs: a 100-nit Rec.709 display, display-linear
 * light, then the camera response curve, gamma and the sRGB OETF.  The transform itself (OpenDRT v0.2.2, lib/OpenDRT.py:221-485) was written for HDR
 * delivery: it has a peak luminance Lp, P3-D65 and Rec.2020 display matrices and the ST 2084 (PQ) and HLG inverse EOTFs.  While this stage is on,
 * de_render_to_image runs it in its general form instead, per pixel:
 *     mean = sum / samples, vignette, exposure scale               exactly as the default display (renderer.py:349-355)
 *     Rec.709 -> XYZ -> display gamut                               two matrix products in sequence, each rounded (gamut: DE_HDR_GAMUT_*)
 *     hue angles, weighted norm, tonescale, flare, chroma compression, hue shift, chroma value      the body of openDR_transform, unchanged, with the
 *                                                                   tonescale constants of `peak_nits` (Lp) and the display scale of `transfer`
 *     min(clamp_max)                                                clamp_max = peak_nits / 100 (linear: display 1.0 is the peak), / 10000 (PQ), / 1000 (HLG)
 *     the inverse EOTF                                              none (DE_HDR_TRANSFER_LINEAR), eotf_pq(rgb, 1) or eotf_hlg(rgb, 1)
 * and stores the SIGNAL, nominally in [0, 1], into the displayed image, (W, H, 3) float32 in the reference's layout.  What is NOT applied in this mode:
 * the camera response LUT, `gamma` and the sRGB OETF — an SDR film curve defined on [0, 1] and an SDR encoding; de_params.selected_crf and
 * de_params.gamma have no effect while the stage is on.  The settings' constants are evaluated once per de_set_hdr_output on the host in double
 * precision and handed to the kernel in its arguments.  All device arithmetic is the library's deterministic f32 (arithmetic contract, digital_earth.h).
 *
 * Everything ahead of the transform is inherited untouched (adaptive per-tile counts, the denoiser, history, the meter's exposure, bloom, local
 * exposure, display sources), and so is everything behind it: output scaling resamples the signal, de_fetch_image* hand it out as floats, and
 * de_fetch_pixels* keep working on it (8 bits of PQ: legal, but coarse — about 4 codes per 1 % of luminance; use the formats below).
 * DE_FLAG_AGX is an SDR transform: de_render_to_image and everything built on it return DE_ERR_STATE while both are on.
 *
 * KNOWN LIMIT, kept from the reference: ONLY DE_HDR_GAMUT_REC709 IS COLORIMETRICALLY MEANINGFUL.  The reference multiplies `v @ m` (lib/OpenDRT.py:86-88),
 * a row vector times the matrices as written, so each of the two products is by the TRANSPOSE of the colorimetric matrix.  For Rec.709 the two
 * transposes cancel; for P3-D65 and Rec.2020 they do not: white (1, 1, 1) arrives in the display gamut as (0.661, 1.409, 0.920) and (0.333, 1.646, 0.989),
 * and 0.18 grey under the DEFAULT setting (1000 nits, Rec.2020, PQ) comes out as the signal (0.256, 0.383, 0.339) — every neutral strongly green.  This
 * library follows the reference's text and is pinned to it executed (tests/golden/ref_opendrt_hdr.npz); it does not repair it.  Until the reference
 * does, use DE_HDR_GAMUT_REC709 for a picture meant to be looked at (Rec.709 primaries in a PQ / HLG container are legal: cICP 1 / 16 or 1 / 18); the
 * other two gamuts reproduce what the reference computes and are NOT a correct BT.2020 / P3 feed for a panel.
 *
 * The corner cases of the reference's text are kept, not repaired: under HLG a pixel whose display-linear luminance is 0 gives 0 * pow(0, negative)
 * = NaN in every channel; the pack below maps NaN to code 0, as the 8-bit pack does.
 *
 * Pixels: de_render_to_hdr_pixels converts the displayed image — of the output size while output scaling is on — into rows top-down, the pixels of a
 * row contiguous (r = H - 1 - v, x = u), like digital_earth_pixels.h:
 *     DE_HDR_PIXELS_RGB10A2   one uint32 per pixel: R in bits 0-9, G in bits 10-19, B in bits 20-29, alpha = 3 in bits 30-31   (maxcode 1023)
 *     DE_HDR_PIXELS_RGB16     three uint16 per pixel, R G B, in the host's (little-endian) byte order                           (maxcode 65535)
 * Per value t, in f32:  cl = t > 0 ? (t < 1 ? t : 1) : 0   (NaN and -0.0 give 0),  s = cl * maxcode,  then DE_PIXELS_TRUNCATE / _ROUND / _DITHER
 * exactly as digital_earth_pixels.h states them with 255 replaced by maxcode, the dither from the same hash keyed by (seed, phase, pixel, channel):
 * code 0 and code maxcode stay exact in every mode.  The codes are full range.
 *
 * Out of scope: a pinned ring (_begin / _end) and a zero-copy view for these pixels.  de_fetch_hdr_pixels is synchronous.
 */
#ifndef DIGITAL_EARTH_HDR_OUTPUT_H
#define DIGITAL_EARTH_HDR_OUTPUT_H
#include "digital_earth.h"
#include "digital_earth_pixels.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_HDR_GAMUT_REC709 0            /* OpenDRT's Rec709 */
#define DE_HDR_GAMUT_P3D65 1             /* OpenDRT's P3D65 */
#define DE_HDR_GAMUT_REC2020 2           /* OpenDRT's Rec2020 */

#define DE_HDR_TRANSFER_LINEAR 0         /* OpenDRT's lin: display-linear light, 1.0 = peak_nits */
#define DE_HDR_TRANSFER_PQ 1             /* OpenDRT's pq: ST 2084, 1.0 = 10 000 nits */
#define DE_HDR_TRANSFER_HLG 2            /* OpenDRT's hlg: BT.2100 HLG, 1.0 = 1000 nits */

#define DE_HDR_PIXELS_RGB10A2 0
#define DE_HDR_PIXELS_RGB16 1

typedef struct de_hdr_output {
    uint32_t struct_bytes;               /* sizeof(de_hdr_output) of the caller; checked like de_tuning */
    int32_t on;                          /* 0 (default): the display is the SDR one, bit for bit */
    float peak_nits;                     /* OpenDRT's Lp, within [100, 10000]; default 1000 */
    int32_t gamut;                       /* DE_HDR_GAMUT_*; default DE_HDR_GAMUT_REC2020 (see KNOWN LIMIT above: only _REC709 is colorimetric) */
    int32_t transfer;                    /* DE_HDR_TRANSFER_*; default DE_HDR_TRANSFER_PQ */
    int32_t pixel_format;                /* DE_HDR_PIXELS_*; default DE_HDR_PIXELS_RGB10A2 */
    int32_t mode;                        /* DE_PIXELS_TRUNCATE (default), DE_PIXELS_ROUND or DE_PIXELS_DITHER */
    uint32_t seed;                       /* of the dither's hash; default 0 */
    int32_t animate;                     /* 0 (default): phase 0 always; otherwise the phase counts this context's HDR conversions */
} de_hdr_output;

/* Set the stage and reset the phase counter.  DE_ERR_INVALID: peak_nits outside [100, 10000] or not finite, an enum out of range, a mismatched
 * struct_bytes (checked whether `on` is set or not). */
int de_set_hdr_output(de_ctx* ctx, const de_hdr_output* settings);
/* The current settings (before any de_set_hdr_output: the defaults above) and, when last_phase is not NULL, the phase of the newest conversion. */
int de_get_hdr_output(de_ctx* ctx, de_hdr_output* out, uint32_t* last_phase);
/* de_render_to_image, then the conversion behind it on the context stream; the pixels stay on the device (valid until the next conversion).
 * DE_ERR_STATE while the stage is off. */
int de_render_to_hdr_pixels(de_ctx* ctx, const void** device_pixels);
/* The pixels of the frame as it stands into `out` (out_bytes >= width * height * 4 for RGB10A2, * 6 for RGB16, of the output size; else
 * DE_ERR_INVALID); mirrors de_fetch_pixels. */
int de_fetch_hdr_pixels(de_ctx* ctx, void* out, uint64_t out_bytes);
/* The transform alone on n colours (scene-linear Rec.709, already exposed): rgb and out are n x 3 floats.  `settings` as for de_set_hdr_output (its
 * `on` and pixel fields are not read); the context's own setting is not touched. */
int de_debug_hdr_transform(de_ctx* ctx, const float* rgb, uint64_t n, const de_hdr_output* settings, float* out);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_HDR_OUTPUT_H */

/* digital_earth_exr_aovs.h — opt-in AOV channels of the OpenEXR output of libdigitalearth_hip.so (same library, additions only).
 *
 * The file of digital_earth_exr.h holds the radiance as B, G, R.  A bit mask adds, in the SAME single-part scan-line file, what a compositor or an
 * external denoiser wants beside it, all of it already on the device: the noise-free first-hit guides (digital_earth_denoise.h), the variance of the
 * mean from the sums of squares S2 and the sample counts.  With the mask 0 — the state before any call below — every EXR entry
 * point returns the bytes, the capacity, the front length and the ring estimate it returns without this header.
 *
 * THE CHANNELS.
 *     bit  group           channels (EXR names)                         pixel type          source
 *       1  depth           Z                                            always FLOAT        the guide's distance in metres; 0 where no ray hits land
 *                                                                                           (`coverage` tells the two apart; no infinity is invented)
 *       2  normal          N.X, N.Y, N.Z                                the file's          the guide's normal
 *       4  albedo          albedo.R, albedo.G, albedo.B                 the file's          the guide's albedo
 *       8  coverage        coverage                                     the file's          the guide's land coverage
 *      16  transmittance   transmittance                                the file's          the guide's cloud transmittance
 *      32  variance        variance.R, variance.G, variance.B           always FLOAT        S1, S2 and n (THE VARIANCE)
 *      64  samples         samples                                      always FLOAT        n, the pixel's divisor, as that float32
 * Z is FLOAT because a HALF would clamp at 65504 m.  n is the divisor the radiance's mean uses for that pixel: the frame's sample count or, inside an
 * adaptive frame, the tile's own.  The guides, S2 and n are the FRAME's whatever de_exr.source is — a stage's mean has no guides or S2 of its own —,
 * and the variance's S1 is always the context's own sums, the buffer S2 was accumulated beside.
 * The guides lie on the device in the sums' row orientation and are turned top-down with them.
 *
 * THE ORDER.  The `channels` attribute and the planes of every line hold the channels sorted by name as bytes, which OpenEXR requires; uppercase sorts
 * before lowercase.  With everything on: B, G, N.X, N.Y, N.Z, R, Z, albedo.B, albedo.G, albedo.R, coverage, samples, transmittance, variance.B,
 * variance.G, variance.R.  One host function makes the order (csrc/exr_tables.h: exr_channel_list, a byte-wise insertion sort).
 *
 * THE SAMPLE of an AOV channel.  de_exr.scale multiplies the radiance only.  A channel at the file's pixel type goes through THE SAMPLE of
 * digital_earth_exr.h with scale 1 (a NaN +0; HALF clamps to +-65504, nearest even, subnormals kept).  A FLOAT channel stores its 32 bits, a NaN +0.
 *
 * THE VARIANCE of the mean, per colour channel, float32 at every step, no operation fused with another:
 *     n < 2 (or n a NaN):  0
 *     mean = S1 / n;  prod = S1 * mean;  d = S2 - prod;  q = d / (n - 1);  sv = q if q > 0 else 0 (so a NaN q gives 0);  variance = sv / n
 * sv is the sample variance max(0, (S2 - S1 mean) / (n - 1)) of DESIGN.md §10.  It needs S2 to hold every sample of the frame: the denoiser on since
 * before the frame's first sample, or an adaptive frame.  Otherwise every conversion answers DE_ERR_STATE, its message saying how to get S2 (turn the
 * denoiser on before the frame's first sample, or render adaptively), and no file is made.  A reduce (de_reduce, de_reduce_progressive,
 * de_reduce_ordered), an upload and a bound buffer mark S2 incomplete themselves.  Where the sums shown are not this context's own or S2 is only a
 * part's, the variance is refused as the denoiser is, with DE_ERR_STATE as well: while a display source is set (de_set_display_source, or the
 * assembled frame of de_reduce_progressive), under a tile partition and under a sample partition.  Only the variance group is refused there;
 * `samples` stays the divisor the radiance uses.  This output never changes when S2 is accumulated.
 *
 * THE FILE is digital_earth_exr.h's THE FILE with these changes, byte for byte (tests/exr_aov_ref.py restates it):
 *     the `channels` attribute lists the channels above in THE ORDER, each with its own pixel type; the front is 313 - 54 + sum(len(name) + 17) bytes
 *         (626 with everything on) and the offset table follows it;
 *     a line's raw bytes are, for each channel in THE ORDER, its W samples of bps bytes (2 HALF, 4 FLOAT): line_bytes = W sum(bps), a block's
 *         P = lines line_bytes; reorder, predictor, deflate chunks, raw fallback and offset table are unchanged;
 *     de_exr_capacity = front + 8 nb + 8 nb + H W sum(bps).
 * LIMIT: H W sum(bps) <= 2^27 (DE_ERR_INVALID otherwise) — the coded tail counts bytes in 32 bits.  Everything on is 42 bytes per pixel at HALF
 * (1920 x 1080 fits, 3840 x 2160 does not) and 64 at FLOAT (1920 x 1080 is just under the limit).
 * OUT OF SCOPE: multi-part, tiled and deep files, UINT channels, alpha, per-channel scale, AOVs on de_debug_exr, frames past the limit, S2 without
 * the denoiser or adaptive mode.
 */
#ifndef DIGITAL_EARTH_EXR_AOVS_H
#define DIGITAL_EARTH_EXR_AOVS_H
#include "digital_earth_exr.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_EXR_AOV_DEPTH 1
#define DE_EXR_AOV_NORMAL 2
#define DE_EXR_AOV_ALBEDO 4
#define DE_EXR_AOV_COVERAGE 8
#define DE_EXR_AOV_TRANSMITTANCE 16
#define DE_EXR_AOV_VARIANCE 32
#define DE_EXR_AOV_SAMPLES 64
#define DE_EXR_AOV_ALL 127

/* The channel groups of every later EXR conversion of this context.  DE_ERR_INVALID: an unknown bit, or the context's size passes the limit with this
 * mask at the current de_exr settings (de_set_exr checks the same against the mask in force); DE_ERR_STATE while EXR fetches are in flight.  A refused
 * call changes nothing. */
int de_set_exr_aovs(de_ctx* ctx, uint32_t mask);
/* The mask in force (before any de_set_exr_aovs: 0). */
int de_get_exr_aovs(de_ctx* ctx, uint32_t* mask);
/* The conversion once on host-given arrays, free of the display, with buffers of its own: `image` [H][W][3] float32 in R, G, B order is read as the
 * sums S1; `guides` [H][W][9] float32 in de_fetch_guides' order (coverage, distance, normal x y z, albedo r g b, transmittance); `s2` [H][W][3];
 * `counts` [H][W] float32, the divisor n of each pixel — of B, G, R too; where it is NULL they are divided by 1.  Rows top-down.  `guides`, `s2`
 * and `counts` may be NULL when no selected channel reads them (DE_ERR_INVALID otherwise).  settings->source is not read. */
int de_debug_exr_aovs(de_ctx* ctx, const float* image, const float* guides, const float* s2, const float* counts, int W, int H, const de_exr* settings, uint32_t mask, void* out, uint64_t out_bytes, uint64_t* len);
/* de_debug_exr_framing with a mask: the front of a W x H file, its offset table zeroed, and the capacity.  No device and no context. */
int de_debug_exr_aov_framing(const de_exr* settings, uint32_t mask, int W, int H, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_EXR_AOVS_H */

/* digital_earth_output_scale.h — opt-in output scaling of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * A context renders W x H and, without this header, delivers W x H.  While the stage below is on, everything that hands out the DISPLAYED image
 * — de_render_to_image, de_fetch_image, de_fetch_image_view, de_fetch_image_begin / _end, de_render_to_pixels and the de_fetch_pixels* calls —
 * delivers `width` x `height` instead (ow x oh below): the image that the unchanged display transform wrote, resampled on the GPU by a separable
 * polyphase filter, and, for the pixel calls, packed from the resampled image by the unchanged pack kernel.  The stage works on display-referred
 * values, the [0, 1] floats of de_fetch_image, as image and video scalers do.  Everything ahead of the display (the sums, the samples, denoiser,
 * history, meter, bloom, local exposure, the vignette) runs at W x H and knows nothing of the output size.  While the stage is off, the default,
 * every call returns exactly the bytes it returned before this header existed.  Layouts are unchanged: floats (ow, oh, 3) with the pixels of a
 * column contiguous, index (u oh + v) 3 + c; pixels [oh][ow][channels].
 *
 * THE FILTER, per axis (n_src samples in, n_dst out), in double precision on the host:
 *     r = n_src / n_dst,   s = max(r, 1),   a = the filter's support
 *     x_j = (j + 0.5) r - 0.5                              the centre of output sample j in source coordinates
 *     taps of j: the integers i with |i - x_j| < a s, ascending: first_j = floor(x_j - a s) + 1 ... ceil(x_j + a s) - 1
 *                (an empty set — the box filter enlarging, x_j exactly half-way between two samples — is the one tap floor(x_j + 0.5))
 *     weight of tap i: k((i - x_j) / s), then divided by the sum of the row's weights (added in tap order)
 *     k: DE_SCALE_BOX       1                                                        a = 0.5
 *        DE_SCALE_TRIANGLE  1 - |t|                                                  a = 1
 *        DE_SCALE_MITCHELL  (7 |t|^3 - 12 |t|^2 + 16/3) / 6           for |t| < 1,   a = 2      (B = C = 1/3)
 *                           (-7/3 |t|^3 + 12 |t|^2 - 20 |t| + 32/3) / 6  for 1 <= |t| < 2
 *        DE_SCALE_LANCZOS3  sinc(t) sinc(t / 3),  sinc(z) = sin(pi z) / (pi z), 1 at 0  a = 3
 * `first_j` is kept UNCLAMPED (it may be negative); a tap outside [0, n_src) reads the edge sample: its index is clamped when it is gathered.  The
 * rows of an axis are padded with zero weights behind their last tap to one tap count, the largest of the axis (at most 2 ceil(3 * 8) + 1 = 49).
 * The normalised weights are rounded to float32 and then CORRECTED so that the float32 weights of every row, added in tap order in float32 from
 * 0.0f, give exactly 1.0f: the row's LAST tap (ahead of the padding) is replaced by fl(1 - P), P the float32 sum of the taps before it, added in tap
 * order.  (P + fl(1 - P) differs from 1 by at most half an ulp of the correction, 2^-25, so the sum rounds to 1.0f; the library checks the sum again
 * and refuses the table otherwise.)  Hence black and a clipped white of 1.0 survive any scale exactly: 1.0 does not come out as 0.99999994 and
 * DE_PIXELS_TRUNCATE does not turn it into 254.
 *
 * THE ARITHMETIC, all float32: two passes with a float32 intermediate, along v first ((W, H, 3) -> (W, oh, 3)), then along u (-> (ow, oh, 3)).
 * Each value of a pass is   acc = 0.0f;  acc = acc + w[t] * src[t]   for t = 0 ... taps - 1 in ascending order, the padding included: a multiply,
 * then an add, never an fma.  An axis whose output size equals its source size is a COPY: no pass runs on it (Lanczos weights at ratio 1 are not
 * exactly a delta in floating point), so scaling to W x H is the identity, bit for bit, for every filter.  The LAST pass that runs clamps its result
 * as the pixel conversion does, t > 0 ? (t < 1 ? t : 1) : 0 (Mitchell and Lanczos overshoot; NaN and -0.0 give 0); when no pass runs nothing is
 * clamped.  tests/output_scale_ref.py restates all of this in numpy, and the GPU equals it bit for bit.
 */
#ifndef DIGITAL_EARTH_OUTPUT_SCALE_H
#define DIGITAL_EARTH_OUTPUT_SCALE_H
#include "digital_earth.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_SCALE_BOX 0        /* support 0.5: exact area average when shrinking by an integer, nearest when enlarging */
#define DE_SCALE_TRIANGLE 1   /* support 1 */
#define DE_SCALE_MITCHELL 2   /* support 2, B = C = 1/3 */
#define DE_SCALE_LANCZOS3 3   /* support 3 */

typedef struct de_output_scale {
    uint32_t struct_bytes;               /* sizeof(de_output_scale) of the caller; checked like de_tuning */
    int32_t enabled;                     /* 0 (default): the stage is off and the context delivers W x H */
    int32_t width, height;               /* the output size; 0, 0 stands for the context's W, H (default) */
    int32_t filter;                      /* DE_SCALE_*; default DE_SCALE_LANCZOS3 */
} de_output_scale;

/* Set the stage.  DE_ERR_INVALID: a mismatched struct_bytes; a filter out of range; width not a positive multiple of 16 or height of 8 (de_create's
 * rule: the pack kernel runs unchanged on the output); width / W or height / H outside [1/8, 8]; width * height > 2^28.  The size is checked whether
 * or not `enabled` is set.  DE_ERR_STATE while a lagged float fetch or a lagged pixel fetch is in flight (de_fetch_image_begin or
 * de_fetch_pixels_begin without its _end): what a pending _end returns has the size of its _begin.  A refused call changes nothing.  Staging
 * buffers that are too small for the new size are re-allocated by the next fetch that uses them, so a pointer from de_fetch_image_view,
 * de_fetch_pixels_view or an _end does not outlive a change of size. */
int de_set_output_scale(de_ctx* ctx, const de_output_scale* settings);
/* The current settings (before any de_set_output_scale: off, W x H, DE_SCALE_LANCZOS3). */
int de_get_output_scale(de_ctx* ctx, de_output_scale* out);
/* The size of what the calls above deliver now: width x height while the stage is on, W x H while it is off. */
int de_output_size(de_ctx* ctx, int* width, int* height);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_OUTPUT_SCALE_H */

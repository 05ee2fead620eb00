/* digital_earth_look.h — opt-in look LUTs of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * A look, a print emulation or a display calibration travels as a .cube file: a 1D table (three per-channel curves) or a 3D table (a lattice of
 * colours).  While the stage below is on, every pixel that the display transform wrote is sent through the tables, on the GPU, in place, directly
 * behind the display launch and ahead of output scaling: everything that hands out the DISPLAYED image — de_render_to_image, de_fetch_image and its
 * view and ring, the 8-bit, HDR and video pixels — delivers the graded image; de_fetch_hdr and every intermediate fetch (denoised, history, bloom,
 * local exposure) are untouched.  While the stage is off, the default, every call returns exactly the bytes it returned before this header existed.
 *
 * WHICH SIGNAL.  The stage acts on whatever signal the display wrote: the SDR picture (sRGB-encoded, under OpenDRT or AgX), or PQ / HLG /
 * display-linear values under the HDR output (digital_earth_hdr_output.h).  A table is made for one signal; loading one made for that signal is the
 * caller's business.  The library cannot tell and does not try.
 *
 * THE ARITHMETIC, all float32; every product is rounded before it is added (a multiply, then an add, never an fma), in exactly this order.
 *
 * Coordinate, per channel and per table of edge N (min, max: the table's input domain of that channel):
 *     k = fl((N - 1) / (max - min))        formed in double on the host from the float32 min and max, rounded to float32 once
 *     t = (x - min) * k
 *     t = t > 0 ? (t < N - 1 ? t : N - 1) : 0        NaN gives 0
 *     i = min((int)t, N - 2)
 *     f = t - (float)i                     exact; 0 <= f <= 1, and f = 1 only at the domain's upper end
 *
 * 1D table T[N][3], channel c with its own i, f:      y_c = a (1 - f) + b f,   a = T[i][c], b = T[i + 1][c].
 *
 * 3D table T[N][N][N][3], entry (r, g, b) at ((b N + g) N + r) 3 + c, red fastest, the file's own order.  (ir, fr), (ig, fg), (ib, fb) from the red,
 * green and blue inputs; cRGB below is the entry (ir + R, ig + G, ib + B), all three channels of it taking the same weights.
 *   DE_LOOK_TRILINEAR: the same mix nested along r, then g, then b:
 *     c00 = c000 (1 - fr) + c100 fr     c10 = c010 (1 - fr) + c110 fr     c01 = c001 (1 - fr) + c101 fr     c11 = c011 (1 - fr) + c111 fr
 *     c0 = c00 (1 - fg) + c10 fg        c1 = c01 (1 - fg) + c11 fg        y = c0 (1 - fb) + c1 fb
 *   DE_LOOK_TETRAHEDRAL: the Kuhn split of the cell into six tetrahedra around the diagonal c000 - c111.  The branches are tried in this order:
 *     if fr >= fg:   if fg >= fb:        y = (1 - fr) c000 + (fr - fg) c100 + (fg - fb) c110 + fb c111
 *                    else if fr >= fb:   y = (1 - fr) c000 + (fr - fb) c100 + (fb - fg) c101 + fg c111
 *                    else:               y = (1 - fb) c000 + (fb - fr) c001 + (fr - fg) c101 + fg c111
 *     else:          if fb >= fg:        y = (1 - fb) c000 + (fb - fg) c001 + (fg - fr) c011 + fr c111
 *                    else if fb >= fr:   y = (1 - fg) c000 + (fg - fb) c010 + (fb - fr) c011 + fr c111
 *                    else:               y = (1 - fg) c000 + (fg - fr) c010 + (fr - fb) c110 + fb c111
 *     The four terms are added left to right.  On a tie two branches apply; they differ in one vertex, whose weight is exactly 0, and every table
 *     value is finite, so both give the same value.
 *
 * Order of application, x the pixel as the display wrote it: the 1D table first if present, y = T1(x); then the 3D table on its result, y = T3(y)
 * (on x when there is no 1D table); then per channel
 *     o = x (1 - s) + y s                  s = strength, the ORIGINAL x
 *     o = o > 0 ? (o < 1 ? o : 1) : 0      the display's clamp: NaN and -0.0 give 0
 *
 * Consequences (tests/test_look_ref.py holds the numpy restatement tests/look_ref.py to them, and the GPU equals the restatement bit for bit):
 *   - a lattice point reproduces its table entry exactly (f = 0: a 1 + b 0), as far as the clamp to [0, 1] lets it through;
 *   - with the default domain 0, 1: k = N - 1 exactly, and x = 1.0 lands exactly on the last entry (i = N - 2, f = 1: a 0 + b 1);
 *   - strength = 0 is the identity on [0, 1], bit for bit (x 1 + y 0, y finite), for every table;
 *   - strength = 1 is exactly y clamped (x 0 + y 1, x finite: the display writes [0, 1] only).
 * A pixel that is not finite can only come through de_debug_look; IEEE arithmetic decides it (NaN in, 0 out; +inf in at strength 1: inf 0 = NaN, 0 out).
 * Whatever comes in, what goes out lies in [0, 1].
 */
#ifndef DIGITAL_EARTH_LOOK_H
#define DIGITAL_EARTH_LOOK_H
#include "digital_earth.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_LOOK_TRILINEAR   0
#define DE_LOOK_TETRAHEDRAL 1      /* default */
#define DE_LOOK_MAX_1D  65536
#define DE_LOOK_MAX_3D  65         /* edge length */

typedef struct de_look {
    uint32_t struct_bytes;         /* sizeof(de_look) of the caller; checked like de_tuning */
    int32_t  enabled;              /* 0 (default): the stage is off */
    int32_t  interpolation;        /* DE_LOOK_*; used by the 3D table only */
    float    strength;             /* [0, 1], default 1: out = x (1 - s) + y s */
    int32_t  size_1d;              /* 0: no 1D table; else 2 .. DE_LOOK_MAX_1D */
    float    min_1d[3], max_1d[3]; /* the 1D table's input domain per channel (default 0, 1) */
    int32_t  size_3d;              /* 0: no 3D table; else 2 .. DE_LOOK_MAX_3D */
    float    min_3d[3], max_3d[3]; /* the 3D table's input domain per channel (default 0, 1) */
} de_look;

/* Set the stage and copy the tables to the device: table_1d holds size_1d x 3 floats, entry i of channel c at 3 i + c; table_3d holds size_3d^3 x 3
 * floats, red fastest, ((b N + g) N + r) 3 + c, the file's own order.  The call waits for the upload: the caller's memory may die with it.  A table
 * whose size is 0 is dropped; the domain of a table whose size is 0 is not looked at.  enabled = 0 with tables keeps them for a later call (the
 * tables always travel with the call: there is no way to turn the stage on without naming them).
 * DE_ERR_INVALID: a mismatched struct_bytes; an interpolation out of range; a strength outside [0, 1] or NaN; a size out of range; enabled with both
 * sizes 0; a null table for a non-zero size; a domain that is not finite with max > min, or so narrow that k is not finite; any non-finite table
 * value.  A refused call changes nothing: the previous look stays in force.  The stage changes no size, so it may be set while lagged fetches are
 * in flight: a fetch already begun keeps the look it was begun with. */
int de_set_look(de_ctx* ctx, const de_look* settings, const float* table_1d, const float* table_3d);
/* The current settings; all zeros but struct_bytes while the stage is off. */
int de_get_look(de_ctx* ctx, de_look* out);
/* The kernel once over n_pixels host-given pixels (rgb and out: n_pixels x 3 floats; 1 <= n_pixels <= 2^28), with settings and tables of its own,
 * checked like de_set_look's (`enabled` is not looked at, but one table must be there).  Touches no context state. */
int de_debug_look(de_ctx* ctx, const float* rgb, uint64_t n_pixels, const de_look* settings, const float* table_1d, const float* table_3d, float* out);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_LOOK_H */

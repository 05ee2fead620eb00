/* digital_earth_rgbe.h — opt-in Radiance HDR output of libdigitalearth_hip.so: RGBE frames, run-length coded on the GPU (same library, ABI 6,
 * additions only).
 *
 * The scene-linear frame in the format environment maps are traded in: what include/digital_earth_exr.h delivers as OpenEXR — the frame's MEAN, or the
 * mean a stage ahead of the display made of it, in FRONT of the display transform — as one complete Radiance picture file (.hdr), and the
 * scene-linear panorama of include/digital_earth_environment.h as one such file too.  `source` takes the DE_EXR_SOURCE_* values with the refusals and
 * the side effects digital_earth_exr.h states for them.  Output scaling and the look do not apply: the file is always the context's W x H (the
 * panorama's width x height).  File row r, column x is the pixel de_fetch_pixels puts at row r, column x: rows run top-down, as the EXR file has them.
 *
 * THE SAMPLE, in integers.  v_c = mean_c * scale in float32 (one multiplication, not fused), c = R, G, B.
 *   1. A NaN or a value with the sign bit set becomes +0.
 *   2. Anything above 255 2^119 (bits 0x7EFF0000), +inf included, becomes 255 2^119: the largest RGBE value.
 *   3. m = max(v_R, v_G, v_B) — of non-negative floats, the one with the largest bits.
 *   4. m < 1e-32f: the pixel is 00 00 00 00.
 *   5. Else e = (bits(m) >> 23) - 126, so that m = f 2^e with f in [0.5, 1).  m is a normal float: 1e-32 is.  With M_c = the 24-bit significand of v_c
 *      (0 for +0 and for a denormal, which lies below every step) and sh_c = 16 + (bits(m) >> 23) - (bits(v_c) >> 23), v_c 2^(8 - e) = M_c / 2^sh_c exactly.
 *   6. rounding DE_RGBE_ROUND_TRUNC (the default; Radiance's own float2rgbe): q_c = floor(v_c 2^(8 - e)) = M_c >> sh_c, E = e + 128.
 *   7. rounding DE_RGBE_ROUND_NEAREST: q_c = floor(v_c 2^(8 - e) + 1/2) = (M_c + 2^(sh_c - 1)) >> sh_c.  If the largest q is 256, e becomes e + 1 and
 *      all three are taken again under sh_c + 1 (the largest becomes 128).  Should E pass 255 the pixel is the clamp's; step 2 keeps every value below that.
 *   The pixel is the four bytes q_R q_G q_B E.  The scaling by a power of two is exact: the device and a restatement in integers agree bit for bit.
 *   A decoder that returns q 2^(E - 136) reads a TRUNC file with an error in [0, 1) steps of 2^(e - 8), biased low by half a step; the decoders that
 *   return (q + 0.5) 2^(E - 136) (Radiance's own rgbe2float) centre it: |error| <= 1/2 step.  NEAREST is meant for the first kind: |error| <= 1/2 step there.
 *
 * THE FILE, byte for byte.  tests/rgbe_ref.py restates it in numpy and the GPU equals it byte for byte.
 * FRONT (the host's, once per setting and size), its lines in order:
 *     #?RADIANCE\n
 *     FORMAT=32-bit_rle_rgbe\n
 *     PRIMARIES=0.64 0.33 0.3 0.6 0.15 0.06 0.3127 0.329\n       Rec.709 / D65, which is what the sums are; always written, for Radiance's default white is equal-energy
 *     EXPOSURE=%.9g\n                                            of `scale`, only when scale != 1: the file's values are radiance times EXPOSURE
 *     \n
 *     -Y H +X W\n
 * A ROW, with `rle` on and 8 <= W <= 32767: 02 02 hi(W) lo(W), then the four planes R, G, B, E of the row — its W bytes q_R, then q_G, q_B, E —
 * each coded alone:
 *     A maximal stretch of equal bytes of length L >= 4 is a RUN: floor(L / 127) packets FF v and, if r = L mod 127 > 0, one packet (80 + r) v.
 *     What lies between runs are LITERALS: each maximal literal stretch is cut every 128 bytes into packets n, then n bytes, n = 1 ... 128.
 *     No packet crosses a plane.
 * THE BOUND of a coded plane is W + ceil(W / 128).  Proof: a run of L >= 4 costs 2 ceil(L / 127) <= L - 2 bytes (L = 4: 2; beyond, 2 L / 127 + 2 <= L - 2).
 * A literal stretch of n costs n + ceil(n / 128) <= n + floor(n / 128) + 1.  Runs and literal stretches alternate, so R runs lie beside at most R + 1
 * literal stretches, and a plane costs at most W + floor(W / 128) + (R + 1) - 2 R: with a run in it no more than W + floor(W / 128), without one
 * exactly W + ceil(W / 128) — a run always pays for the count byte of the literal stretch behind it.  A row is at most 4 + 4 (W + ceil(W / 128)).
 * A ROW with `rle` off, or with W < 8 or W > 32767, is FLAT: W pixels of four bytes R G B E, no row header — what the format prescribes there.
 * THE LENGTH leaves the device with the file, as the EXR file's does: on the device the file is preceded by a 16-byte word {uint64 length, uint32
 * status, uint32 pieces}.  de_rgbe_capacity = front + H (4 + 4 (W + ceil(W / 128))), flat front + 4 W H, is the proven bound.  Every
 * store is checked against its slot and the capacity: one that would pass is not made, raises the status word and ends the conversion with
 * DE_ERR_INTERNAL.  LIMIT: 4 W H <= 2^27 (DE_ERR_INVALID otherwise): 4096 x 2048 and 3840 x 2160 fit.
 * OUT OF SCOPE: old-style run-length coding, FORMAT=32-bit_rle_xyze, AOV channels in this format, other orientations than -Y +X.
 *
 * ENVIRONMENT MAPS.  While the panorama stage is on and all six linear slots of include/digital_earth_environment.h are held, de_render_to_rgbe,
 * de_fetch_rgbe, de_fetch_rgbe_view and de_fetch_rgbe_begin / _end deliver ONE file of panorama.width x panorama.height and de_rgbe_capacity answers
 * for that size: the slots resampled by the unchanged row-major resampling kernel into the image this coder reads with a divisor of 1, exactly as
 * the EXR calls do.  rle, rounding and scale are read at the fetch; `source` is read at the CAPTURE (de_exr.source: the slots are what they are).
 * With the stage on and fewer than six linear slots the calls answer DE_ERR_STATE.  de_set_panorama answers DE_ERR_STATE while an RGBE fetch begun
 * with the stage on is in flight.
 *
 * The conversion runs on the context stream with no host synchronisation in it.  Every other fetch and its buffers are untouched; the RGBE fetches
 * have device buffers, a pinned staging buffer and a four-deep pinned ring of their own, all allocated on first use.  With none of the calls below
 * made, nothing is allocated and nothing runs.
 */
#ifndef DIGITAL_EARTH_RGBE_H
#define DIGITAL_EARTH_RGBE_H
#include "digital_earth_environment.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_RGBE_ROUND_TRUNC 0          /* Radiance's own float2rgbe; suits decoders that add half a step */
#define DE_RGBE_ROUND_NEAREST 1        /* suits decoders that return q 2^(E - 136) */

typedef struct de_rgbe {
    uint32_t struct_bytes;               /* sizeof(de_rgbe) of the caller; checked like de_exr */
    int32_t source;                      /* DE_EXR_SOURCE_*; default DE_EXR_SOURCE_MEAN */
    int32_t rle;                         /* 0: flat rows; 1 (the default): run-length coded rows where the format allows them */
    int32_t rounding;                    /* DE_RGBE_ROUND_*; default DE_RGBE_ROUND_TRUNC */
    float scale;                         /* finite, > 0: multiplied into every sample in float32 and written as EXPOSURE; default 1.0 */
} de_rgbe;

/* Set the source, the coding, the rounding and the scale.  DE_ERR_INVALID: a value out of range, a mismatched struct_bytes; DE_ERR_STATE while RGBE
 * fetches are in flight (de_fetch_rgbe_begin without its _end).  A refused call changes nothing. */
int de_set_rgbe(de_ctx* ctx, const de_rgbe* settings);
/* The current settings (before any de_set_rgbe: the defaults above). */
int de_get_rgbe(de_ctx* ctx, de_rgbe* out);
/* The proven upper bound of any frame's length at the current settings.  DE_ERR_INVALID: the size passes the limit. */
int de_rgbe_capacity(de_ctx* ctx, uint64_t* bytes);
/* The stages up to the source's and the conversion behind them on the context stream; the file stays on the device (valid until the next conversion),
 * its length in the uint64 at *device_len (may be NULL), 16 bytes in front of it.  Nothing is waited for. */
int de_render_to_rgbe(de_ctx* ctx, const void** device_stream, const uint64_t** device_len);
/* The frame as it stands into `out`.  *len is the file's length either way; DE_ERR_INVALID if out_bytes is smaller (nothing is copied into `out`). */
int de_fetch_rgbe(de_ctx* ctx, void* out, uint64_t out_bytes, uint64_t* len);
/* The same without the last host copy: *host = the library's pinned RGBE staging buffer, valid until the next de_fetch_rgbe or de_fetch_rgbe_view. */
int de_fetch_rgbe_view(de_ctx* ctx, const void** host, uint64_t* len);
/* The recording loop pipelined, as de_fetch_exr_begin / _end, through a ring of four of its own: _begin enqueues the stages, the conversion and the
 * copy of the file's front part (the first estimate: the front and half the flat bytes) and returns at once; _end waits for the oldest RGBE fetch
 * begun, copies what the front part did not hold and hands out its buffer, valid until the ring comes round to it.  DE_ERR_STATE: a fifth _begin
 * without an _end, an _end without a _begin. */
int de_fetch_rgbe_begin(de_ctx* ctx);
int de_fetch_rgbe_end(de_ctx* ctx, const void** host, uint64_t* len);
/* The conversion once on a host-given image, free of the display: `image` is [H][W][3] float32 in R, G, B order, rows top-down, any W, H >= 1 within
 * the limit (DE_ERR_INVALID otherwise).  settings->source is not read; with scale 1 the image is what is converted.  Buffers of its own. */
int de_debug_rgbe(de_ctx* ctx, const float* image, int W, int H, const de_rgbe* settings, void* out, uint64_t out_bytes, uint64_t* len);
/* The host's part alone, no device and no context: the front of a W x H file into `out` (*len = its length; DE_ERR_INVALID and nothing written if
 * out_bytes is smaller; out may be NULL with out_bytes 0) and the capacity de_rgbe_capacity would answer.  Refuses what de_set_rgbe and
 * de_debug_rgbe refuse. */
int de_debug_rgbe_framing(const de_rgbe* settings, int W, int H, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity);
/* The twin of de_debug_environment_exr: the resampling and the RGBE conversion once on six host-given linear faces, faces[6][n][n][3] (any n in
 * 4 ... 16384), with `panorama` as de_set_panorama and `rgbe` as de_set_rgbe take them (`on` and `source` are not read).  The file goes to `out`, its
 * length to *len — also when out_bytes is too small (DE_ERR_INVALID).  Buffers and tables of its own; the context's settings and slots are untouched. */
int de_debug_environment_rgbe(de_ctx* ctx, const float* faces, int n, const de_panorama* panorama, const de_rgbe* rgbe, void* out, uint64_t out_bytes, uint64_t* len);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_RGBE_H */

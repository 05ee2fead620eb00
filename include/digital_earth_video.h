/* digital_earth_video.h — opt-in video frame output of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * An encoder, a raw-video pipe or a player takes Y'CbCr 4:2:0, not RGB.  The entry points below turn the DISPLAYED image — (W, H, 3) float32, pixels
 * of a column contiguous, row 0 at the bottom — into the planes of one video frame on the GPU and fetch those: 1.5 bytes per pixel at 8 bits, 3 at
 * 10 bits.  The frame is ONE contiguous buffer, planes tightly packed one after the other, rows top-down and the samples of a row contiguous
 * (r = H - 1 - v, x = u, as digital_earth_pixels.h).  With CW = W / 2, CH = H / 2 and B = bytes per sample (1 or 2):
 *     DE_VIDEO_NV12   B = 1   Y [H][W]            then CbCr [CH][CW][2]                      (Cb first)
 *     DE_VIDEO_I420   B = 1   Y [H][W]            then Cb [CH][CW]        then Cr [CH][CW]
 *     DE_VIDEO_P010   B = 2   Y [H][W] uint16     then CbCr [CH][CW][2]   the 10-bit code in the HIGH bits of each little-endian word (code << 6)
 *     DE_VIDEO_I010   B = 2   Y [H][W] uint16     then Cb [CH][CW]        then Cr [CH][CW]   the code in the LOW 10 bits: yuv420p10le
 * W * H * 3 / 2 * B bytes in all.  W and H are those of the displayed image: the output size while output scaling is on
 * (digital_earth_output_scale.h).  An odd width or height cannot be 4:2:0 (DE_ERR_STATE from the context's calls, DE_ERR_INVALID from
 * de_debug_video); a context's own W x H is always even (multiples of 16 and 8).
 *
 * THE ARITHMETIC, all f32, every operation rounded on its own (no fused multiply-add), in exactly this order.  The constants are evaluated once per
 * de_set_video on the host in double and rounded to f32:
 *     kr = f32(Kr), kb = f32(Kb), kg = 1.0f - (kr + kb)  (two f32 operations: then (kr + kb) + kg is exactly 1.0f and white has Y = 1)
 *     sb = f32(0.5 / (1 - Kb)),  sr = f32(0.5 / (1 - Kr))
 *     DE_VIDEO_MATRIX_BT709  Kr 0.2126  Kb 0.0722       _BT601  0.299  0.114       _BT2020  0.2627  0.0593  (the non-constant-luminance form)
 *   per pixel, from the three values t of the displayed image:
 *     R', G', B' = t > 0 ? (t < 1 ? t : 1) : 0                      (digital_earth_pixels.h's clamp: NaN and -0.0 give 0, +inf gives 1)
 *     Y  = ((kr * R') + (kb * B')) + (kg * G')
 *     Cb = (B' - Y) * sb,   Cr = (R' - Y) * sr                      per pixel, at full resolution
 *   per 4:2:0 chroma sample (i, j), j counted top-down, of either difference c(x, r) (column x, output row r), taps outside the image repeating the
 *   edge pixel (x = -1 reads x = 0, r = -1 reads r = 0; no other tap can leave an even-sized image):
 *     DE_VIDEO_SITING_CENTER    h(r) = c(2i, r) + c(2i + 1, r)                          C = (h(2j) + h(2j + 1)) * 0.25          JPEG / MPEG-1
 *     DE_VIDEO_SITING_LEFT      h(r) = (c(2i - 1, r) + c(2i + 1, r)) + 2 * c(2i, r)     C = (h(2j) + h(2j + 1)) * 0.125         MPEG-2 / H.264 default
 *     DE_VIDEO_SITING_TOPLEFT   h as LEFT                                               C = ((h(2j - 1) + h(2j + 1)) + 2 * h(2j)) * 0.0625     BT.2020 / HDR
 *   codes at n = 8 or 10 bits, k = 2^(n - 8), M = 2^n - 1 (ITU-T H.273), then clipped to the plane's legal range [lo, hi]:
 *     DE_VIDEO_RANGE_LIMITED    y = Y * (219 k) + 16 k   in [16 k, 235 k]       c = C * (224 k) + 128 k     in [16 k, 240 k]
 *     DE_VIDEO_RANGE_FULL       y = Y * M + 0            in [0, M]              c = C * M + 2^(n - 1)       in [0, M]
 *     s = v > lo ? (v < hi ? v : hi) : lo                            (a multiply, then an add, then the clip)
 *   quantised by `mode` as digital_earth_pixels.h states it, with 255 replaced by the span [lo, hi]:
 *     DE_PIXELS_TRUNCATE  q = (int)s
 *     DE_PIXELS_ROUND     q = (int)(s + 0.5)
 *     DE_PIXELS_DITHER    q = (int)((s + 0.5) + a * tri),  d = s - lo, e = hi - s, a = min(min(d, e), 1),  tri = pixels' triangular noise of
 *                         mix(key ^ idx), key = mix(seed + 0x9E3779B9 phase) (DESIGN.md §14 has mix), idx = 4 * (the sample's index in its plane, row-major,
 *                         r W + x for Y and j CW + i for Cb and Cr) + plane (0 = Y, 1 = Cb, 2 = Cr)
 * so the lowest and the highest legal code of a plane stay exact in every mode: black is (16, 128, 128) k and white (235, 128, 128) k in limited
 * range.  With animate = 0 the phase is 0 always; otherwise it counts this context's conversions since de_set_video.  tests/video_ref.py restates all
 * of this in numpy, and the GPU equals it byte for byte.  Out of scope: 4:2:2 / 4:4:4, alpha, constant-luminance BT.2020, super-white / sub-black.
 *
 * The conversion is one kernel behind the unchanged display transform (and behind output scaling) and reads its output, so everything the display
 * honours is inherited: adaptive counts, the denoiser, history, the meter, bloom, local exposure, display sources, AgX — and the HDR signal while
 * de_set_hdr_output is on: PQ in a Rec.2020 container, NCL matrix, 10 bits, top-left siting is {DE_VIDEO_I010 or _P010, _MATRIX_BT2020, _SITING_TOPLEFT}.
 * KNOWN LIMIT, carried over from digital_earth_hdr_output.h: only DE_HDR_GAMUT_REC709 is colorimetrically meaningful there (the reference's P3 / Rec.2020
 * gamut products multiply by the transposed matrices); this stage packs whatever signal that stage produced.
 * de_render_to_image, de_fetch_image*, de_fetch_pixels*, de_fetch_hdr_pixels and their buffers are untouched; the video fetches have a device buffer,
 * a pinned staging buffer and a four-deep pinned ring of their own (each sized for the 10-bit formats, allocated on first use), so float, pixel and
 * video fetches may be in flight together and each _end hands out the oldest of its own ring.
 */
#ifndef DIGITAL_EARTH_VIDEO_H
#define DIGITAL_EARTH_VIDEO_H
#include "digital_earth_pixels.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_VIDEO_NV12 0
#define DE_VIDEO_I420 1
#define DE_VIDEO_P010 2
#define DE_VIDEO_I010 3

#define DE_VIDEO_MATRIX_BT709 0
#define DE_VIDEO_MATRIX_BT601 1
#define DE_VIDEO_MATRIX_BT2020 2

#define DE_VIDEO_RANGE_LIMITED 0
#define DE_VIDEO_RANGE_FULL 1

#define DE_VIDEO_SITING_LEFT 0
#define DE_VIDEO_SITING_CENTER 1
#define DE_VIDEO_SITING_TOPLEFT 2

typedef struct de_video {
    uint32_t struct_bytes;               /* sizeof(de_video) of the caller; checked like de_pixels */
    int32_t format;                      /* DE_VIDEO_NV12 (default), _I420, _P010 or _I010 */
    int32_t matrix;                      /* DE_VIDEO_MATRIX_BT709 (default), _BT601 or _BT2020 */
    int32_t range;                       /* DE_VIDEO_RANGE_LIMITED (default) or _FULL */
    int32_t siting;                      /* DE_VIDEO_SITING_LEFT (default), _CENTER or _TOPLEFT */
    int32_t mode;                        /* DE_PIXELS_TRUNCATE, DE_PIXELS_ROUND (default) or DE_PIXELS_DITHER */
    uint32_t seed;                       /* of the dither's hash; default 0 */
    int32_t animate;                     /* 0 (default): phase 0 always; otherwise the phase counts this context's conversions */
} de_video;

/* Set the frame format and reset the phase counter.  DE_ERR_INVALID: any enum out of range, a mismatched struct_bytes; DE_ERR_STATE while video
 * fetches are in flight (de_fetch_videoframe_begin without its _end).  A refused call changes nothing. */
int de_set_video(de_ctx* ctx, const de_video* settings);
/* The current settings (before any de_set_video: the defaults above) and, when last_phase is not NULL, the phase of the newest conversion. */
int de_get_video(de_ctx* ctx, de_video* out, uint32_t* last_phase);
/* The frame's size and geometry at the current settings and output size; any pointer may be NULL.  plane_offsets: the byte offset of the first Y, Cb
 * and Cr sample; plane_strides: the bytes from one row of that plane to the next (NV12 / P010: Cr = Cb + one sample, both with the interleaved
 * plane's stride).  DE_ERR_STATE for an odd output size. */
int de_videoframe_bytes(de_ctx* ctx, uint64_t* bytes, uint64_t* plane_offsets, uint64_t* plane_strides);
/* de_render_to_image, then the conversion behind it on the context stream; the frame stays on the device (valid until the next conversion). */
int de_render_to_video(de_ctx* ctx, const void** device_frame);
/* The frame as it stands into `out` (out_bytes >= the frame's bytes, else DE_ERR_INVALID); mirrors de_fetch_pixels. */
int de_fetch_video(de_ctx* ctx, void* out, uint64_t out_bytes);
/* The same without the last host copy: *host = the library's pinned video staging buffer, valid until the next de_fetch_video or
 * de_fetch_videoframe_view on this context. */
int de_fetch_videoframe_view(de_ctx* ctx, const void** host);
/* The recording loop pipelined, as de_fetch_pixels_begin / _end: _begin enqueues the display transform, the conversion and the copy into one of four
 * pinned buffers and returns at once; _end waits for the oldest video fetch begun and hands out its buffer, valid until the ring comes round to it.
 * DE_ERR_STATE: a fifth _begin without an _end, an _end without a _begin. */
int de_fetch_videoframe_begin(de_ctx* ctx);
int de_fetch_videoframe_end(de_ctx* ctx, const void** host);
/* The conversion once on a host-given (W, H, 3) image of ANY even size (DE_ERR_INVALID otherwise, or W * H > 2^28), free of the context's size.
 * Buffers of its own; the context's settings, frame and phase counter are not touched.  `out` takes W * H * 3 / 2 * B bytes. */
int de_debug_video(de_ctx* ctx, const float* image, int W, int H, const de_video* settings, uint32_t phase, void* out);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_VIDEO_H */

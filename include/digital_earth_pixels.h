/* digital_earth_pixels.h — opt-in 8-bit pixel output of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * de_fetch_image hands back the reference's field: (W, H, 3) float32, pixels of a column contiguous, row 0 at the bottom — 12 bytes per pixel over
 * the link, and a clip, a scale, a cast, a transpose and a flip on one host thread before a canvas, an image writer or an encoder can take it.  The
 * entry points below convert the displayed image on the GPU instead and fetch the bytes: out[r][x][ch], `channels` (3 or 4) bytes per pixel, pixels
 * of a ROW contiguous, row 0 at the TOP (r = H - 1 - v, x = u), alpha = 255.  Per value t of the displayed image, all in f32:
 *     cl = t > 0 ? (t < 1 ? t : 1) : 0          (NaN and -0.0 give 0, +inf gives 1)
 *     s  = cl * 255
 *     DE_PIXELS_TRUNCATE  q = (int)s             the reference's to_vec3u: what a screenshot has always held
 *     DE_PIXELS_ROUND     q = (int)(s + 0.5)
 *     DE_PIXELS_DITHER    q = (int)((s + 0.5) + a * tri),  a = min(s, 255 - s, 1),  tri triangular on (-1, 1) from a 32-bit hash of (seed, phase,
 *                         pixel, channel): two LSB wide, unbiased, and fading out at both ends so that black stays 0 and clipped white stays 255
 * (DESIGN.md §14 has the hash).  With animate = 0 the phase is 0 and a frame always gives the same bytes; otherwise the phase is the number of
 * conversions this context has run since de_set_pixels, so the pattern changes from display to display.
 *
 * The conversion is one kernel behind the unchanged display transform and reads its output, so everything the display honours is inherited (adaptive
 * counts, the denoiser, history, the meter, bloom, display sources, AgX).  de_render_to_image, de_fetch_image* and the image they produce are
 * untouched; the pixel fetches have a staging buffer and a four-deep pinned ring of their own (W * H * channels bytes on the device, five times that
 * pinned, allocated on first use), so float and pixel fetches may be in flight together and each _end hands out the oldest of its own ring.
 */
#ifndef DIGITAL_EARTH_PIXELS_H
#define DIGITAL_EARTH_PIXELS_H
#include "digital_earth.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_PIXELS_TRUNCATE 0
#define DE_PIXELS_ROUND 1
#define DE_PIXELS_DITHER 2

typedef struct de_pixels {
    uint32_t struct_bytes;               /* sizeof(de_pixels) of the caller; checked like de_tuning */
    int32_t channels;                    /* 3 (RGB8) or 4 (RGBA8, alpha 255); default 4 */
    int32_t mode;                        /* DE_PIXELS_TRUNCATE (default), DE_PIXELS_ROUND or DE_PIXELS_DITHER */
    uint32_t seed;                       /* of the dither's hash; default 0 */
    int32_t animate;                     /* 0 (default): phase 0 always; otherwise the phase counts this context's conversions */
} de_pixels;

/* Set the pixel format and reset the phase counter.  DE_ERR_INVALID: channels not 3 or 4, mode not 0 ... 2, a mismatched struct_bytes;
 * DE_ERR_STATE while pixel fetches are in flight (de_fetch_pixels_begin without its _end). */
int de_set_pixels(de_ctx* ctx, const de_pixels* settings);
/* The current settings (before any de_set_pixels: 4 channels, truncate, seed 0, animate 0) and, when last_phase is not NULL, the phase of the newest
 * conversion (0 before the first). */
int de_get_pixels(de_ctx* ctx, de_pixels* out, uint32_t* last_phase);
/* de_render_to_image, then the conversion behind it on the context stream; the pixels stay on the device (valid until the next conversion). */
int de_render_to_pixels(de_ctx* ctx, const uint8_t** device_pixels);
/* The pixels of the frame as it stands into `out` (out_bytes >= W * H * channels, else DE_ERR_INVALID); mirrors de_fetch_image. */
int de_fetch_pixels(de_ctx* ctx, uint8_t* out, uint64_t out_bytes);
/* The same without the last host copy: *host = the library's pinned pixel staging buffer, valid until the next de_fetch_pixels or
 * de_fetch_pixels_view on this context; mirrors de_fetch_image_view. */
int de_fetch_pixels_view(de_ctx* ctx, const uint8_t** host);
/* The window loop pipelined, as de_fetch_image_begin / _end: _begin enqueues the display transform, the conversion and the copy into one of four
 * pinned buffers and returns at once (no host synchronisation); _end waits for the oldest pixel fetch begun and hands out its buffer, valid until the
 * ring comes round to it (the fourth _begin after the one that filled it).  DE_ERR_STATE: a fifth _begin without an _end, an _end without a _begin. */
int de_fetch_pixels_begin(de_ctx* ctx);
int de_fetch_pixels_end(de_ctx* ctx, const uint8_t** host);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_PIXELS_H */

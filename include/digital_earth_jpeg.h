/* digital_earth_jpeg.h — opt-in JPEG output of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * A headless renderer's picture has to leave the node as something a consumer can open.  The entry points below turn the DISPLAYED image — the one
 * every packed output reads, behind the display transform, the look and output scaling — into one baseline JPEG (ITU-T T.81 sequential DCT, Huffman,
 * 8 bits; JFIF 1.02) on the GPU and fetch that: ONE contiguous, complete file image, of the order of a tenth of a byte per float of the image.
 *
 * INPUT.  W and H are the output size (digital_earth_output_scale.h) and must be even (DE_ERR_STATE from the context's calls, DE_ERR_INVALID from
 * de_debug_jpeg).  The samples are exactly the codes de_debug_video gives for {DE_VIDEO_I420, DE_VIDEO_MATRIX_BT601, DE_VIDEO_RANGE_FULL,
 * DE_VIDEO_SITING_CENTER, DE_PIXELS_ROUND} — JFIF's Y'CbCr, stated in digital_earth_video.h and not again here; videoframe_pack_kernel writes them,
 * unchanged, into planes this stage owns.  No dither: it would only feed the quantiser noise.
 * MCU.  16 x 16 pixels: four Y blocks in raster order, one Cb, one Cr, interleaved in one scan; SOF0's sampling factors are 2x2, 1x1, 1x1.  MCUs run
 * left to right, top row first (rows top-down, as all packed outputs).  A sample outside the image repeats its plane's last column / last row; SOF0
 * carries the true W and H.
 * DCT.  Integer, per 8 x 8 block, s = code - 128:
 *     M[u][x] = rint(2^14 * 1/2 c(u) cos((2 x + 1) u pi / 16)),  c(0) = 1 / sqrt(2), c = 1 otherwise      (on the host in double, int32)
 *     T[y][u] = sum_x M[u][x] s[y][x],   T' = (T + 2^9) >> 10   (arithmetic shift)
 *     F[v][u] = sum_y M[v][y] T'[y][u]                           the true coefficient x 2^18
 *   |T| <= 5 932 032, |T'| <= 5793, |F| <= 268 470 792: int32 throughout.
 * QUANTISER.  q = sign(F) ((|F| + D / 2) / D), D = Q << 18, integer division: ties away from zero.  Q: T.81 Annex K.1 (luminance) and K.2
 * (chrominance) scaled by the IJG rule for quality 1 ... 100: scale = 5000 / quality below 50, otherwise 200 - 2 quality; Q = clamp((base scale +
 * 50) / 100, 1, 255), all in integers, computed by de_set_jpeg.  DQT carries them in zigzag order at 8-bit precision.
 * ENTROPY CODING.  Huffman with the four typical tables of Annex K.3 - K.6, written into DHT, never optimised per frame.  DC: the difference to the
 * previous block of the same component, the predictor 0 at the start of every restart interval.  AC: run / size with ZRL (0xF0) and EOB (0x00).  A
 * negative value is coded as value - 1 in `size` bits.  Bits are packed MSB first, a 0x00 follows every 0xFF data byte, every interval is padded to a
 * byte boundary with 1-bits; RSTm, m = interval index mod 8, stands between intervals, none after the last; EOI ends the stream.
 * RESTART INTERVAL.  restart_mcus in 1 ... 65535, written into DRI: the encoder's unit of parallelism (intervals are independent by construction).
 * Streams without restart markers are out of scope.  The default, DE_JPEG_DEFAULT_RESTART = 2, is the value among {1, 2, 4, 8, 16, one MCU row} with
 * the lowest encode time at 1920 x 1080 whose stream is at most 2 % longer than the one-MCU-row stream of the same frame: the table measured on an
 * MI355X in profiles/jpeg.md.
 * FRAMING, written by the host once per de_set_jpeg (and per output size) into the front of the stream: SOI; APP0 "JFIF" 1.02, units 0, density 1:1,
 * no thumbnail; DQT x 2; SOF0; DHT x 4 (DC luminance, AC luminance, DC chrominance, AC chrominance); DRI; SOS with Ss = 0, Se = 63, Ah / Al = 0 —
 * 629 bytes.  The device appends the entropy-coded data and EOI.  tests/jpeg_ref.py restates all of this in numpy integers on top of
 * tests/video_ref.py's planes, and the GPU equals it byte for byte.
 * THE LENGTH leaves the device with the stream: on the device the stream is preceded by a 16-byte word {uint64 length, uint32 status, uint32
 * intervals}; a fetch copies that word and then `length` bytes, never the capacity.  de_jpeg_capacity is the proven upper bound of any frame (the
 * worst case of a block is derived in csrc/jpeg_kernels.hip): every device buffer is that large, and a store that would pass it — the derivation says
 * there is none — ends the conversion with DE_ERR_INTERNAL instead of being made.
 * OUT OF SCOPE: progressive and arithmetic coding, 4:4:4 / 4:2:2 / grayscale, optimised Huffman tables, EXIF / ICC, and the meaning of the HDR signal —
 * the stage encodes whatever signal the display wrote (de_set_hdr_output's PQ / HLG included), as the video stage does.
 *
 * The conversion runs behind the unchanged display transform on the context stream with no host synchronisation in it.  de_render_to_image,
 * de_fetch_image*, de_fetch_pixels*, de_fetch_hdr_pixels, de_fetch_video* and their buffers are untouched; the JPEG fetches have device buffers, a
 * pinned staging buffer and a four-deep pinned ring of their own, all allocated on first use, so float, pixel, video and JPEG fetches may be in flight
 * together and each _end hands out the oldest of its own ring.  With none of the calls below made, nothing is allocated and nothing runs.
 */
#ifndef DIGITAL_EARTH_JPEG_H
#define DIGITAL_EARTH_JPEG_H
#include "digital_earth_video.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_JPEG_DEFAULT_RESTART 2      /* MCUs per restart interval: measured, profiles/jpeg.md */
#define DE_ERR_INTERNAL (-6)           /* a check the library's own derivation says cannot fail did: nothing was written out of bounds */

typedef struct de_jpeg {
    uint32_t struct_bytes;               /* sizeof(de_jpeg) of the caller; checked like de_pixels */
    int32_t quality;                     /* 1 ... 100, the IJG scale; default 90 */
    int32_t restart_mcus;                /* 1 ... 65535 MCUs per restart interval; default DE_JPEG_DEFAULT_RESTART */
} de_jpeg;

/* Set the quality and the restart interval; computes the tables and the framing.  DE_ERR_INVALID: a value out of range, a mismatched struct_bytes;
 * DE_ERR_STATE while JPEG fetches are in flight (de_fetch_jpeg_begin without its _end).  A refused call changes nothing. */
int de_set_jpeg(de_ctx* ctx, const de_jpeg* settings);
/* The current settings (before any de_set_jpeg: the defaults above). */
int de_get_jpeg(de_ctx* ctx, de_jpeg* out);
/* An upper bound of any frame's length at the current settings and output size.  DE_ERR_STATE for an odd output size. */
int de_jpeg_capacity(de_ctx* ctx, uint64_t* bytes);
/* de_render_to_image, then the conversion behind it on the context stream; the stream stays on the device (valid until the next conversion), its
 * length in the uint64 at *device_len (may be NULL), 16 bytes in front of it.  Nothing is waited for. */
int de_render_to_jpeg(de_ctx* ctx, const void** device_stream, const uint64_t** device_len);
/* The frame as it stands into `out`.  *len is the frame's length either way; DE_ERR_INVALID if out_bytes is smaller (nothing is copied into `out`). */
int de_fetch_jpeg(de_ctx* ctx, void* out, uint64_t out_bytes, uint64_t* len);
/* The same without the last host copy: *host = the library's pinned JPEG staging buffer, valid until the next de_fetch_jpeg or de_fetch_jpeg_view. */
int de_fetch_jpeg_view(de_ctx* ctx, const void** host, uint64_t* len);
/* The recording loop pipelined, as de_fetch_videoframe_begin / _end: _begin enqueues the display transform, the conversion and the copy of the frame's
 * front into one of four pinned buffers and returns at once; _end waits for the oldest JPEG fetch begun, copies what the front did not hold (the
 * front grows with the frames: a steady sequence copies once) and hands out its buffer, valid until the ring comes round to it.
 * DE_ERR_STATE: a fifth _begin without an _end, an _end without a _begin. */
int de_fetch_jpeg_begin(de_ctx* ctx);
int de_fetch_jpeg_end(de_ctx* ctx, const void** host, uint64_t* len);
/* The conversion once on a host-given (W, H, 3) image of ANY even size (DE_ERR_INVALID otherwise, or W * H > 2^24), free of the context's size.
 * Buffers of its own; the context's settings and streams are not touched.  *len and out_bytes as de_fetch_jpeg. */
int de_debug_jpeg(de_ctx* ctx, const float* image, int W, int H, const de_jpeg* settings, void* out, uint64_t out_bytes, uint64_t* len);
/* The host's part alone, no device and no context: the framing of a W x H frame at `settings` into `out` (*len = 629; DE_ERR_INVALID and nothing
 * written if out_bytes is smaller; out may be NULL with out_bytes 0) and the capacity de_jpeg_capacity would answer.  Refuses what de_set_jpeg refuses. */
int de_debug_jpeg_framing(const de_jpeg* settings, int W, int H, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_JPEG_H */

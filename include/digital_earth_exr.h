/* digital_earth_exr.h — opt-in OpenEXR output of libdigitalearth_hip.so (same library, additions only).
 *
 * The scene-linear file — the radiance a path tracer exists to produce, the one people composite, grade, denoise elsewhere and archive — made on the
 * GPU: the entry points below turn the frame's MEAN (or the mean a stage ahead of the display made of it) into one complete OpenEXR scan-line file
 * (converted, laid out in planes, reordered, predicted, deflated, framed) and fetch that.  Every other file of this library sits behind the display
 * transform; this one sits in front of it.
 *   source DE_EXR_SOURCE_MEAN             what the display launch would read with every stage off: the sums (the context's own, the display source of
 *                                         de_set_display_source, or the reduced frame), each channel divided in float32 by the frame's sample count or,
 *                                         inside an adaptive frame, by the tile's own
 *   source DE_EXR_SOURCE_DENOISED, _HISTORY, _BLOOM, _LOCAL_EXPOSURE
 *                                         exactly the image de_fetch_denoised_hdr / de_fetch_history_hdr (its colour) / de_fetch_bloom_hdr /
 *                                         de_fetch_local_exposure_hdr hand out: the display's stage chain left at that stage.  They refuse with the same
 *                                         codes and messages as those fetches and have the same side effects on the meter and the history, no others.
 * Output scaling and the look act on the DISPLAYED image and do not apply: the file is always the context's W x H.  File row r, column x is the pixel
 * de_fetch_pixels puts at row r, column x: rows run top-down.
 *
 * THE SAMPLE, in integers.  1. v = mean * scale in float32 (one multiplication, not fused).  2. A NaN becomes +0 in both pixel types.  3. FLOAT stores
 * the 32 bits of v.  4. HALF: with s = the sign bit and a = the other 31 bits of v,
 *       a >= 0x477FE000 (|v| >= 65504, the infinities included)   s | 0x7BFF                               (the clamp to +-65504)
 *       a >= 0x38800000 (|v| >= 2^-14, a normal half)             s | ((a + 0xFFF + ((a >> 13) & 1) - 0x38000000) >> 13)      (nearest, ties to even)
 *       a <= 0x33000000 (|v| <= 2^-25)                            s                                        (2^-25 itself is the tie between 0 and the smallest)
 *       else, with e = a >> 23, m = (a & 0x7FFFFF) | 0x800000, k = 126 - e (14 ... 24): h = m >> k, r = m & (2^k - 1);  h + 1 if r > 2^(k-1), or if
 *       r == 2^(k-1) and h is odd;  s | h                                                                    (a subnormal half, kept)
 *    — for every v that is not a NaN, the binary16 that clip(v, -65504, 65504) rounds to under IEEE 754 round-to-nearest-even.
 *
 * THE FILE, byte for byte; everything is little-endian.  tests/exr_ref.py restates it in numpy and the GPU equals it byte for byte.
 * FRONT (the host's, once per setting and size).  Magic and version 76 2F 31 01, 02 00 00 00.  Then the eight required attributes in this order, each
 * as name\0 type\0 int32 size, value:
 *     channels (chlist)            the channels B, G, R in that order, then \0; each is name\0, int32 pixel type (1 HALF, 2 FLOAT), uint8 pLinear 0, three
 *                                  zero bytes, int32 xSampling 1, int32 ySampling 1
 *     compression (compression)    1 byte: 0, 2 or 3
 *     dataWindow (box2i)           0, 0, W - 1, H - 1
 *     displayWindow (box2i)        0, 0, W - 1, H - 1
 *     lineOrder (lineOrder)        1 byte, 0 (increasing y)
 *     pixelAspectRatio (float)     1.0
 *     screenWindowCenter (v2f)     0, 0
 *     screenWindowWidth (float)    1.0
 * then one 00 byte: 313 bytes.  Then the OFFSET TABLE: nb = ceil(H / L) uint64 absolute file offsets of the blocks, L = 16 lines per block under ZIP
 * and 1 under ZIPS and NONE.  The device writes the table — it knows the lengths —; the front's length, 313 + 8 nb, is fixed.
 * BLOCK b holds the lines y0 = b L ... min(y0 + L, H) - 1: int32 y0, int32 dataSize, then dataSize bytes.  With bps = 2 (HALF) or 4 (FLOAT):
 * RAW BLOCK BYTES r[0 .. P), P = lines W 3 bps: for each line top-down all W samples of B, then of G, then of R; a sample's own bytes are not swizzled.
 * ZIP / ZIPS PAYLOAD.  h = (P + 1) / 2; t[i] = r[2 i] for i < h, t[h + i] = r[2 i + 1]; p[0] = t[0], p[i] = (t[i] - t[i - 1] + 128) mod 256.  The
 * payload is one zlib stream over p: 78 01; then p cut every chunk_bytes (1024 ... 65535) into deflate chunks coded EXACTLY as the PNG output's chunks
 * (digital_earth_png.h: TOKENS, CODES, ALIGNMENT — the same tokens, the same code construction and 15-bit repair, the same 1222-bit header, the same
 * stored fallback per chunk, the same empty stored block behind every chunk but the block's last, BFINAL on the block's last); then the Adler-32 of p,
 * big-endian.  No chunk, match or run crosses a block.
 * RAW FALLBACK.  If that stream's length Z >= P the block is written raw instead: dataSize = P and the data is r.  (Readers take dataSize == P as
 * "not compressed" and refuse dataSize > P.)  NONE: dataSize = P, data r, L = 1.
 * THE LENGTH leaves the device with the file, as the PNG file's does: on the device the file is preceded by a 16-byte word {uint64 length, uint32
 * status, uint32 pieces}.  de_exr_capacity = front + 8 nb + H W 3 bps is the proven bound (a block is at most its 8-byte header and P
 * bytes, by the raw fallback).  Every store is checked against its slot and the capacity: one that would pass is not made, raises the status word and
 * ends the conversion with DE_ERR_INTERNAL.  LIMIT: H W 3 bps <= 2^27 (DE_ERR_INVALID otherwise): 3840 x 2160 at FLOAT fits.
 * DE_EXR_DEFAULT_CHUNK = 32768 is the PNG output's measured default; for this output it is UNMEASURED (the rule: profiles/exr.md).
 * OUT OF SCOPE: PIZ / PXR24 / B44 / DWA compression, tiles, multi-part and deep files, alpha, luminance /
 * chroma, the `chromaticities` attribute (absent means Rec.709 primaries and D65, which is what the sums are), LZ77 beyond distance 1.
 * Extra channels beside B, G, R (depth, normal, albedo, coverage, transmittance, variance, samples) are digital_earth_exr_aovs.h's.
 *
 * The conversion runs on the context stream with no host synchronisation in it.  Every other fetch and its buffers are untouched; the EXR fetches have
 * device buffers, a pinned staging buffer and a four-deep pinned ring of their own, all allocated on first use.  With none of the calls below made,
 * nothing is allocated and nothing runs.
 */
#ifndef DIGITAL_EARTH_EXR_H
#define DIGITAL_EARTH_EXR_H
#include "digital_earth_png.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_EXR_SOURCE_MEAN 0
#define DE_EXR_SOURCE_DENOISED 1
#define DE_EXR_SOURCE_HISTORY 2
#define DE_EXR_SOURCE_BLOOM 3
#define DE_EXR_SOURCE_LOCAL_EXPOSURE 4
#define DE_EXR_PIXEL_HALF 1            /* the file's own pixel type numbers */
#define DE_EXR_PIXEL_FLOAT 2
#define DE_EXR_COMPRESSION_NONE 0      /* the file's own compression numbers */
#define DE_EXR_COMPRESSION_ZIPS 2
#define DE_EXR_COMPRESSION_ZIP 3
#define DE_EXR_DEFAULT_CHUNK 32768     /* predicted bytes per deflate chunk: unmeasured for this output (the PNG output's), profiles/exr.md */

typedef struct de_exr {
    uint32_t struct_bytes;               /* sizeof(de_exr) of the caller; checked like de_png */
    int32_t source;                      /* DE_EXR_SOURCE_*; default DE_EXR_SOURCE_MEAN */
    int32_t pixel_type;                  /* DE_EXR_PIXEL_*; default DE_EXR_PIXEL_HALF */
    int32_t compression;                 /* DE_EXR_COMPRESSION_*; default DE_EXR_COMPRESSION_ZIP */
    int32_t chunk_bytes;                 /* 1024 ... 65535; default DE_EXR_DEFAULT_CHUNK */
    float scale;                         /* finite, > 0: multiplied into every sample in float32; default 1.0 */
} de_exr;

/* Set the source, the pixel type, the compression, the chunk size and the scale.  DE_ERR_INVALID: a value out of range, a mismatched struct_bytes;
 * DE_ERR_STATE while EXR fetches are in flight (de_fetch_exr_begin without its _end).  A refused call changes nothing. */
int de_set_exr(de_ctx* ctx, const de_exr* settings);
/* The current settings (before any de_set_exr: the defaults above). */
int de_get_exr(de_ctx* ctx, de_exr* out);
/* The proven upper bound of any frame's length at the current settings.  DE_ERR_INVALID: the context's size passes the limit at these settings. */
int de_exr_capacity(de_ctx* ctx, uint64_t* bytes);
/* The stages up to the source's and the conversion behind them on the context stream; the file stays on the device (valid until the next conversion),
 * its length in the uint64 at *device_len (may be NULL), 16 bytes in front of it.  Nothing is waited for. */
int de_render_to_exr(de_ctx* ctx, const void** device_stream, const uint64_t** device_len);
/* The frame as it stands into `out`.  *len is the file's length either way; DE_ERR_INVALID if out_bytes is smaller (nothing is copied into `out`). */
int de_fetch_exr(de_ctx* ctx, void* out, uint64_t out_bytes, uint64_t* len);
/* The same without the last host copy: *host = the library's pinned EXR staging buffer, valid until the next de_fetch_exr or de_fetch_exr_view. */
int de_fetch_exr_view(de_ctx* ctx, const void** host, uint64_t* len);
/* The recording loop pipelined, as de_fetch_png_begin / _end, through a ring of four of its own: _begin enqueues the stages, the conversion and the
 * copy of the file's front part (the first estimate: the front and half the raw bytes) and returns at once; _end waits for the oldest EXR fetch
 * begun, copies what the front part did not hold and hands out its buffer, valid until the ring comes round to it.  DE_ERR_STATE: a fifth _begin
 * without an _end, an _end without a _begin. */
int de_fetch_exr_begin(de_ctx* ctx);
int de_fetch_exr_end(de_ctx* ctx, const void** host, uint64_t* len);
/* The conversion once on a host-given image, free of the display: `image` is [H][W][3] float32 in R, G, B order, rows top-down, any W, H >= 1 within
 * the limit (DE_ERR_INVALID otherwise).  settings->source is not read; with scale 1 the image is what is converted.  Buffers of its own. */
int de_debug_exr(de_ctx* ctx, const float* image, int W, int H, const de_exr* settings, void* out, uint64_t out_bytes, uint64_t* len);
/* The host's part alone, no device and no context: the front of a W x H file, its offset table zeroed, into `out` (*len = 313 + 8 nb; DE_ERR_INVALID
 * and nothing written if out_bytes is smaller; out may be NULL with out_bytes 0) and the capacity de_exr_capacity would answer.  Refuses what
 * de_set_exr and de_debug_exr refuse. */
int de_debug_exr_framing(const de_exr* settings, int W, int H, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_EXR_H */

/* digital_earth_png.h — opt-in PNG output of libdigitalearth_hip.so (same library, ABI 6, additions only).
 *
 * The lossless file — the one people archive, diff and composite — made on the GPU: the entry points below turn the packed pixels of the DISPLAYED
 * image into one complete PNG (filtered, deflated, framed) and fetch that.  The stage does not state the samples again:
 *   source DE_PNG_SOURCE_PIXELS       colour type 2 (3 channels) or 6 (4), depth 8: what pixels_kernels.hip writes at the context's de_set_pixels
 *                                     settings (channels, mode, seed; the dither phase counts this stage's own conversions while `animate` is set)
 *   source DE_PNG_SOURCE_HDR_PIXELS   colour type 2, depth 16, big-endian: the HDR pack at DE_HDR_PIXELS_RGB16 (digital_earth_hdr_output.h);
 *                                     DE_ERR_STATE from the context's calls while the HDR output is off or set to RGB10A2
 * Each pack writes into a buffer this stage owns.  Rows run top-down at the output size; output scaling and the look are inherited.
 *
 * THE STREAM, in integers; tests/png_ref.py restates it in numpy and the GPU equals it byte for byte.
 * FILTER.  bpp = 3, 4 or 6 bytes per pixel, R = W bpp bytes per row.  For byte x = row[i]: a = row[i - bpp], b = above[i], c = above[i - bpp], each 0
 * left of the row or above the first row.  Candidates, mod 256: 0 None x; 1 Sub x - a; 2 Up x - b; 3 Average x - ((a + b) >> 1); 4 Paeth x - P,
 * p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|, P = a if pa <= pb and pa <= pc, else b if pb <= pc, else c.  Cost of a candidate: the sum
 * over the row of |filtered byte read as int8| (v if v < 128, else 256 - v); the lowest cost wins, ties go to the lowest type.  `filter`:
 * DE_PNG_FILTER_ADAPTIVE (default) or a fixed type 0 ... 4 for every row.  The filtered stream S is, per row, the type byte and the R filtered
 * bytes: N = H (1 + R) bytes, N <= 2^27.
 * CHUNKS.  S is cut every chunk_bytes (1024 ... 65535), the last chunk may be shorter.  Chunks are independent — no match and no run crosses a cut —
 * and are the encoder's unit of parallelism.
 * TOKENS of a chunk, left to right: at a byte v followed inside the chunk by r more equal bytes (the run is maximal): the literal v; then r / 258
 * matches (length 258, distance 1); then, with m = r mod 258, one match (m, 1) if m >= 3, else m literals v.  Last, end-of-block (256).
 * CODES.  One dynamic-Huffman block per chunk (BTYPE 10), HLIT = 29 (286 literal / length codes), HDIST = 0, HCLEN = 15.
 *   Code-length code: symbols 16, 17, 18 have length 0 and are never used; 0 ... 15 have length 4 (complete; canonical, so the code of v is v, sent
 *   most significant bit first).  The 286 literal / length lengths and the one distance length follow as 4 bits each: the header is 1222 bits.
 *   Literal / length lengths: count the chunk's symbols (256 once).  Sort the used ones ascending by (count, symbol): m >= 2 of them.  Lengths by
 *   the minimum-redundancy construction of Moffat and Katajainen on that array A[0 .. m):
 *       A[0] += A[1]; root = 0; leaf = 2;
 *       for next = 1 .. m - 2:  twice (the second time adding): take A[root] (and set A[root++] = next) if leaf >= m or — the second time only if
 *           also root < next — A[root] < A[leaf]; otherwise take A[leaf++]
 *       A[m - 2] = 0; for next = m - 3 .. 0: A[next] = A[A[next]] + 1
 *       avbl = 1, used = 0, depth = 0, root = m - 2, next = m - 1; while avbl > 0: { while root >= 0 and A[root] == depth: used++, root--;
 *           while avbl > used: A[next--] = depth, avbl--;  avbl = 2 used, depth++, used = 0 }
 *   Limit: n[l] = the number of lengths l, those above 15 counted at 15; K = sum n[l] << (15 - l); while K != 2^15: n[15]--, the largest l < 15
 *   with n[l] > 0 gives one up (n[l]--, n[l + 1] += 2), K--.  Hand out: lengths 1, 2, ... 15 in turn, n[l] of each, to the sorted symbols from the
 *   LAST (the most frequent) backwards.  Codes: canonical (RFC 1951 §3.2.2).  The distance code: one code, length 1 if the chunk holds a match, else 0;
 *   a match's distance is the single bit 0.
 *   If the dynamic block — ceil((1222 + the tokens' bits) / 8) bytes — is not shorter than the stored block's n + 5 bytes, the stored block (BTYPE 00)
 *   is written instead: this makes the capacity a proof.
 * ALIGNMENT.  Every chunk starts on a byte.  Behind every chunk but the last stands an empty stored block (BFINAL 0, BTYPE 00, padding to the byte,
 * LEN 0, NLEN 0xFFFF).  The last chunk's block has BFINAL 1 and is zero-padded.
 * ZLIB AND PNG FRAMING.  CMF / FLG 78 01 in front of the first chunk.  Each chunk's deflate data is one IDAT, whose CRC-32 the workgroup that wrote
 * it computes.  The Adler-32 of S — per-chunk partials combined on the device — is the data of one more IDAT of 4 bytes, then IEND: a trailer of
 * 28 bytes.  The front is the host's, once per setting and size: signature, IHDR (width, height, depth, colour type, 0, 0, 0) and, for depth 16,
 * cICP {primaries, transfer, 0, 1} exactly as the HDR screenshots carry it (primaries 1 / 12 / 9 for Rec.709 / P3-D65 / Rec.2020, transfer 8 / 16 / 18
 * for linear / PQ / HLG): 33 or 49 bytes.
 * THE LENGTH leaves the device with the file, as the JPEG stream's does: on the device the file is preceded by a 16-byte word {uint64 length,
 * uint32 status, uint32 chunks}.  de_png_capacity = front + N + 24 per chunk + 28 is the proven bound (a chunk of n bytes: 12 of IDAT framing, 2 of
 * CMF / FLG, n + 5 stored, 5 for the empty stored block): a store past a chunk's slot or past the capacity is not made and ends the conversion with
 * DE_ERR_INTERNAL.
 * DE_PNG_DEFAULT_CHUNK = 32768 is the candidate among {4096, 8192, 16384, 32768, 65535} with the lowest encode time at 1920 x 1080 whose file is at
 * most 1 % longer than the 65535-byte-chunk file of the same frame, for the default source (RGBA8) and for RGB16; for RGB8 the rule gives 16384
 * (15 % faster, 0.6 % longer): the table measured on an MI355X in profiles/png.md.
 * OUT OF SCOPE: LZ77 beyond distance 1, palette and grey types, interlace, 10-bit packing, sRGB / gAMA / iCCP / text chunks, APNG.
 *
 * The conversion runs on the context stream with no host synchronisation in it.  Every other fetch and its buffers are untouched; the PNG fetches
 * have device buffers, a pinned staging buffer and a four-deep pinned ring of their own, all allocated on first use.  With none of the calls below
 * made, nothing is allocated and nothing runs.
 */
#ifndef DIGITAL_EARTH_PNG_H
#define DIGITAL_EARTH_PNG_H
#include "digital_earth_jpeg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_PNG_SOURCE_PIXELS 0
#define DE_PNG_SOURCE_HDR_PIXELS 1
#define DE_PNG_FILTER_NONE 0
#define DE_PNG_FILTER_SUB 1
#define DE_PNG_FILTER_UP 2
#define DE_PNG_FILTER_AVERAGE 3
#define DE_PNG_FILTER_PAETH 4
#define DE_PNG_FILTER_ADAPTIVE 5
#define DE_PNG_DEFAULT_CHUNK 32768     /* filtered bytes per deflate chunk: measured, profiles/png.md */

typedef struct de_png {
    uint32_t struct_bytes;               /* sizeof(de_png) of the caller; checked like de_pixels */
    int32_t source;                      /* DE_PNG_SOURCE_*; default DE_PNG_SOURCE_PIXELS */
    int32_t filter;                      /* DE_PNG_FILTER_*; default DE_PNG_FILTER_ADAPTIVE */
    int32_t chunk_bytes;                 /* 1024 ... 65535; default DE_PNG_DEFAULT_CHUNK */
} de_png;

/* Set the source, the filter and the chunk size.  DE_ERR_INVALID: a value out of range, a mismatched struct_bytes; DE_ERR_STATE while PNG fetches
 * are in flight (de_fetch_png_begin without its _end).  A refused call changes nothing. */
int de_set_png(de_ctx* ctx, const de_png* settings);
/* The current settings (before any de_set_png: the defaults above). */
int de_get_png(de_ctx* ctx, de_png* out);
/* The proven upper bound of any frame's length at the current settings and output size.  DE_ERR_STATE: the HDR source without RGB16 HDR output. */
int de_png_capacity(de_ctx* ctx, uint64_t* bytes);
/* de_render_to_image, the pack and the conversion behind it on the context stream; the file stays on the device (valid until the next conversion),
 * its length in the uint64 at *device_len (may be NULL), 16 bytes in front of it.  Nothing is waited for. */
int de_render_to_png(de_ctx* ctx, const void** device_stream, const uint64_t** device_len);
/* The frame as it stands into `out`.  *len is the file's length either way; DE_ERR_INVALID if out_bytes is smaller (nothing is copied into `out`). */
int de_fetch_png(de_ctx* ctx, void* out, uint64_t out_bytes, uint64_t* len);
/* The same without the last host copy: *host = the library's pinned PNG staging buffer, valid until the next de_fetch_png or de_fetch_png_view. */
int de_fetch_png_view(de_ctx* ctx, const void** host, uint64_t* len);
/* The recording loop pipelined, as de_fetch_jpeg_begin / _end, through a ring of four of its own: _begin enqueues the display, the conversion and
 * the copy of the file's front part and returns at once; _end waits for the oldest PNG fetch begun, copies what the front part did not hold (it
 * grows with the frames) and hands out its buffer, valid until the ring comes round to it.  DE_ERR_STATE: a fifth _begin without an _end, an _end
 * without a _begin. */
int de_fetch_png_begin(de_ctx* ctx);
int de_fetch_png_end(de_ctx* ctx, const void** host, uint64_t* len);
/* The conversion once on host-given PACKED pixels, free of the display: `pixels` is [H][W][channels] samples of `depth` bits (8: bytes; 16: uint16
 * in the host's byte order, as de_fetch_hdr_pixels hands them out), channels 3 or 4 at depth 8 and 3 at depth 16, any W, H >= 1 with
 * H (1 + W bpp) <= 2^27 (DE_ERR_INVALID otherwise).  settings->source is not read; depth 16 carries cICP {1, 8, 0, 1}.  Buffers of its own. */
int de_debug_png(de_ctx* ctx, const void* pixels, int W, int H, int channels, int depth, const de_png* settings, void* out, uint64_t out_bytes, uint64_t* len);
/* The host's part alone, no device and no context: the front of a W x H file into `out` (*len = 33 or 49; DE_ERR_INVALID and nothing written if
 * out_bytes is smaller; out may be NULL with out_bytes 0) and the capacity de_png_capacity would answer.  cicp: four bytes for depth 16 (NULL:
 * {1, 8, 0, 1}).  Refuses what de_set_png and de_debug_png refuse. */
int de_debug_png_framing(const de_png* settings, int W, int H, int channels, int depth, const uint8_t* cicp, void* out, uint64_t out_bytes, uint64_t* len, uint64_t* capacity);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_PNG_H */

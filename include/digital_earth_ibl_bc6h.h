/* digital_earth_ibl_bc6h.h — opt-in BC6H_UF16 compression of the IBL output of libdigitalearth_hip.so: the cube chain of include/digital_earth_ibl.h
 * as one DDS file at 1 byte per texel, encoded on the GPU (same library, ABI 6, additions only).  Off, the default, nothing is allocated
 * or run and every other call returns the bytes it returned before this header existed.
 *
 * ARITHMETIC.  Integers only from the first step on; digital_earth_amd/bc6h.py restates the decoder and the encoder in numpy, and the GPU equals the
 * restatement byte for byte.
 *
 * TEXEL TO HALF.  A float32 channel becomes digital_earth_exr.h's HALF (NaN to 0, clamped to 65504, nearest even); then a set sign bit gives 0.  From
 * here on a texel is three integers in 0 ... 0x7BFF.
 *
 * BLOCK.  A level of edge e is cut into 4 x 4 texels, rows top first, texel t = 4 row + column; texel coordinates are clamped to e - 1, so the levels
 * of edge 2 and 1 fill one block by replication.  A face of a level stores max(1, e / 4)^2 blocks of 16 bytes, rows of blocks top first.  A block is
 * one 128-bit little-endian number; bit 0 is the lowest bit of byte 0.
 *
 * DECODING.  The mode is bits 0 ... 1 if they are 00 (mode 1) or 01 (mode 2), else bits 0 ... 4: 00010 mode 3, 00110 4, 01010 5, 01110 6, 10010 7,
 * 10110 8, 11010 9, 11110 10, 00011 11, 00111 12, 01011 13, 01111 14 (written highest bit first); 10011, 10111, 11011, 11111 are reserved and decode to
 * 0 in every texel.  Behind the mode bits the fields follow in this order (R G B: the channel; W X: the two ends of region 0, Y Z: of region 1; D:
 * the partition; a-b: bits a ... b of the field, in that order):
 *    1  p 10, deltas 5 5 5:  GY4 BY4 BZ4 RW0-9 GW0-9 BW0-9 RX0-4 GZ4 GY0-3 GX0-4 BZ0 GZ0-3 BX0-4 BZ1 BY0-3 RY0-4 BZ2 RZ0-4 BZ3 D0-4
 *    2  p 7,  deltas 6 6 6:  GY5 GZ4 GZ5 RW0-6 BZ0 BZ1 BY4 GW0-6 BY5 BZ2 GY4 BW0-6 BZ3 BZ5 BZ4 RX0-5 GY0-3 GX0-5 GZ0-3 BX0-5 BY0-3 RY0-5 RZ0-5 D0-4
 *    3  p 11, deltas 5 4 4:  RW0-9 GW0-9 BW0-9 RX0-4 RW10 GY0-3 GX0-3 GW10 BZ0 GZ0-3 BX0-3 BW10 BZ1 BY0-3 RY0-4 BZ2 RZ0-4 BZ3 D0-4
 *    4  p 11, deltas 4 5 4:  RW0-9 GW0-9 BW0-9 RX0-3 RW10 GZ4 GY0-3 GX0-4 GW10 GZ0-3 BX0-3 BW10 BZ1 BY0-3 RY0-3 BZ0 BZ2 RZ0-3 GY4 BZ3 D0-4
 *    5  p 11, deltas 4 4 5:  RW0-9 GW0-9 BW0-9 RX0-3 RW10 BY4 GY0-3 GX0-3 GW10 BZ0 GZ0-3 BX0-4 BW10 BY0-3 RY0-3 BZ1 BZ2 RZ0-3 BZ4 BZ3 D0-4
 *    6  p 9,  deltas 5 5 5:  RW0-8 BY4 GW0-8 GY4 BW0-8 BZ4 RX0-4 GZ4 GY0-3 GX0-4 BZ0 GZ0-3 BX0-4 BZ1 BY0-3 RY0-4 BZ2 RZ0-4 BZ3 D0-4
 *    7  p 8,  deltas 6 5 5:  RW0-7 GZ4 BY4 GW0-7 BZ2 GY4 BW0-7 BZ3 BZ4 RX0-5 GY0-3 GX0-4 BZ0 GZ0-3 BX0-4 BZ1 BY0-3 RY0-5 RZ0-5 D0-4
 *    8  p 8,  deltas 5 6 5:  RW0-7 BZ0 BY4 GW0-7 GY5 GY4 BW0-7 GZ5 BZ4 RX0-4 GZ4 GY0-3 GX0-5 GZ0-3 BX0-4 BZ1 BY0-3 RY0-4 BZ2 RZ0-4 BZ3 D0-4
 *    9  p 8,  deltas 5 5 6:  RW0-7 BZ1 BY4 GW0-7 BY5 GY4 BW0-7 BZ5 BZ4 RX0-4 GZ4 GY0-3 GX0-4 BZ0 GZ0-3 BX0-5 BY0-3 RY0-4 BZ2 RZ0-4 BZ3 D0-4
 *   10  p 6,  direct:        RW0-5 GZ4 BZ0 BZ1 BY4 GW0-5 GY5 BY5 BZ2 GY4 BW0-5 GZ5 BZ3 BZ5 BZ4 RX0-5 GY0-3 GX0-5 GZ0-3 BX0-5 BY0-3 RY0-5 RZ0-5 D0-4
 *   11  p 10, direct:        RW0-9 GW0-9 BW0-9 RX0-9 GX0-9 BX0-9
 *   12  p 11, deltas 9 9 9:  RW0-9 GW0-9 BW0-9 RX0-8 RW10 GX0-8 GW10 BX0-8 BW10
 *   13  p 12, deltas 8 8 8:  RW0-9 GW0-9 BW0-9 RX0-7 RW11-10 GX0-7 GW11-10 BX0-7 BW11-10
 *   14  p 16, deltas 4 4 4:  RW0-9 GW0-9 BW0-9 RX0-3 RW15-10 GX0-3 GW15-10 BX0-3 BW15-10
 * Modes 1 - 10 have two regions, 82 bits in front of 46 index bits; modes 11 - 14 one region, 65 bits in front of 63.  In a mode with deltas, X, Y, Z
 * are sign-extended from their field's width, added to W of the same channel, and the sum WRAPS: it is taken modulo 2^p.
 *   THE 32 PARTITIONS, the region of texels 0 ... 15, and the ANCHOR texel of region 1 (region 0's anchor is texel 0):
 *     0 0011001100110011 15    1 0001000100010001 15    2 0111011101110111 15    3 0001001100110111 15    4 0000000100010011 15    5 0011011101111111 15
 *     6 0001001101111111 15    7 0000000100110111 15    8 0000000000010011 15    9 0011011111111111 15   10 0000000101111111 15   11 0000000000010111 15
 *    12 0001011111111111 15   13 0000000011111111 15   14 0000111111111111 15   15 0000000000001111 15   16 0000100011101111 15   17 0111000100000000 2
 *    18 0000000010001110 8    19 0111001100010000 2    20 0011000100000000 2    21 0000100011001110 8    22 0000000010001100 8    23 0111001100110001 15
 *    24 0011000100010000 2    25 0000100010001100 8    26 0110011001100110 2    27 0011011001101100 2    28 0001011111101000 8    29 0000111111110000 8
 *    30 0111000110001110 2    31 0011100110011100 2
 *   INDICES, texel 0 first, lowest bit first: 3 bits a texel with two regions, 4 with one; an anchor texel stores one bit less, its top bit being 0.
 *   UNQUANTISATION of an unsigned value x of p bits: p >= 15 gives x; 0 gives 0; all ones gives 0xFFFF; otherwise ((x << 16) + 0x8000) >> p.
 *   INTERPOLATION between the unquantised ends a, b of the texel's region: (a (64 - w) + b w + 32) >> 6 with w = {0, 9, 18, 27, 37, 46, 55, 64}[index]
 *   for 3-bit and {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64}[index] for 4-bit indices.  THE FINAL STEP: (v 31) >> 6, a half's bits.
 *
 * ENCODING, for one block and one candidate given by its regions and the ends' precision p:
 *   1. ENDS.  Per region the ends are the per-channel minimum (first end) and maximum (second end) of the half integers.  Then the diagonal: with
 *      the sums over the region's n texels, n sum(R G) - sum(R) sum(G) in 64 bits; if it is negative G's two ends are exchanged.  The same for B
 *      against R.
 *   2. QUANTISE.  q = ((h 64) / 31) >> (16 - p), capped at 2^p - 1.  Black (0) and 0x7BFF come back exactly at every p: 0 stays 0, and 0x7BFF gives
 *      65534 >> (16 - p) = all ones, which unquantises to 0xFFFF and ends as (0xFFFF 31) >> 6 = 0x7BFF.
 *   3. INDICES.  The palette is made from the unquantised ends by the decoder's interpolation and final step.  Every texel takes the entry of least
 *      sum over the three channels of (decoded - texel)^2, in integers; ties go to the lower index.  The candidate's error is the sum over the texels.
 *   4. ANCHORS.  If a region's anchor texel has the top bit of its index set, that region's ends are exchanged and its indices complemented
 *      (the weights are symmetric: the decoded block does not change).
 *   5. TRANSFORMED MODES.  A mode with deltas is feasible only if every X, Y, Z minus W of its channel, after step 4, fits the signed field:
 *      -2^(d - 1) ... 2^(d - 1) - 1.  A feasible candidate decodes exactly as computed, so the error is computed once per (partition, p).
 *   CANDIDATES.  quality 0: mode 11 alone (one region, p = 10, 4-bit indices).  quality 1: mode 11, and for each of the 32 partitions the feasible
 *   mode of highest precision among mode 1 (p 10), mode 6 (p 9), mode 2 (p 7) and mode 10 (p 6, direct, always feasible).  The block takes the
 *   candidate of least error; ties go to mode 11, then to the lower partition.
 *
 * THE FILE: digital_earth_ibl.h's 148 bytes with DXGI format 95 (BC6H_UF16), flags 0x000A1007 (LINEARSIZE 0x00080000 in place of PITCH 0x8) and
 * pitchOrLinearSize = the bytes of level 0 of one face, 16 (E / 4)^2; then the blocks, face-major, each face followed by its L levels.
 *
 * LIMITS.  Unsigned only (BC6H_UF16).  The one-region delta modes 12 - 14 (and 3 - 5, 7 - 9) are decoded by the readers but never emitted.  The ends
 * are the box's diagonal; there is no least-squares refinement.  No KTX2 container.  The seams of the rough levels are inherited from the chain.
 */
#ifndef DIGITAL_EARTH_IBL_BC6H_H
#define DIGITAL_EARTH_IBL_BC6H_H
#include "digital_earth_ibl.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_IBL_BC6H_DXGI_FORMAT 95

typedef struct de_ibl_bc6h {
    uint32_t struct_bytes;               /* sizeof(de_ibl_bc6h) of the caller */
    int32_t on;                          /* 0 (default) or 1 */
    int32_t quality;                     /* 0 (default): mode 11 alone; 1: the two-region candidates as well */
} de_ibl_bc6h;

/* DE_ERR_INVALID: a mismatched struct_bytes or a field outside the table above.  A call that succeeds drops the blocks an earlier fetch made.  A
 * refused call changes nothing.  Nothing is allocated here. */
int de_set_ibl_bc6h(de_ctx* ctx, const de_ibl_bc6h* settings);
/* The current settings (before any de_set_ibl_bc6h: off, quality 0). */
int de_get_ibl_bc6h(de_ctx* ctx, de_ibl_bc6h* out);
/* The compressed file's length under the current de_ibl settings: 148 + 96 times the sum over the levels of max(1, e / 4)^2.  No build is needed. */
int de_ibl_bc6h_file_bytes(de_ctx* ctx, uint64_t* bytes);
/* The whole file into `out` (out_bytes of room, at least de_ibl_bc6h_file_bytes: DE_ERR_INVALID otherwise).  DE_ERR_STATE before a de_ibl_build under
 * the current IBL settings, or with the stage off.  The blocks are made by the first fetch after a build and kept until the next de_ibl_build,
 * de_set_ibl or de_set_ibl_bc6h. */
int de_fetch_ibl_bc6h_dds(de_ctx* ctx, void* out, uint64_t out_bytes);
/* The encoder alone on a host-given image rgb[h][w][3], any w, h in 1 ... 16384, clamped as a level is: ceil(w / 4) ceil(h / 4) blocks into `blocks`
 * (`bytes` of room: DE_ERR_INVALID if too few).  `settings`: quality is used, `on` is checked and not used.  Buffers of its own; every refusal
 * answers before the context is read. */
int de_debug_bc6h_encode(de_ctx* ctx, const float* rgb, int w, int h, const de_ibl_bc6h* settings, void* blocks, uint64_t bytes);
/* de_debug_ibl with a compressed file out: the bake once on six host-given linear faces, then the encoder.  Each output may be NULL: sh[27]; levels
 * (float32, level-major, as de_debug_ibl); half_levels: the same texels as half integers, uint16, same order: what the blocks encode; dds with
 * dds_bytes of room.  The context's settings, slots and product are untouched.  Every argument and setting refusal answers before the context is
 * read. */
int de_debug_ibl_bc6h(de_ctx* ctx, const float* faces, int n, const de_panorama* panorama, const de_ibl* ibl, const de_ibl_bc6h* settings, float* sh, float* levels, uint16_t* half_levels, void* dds, uint64_t dds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_IBL_BC6H_H */

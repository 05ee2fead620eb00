// bc6h_tables.h — the tables of BC6H_UF16 (include/digital_earth_ibl_bc6h.h) and the host side of the compressed IBL file, plain C++ with
// no HIP in it: the 32 two-region partitions as bitmaps, their anchors, the interpolation weights, one field-layout table per mode (read by the packer
// of bc6h_body.h), the geometry of the file and its front.  tools/bc6h_host_check.cpp compiles it with bc6h_body.h under the sanitizers and prints the
// layouts bit by bit; tests/test_ibl_bc6h_abi.py holds that print against digital_earth_amd/bc6h.py's tables, which were written on their own.
// Every table is a constant expression: device code reads it from constant memory at wave-uniform or near-uniform addresses.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "ibl_tables.h"

#define BC6H_DXGI_FORMAT 95u
#define BC6H_HALF_MAX 0x7BFFu
#define BC6H_MAX_IMAGES IBL_MAX_LEVELS

// bit t of entry k: the region of texel t = 4 row + column under partition k
static constexpr uint16_t BC6H_PARTITION[32] = {
    0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
    0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C};
// the anchor texel of region 1 (region 0's is texel 0)
static constexpr uint8_t BC6H_ANCHOR[32] = {15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2};
static constexpr uint8_t BC6H_WEIGHT3[8] = {0, 9, 18, 27, 37, 46, 55, 64};
static constexpr uint8_t BC6H_WEIGHT4[16] = {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64};

// mode m = 1 ... 14 at [m - 1]: the mode bits' value and count, the ends' precision, the delta bits of R G B (0: direct ends), the regions
struct Bc6hMode { uint8_t value, count, precision, delta[3], regions; };
static constexpr Bc6hMode BC6H_MODE[14] = {
    {0, 2, 10, {5, 5, 5}, 2}, {1, 2, 7, {6, 6, 6}, 2}, {2, 5, 11, {5, 4, 4}, 2}, {6, 5, 11, {4, 5, 4}, 2}, {10, 5, 11, {4, 4, 5}, 2}, {14, 5, 9, {5, 5, 5}, 2},
    {18, 5, 8, {6, 5, 5}, 2}, {22, 5, 8, {5, 6, 5}, 2}, {26, 5, 8, {5, 5, 6}, 2}, {30, 5, 6, {0, 0, 0}, 2},
    {3, 5, 10, {0, 0, 0}, 1}, {7, 5, 11, {9, 9, 9}, 1}, {11, 5, 12, {8, 8, 8}, 1}, {15, 5, 16, {4, 4, 4}, 1}};

// The fields: end e = 0 ... 3 (W X of region 0, Y Z of region 1) of channel c at 3 e + c; D the partition.
enum { BC6H_RW, BC6H_GW, BC6H_BW, BC6H_RX, BC6H_GX, BC6H_BX, BC6H_RY, BC6H_GY, BC6H_BY, BC6H_RZ, BC6H_GZ, BC6H_BZ, BC6H_D };
// One run of a layout: `count` bits of `field` from bit `low` upwards (reversed: from low + count - 1 downwards), at the next free bits of the block.
#define BC6H_F(field, low, count) (uint16_t)((field) | ((low) << 4) | ((count) << 8))
#define BC6H_FR(field, low, count) (uint16_t)(BC6H_F(field, low, count) | 0x1000)
#define BC6H_LAYOUT_RUNS 26
// behind the mode bits, in file order; a zero ends the list
static constexpr uint16_t BC6H_LAYOUT[14][BC6H_LAYOUT_RUNS] = {
    /* 1 */ {BC6H_F(BC6H_GY, 4, 1), BC6H_F(BC6H_BY, 4, 1), BC6H_F(BC6H_BZ, 4, 1), BC6H_F(BC6H_RW, 0, 10), BC6H_F(BC6H_GW, 0, 10), BC6H_F(BC6H_BW, 0, 10), BC6H_F(BC6H_RX, 0, 5),
             BC6H_F(BC6H_GZ, 4, 1), BC6H_F(BC6H_GY, 0, 4), BC6H_F(BC6H_GX, 0, 5), BC6H_F(BC6H_BZ, 0, 1), BC6H_F(BC6H_GZ, 0, 4), BC6H_F(BC6H_BX, 0, 5), BC6H_F(BC6H_BZ, 1, 1),
             BC6H_F(BC6H_BY, 0, 4), BC6H_F(BC6H_RY, 0, 5), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_RZ, 0, 5), BC6H_F(BC6H_BZ, 3, 1), BC6H_F(BC6H_D, 0, 5)},
    /* 2 */ {BC6H_F(BC6H_GY, 5, 1), BC6H_F(BC6H_GZ, 4, 1), BC6H_F(BC6H_GZ, 5, 1), BC6H_F(BC6H_RW, 0, 7), BC6H_F(BC6H_BZ, 0, 1), BC6H_F(BC6H_BZ, 1, 1), BC6H_F(BC6H_BY, 4, 1),
             BC6H_F(BC6H_GW, 0, 7), BC6H_F(BC6H_BY, 5, 1), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_GY, 4, 1), BC6H_F(BC6H_BW, 0, 7), BC6H_F(BC6H_BZ, 3, 1), BC6H_F(BC6H_BZ, 5, 1),
             BC6H_F(BC6H_BZ, 4, 1), BC6H_F(BC6H_RX, 0, 6), BC6H_F(BC6H_GY, 0, 4), BC6H_F(BC6H_GX, 0, 6), BC6H_F(BC6H_GZ, 0, 4), BC6H_F(BC6H_BX, 0, 6), BC6H_F(BC6H_BY, 0, 4),
             BC6H_F(BC6H_RY, 0, 6), BC6H_F(BC6H_RZ, 0, 6), BC6H_F(BC6H_D, 0, 5)},
    /* 3 */ {BC6H_F(BC6H_RW, 0, 10), BC6H_F(BC6H_GW, 0, 10), BC6H_F(BC6H_BW, 0, 10), BC6H_F(BC6H_RX, 0, 5), BC6H_F(BC6H_RW, 10, 1), BC6H_F(BC6H_GY, 0, 4), BC6H_F(BC6H_GX, 0, 4),
             BC6H_F(BC6H_GW, 10, 1), BC6H_F(BC6H_BZ, 0, 1), BC6H_F(BC6H_GZ, 0, 4), BC6H_F(BC6H_BX, 0, 4), BC6H_F(BC6H_BW, 10, 1), BC6H_F(BC6H_BZ, 1, 1), BC6H_F(BC6H_BY, 0, 4),
             BC6H_F(BC6H_RY, 0, 5), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_RZ, 0, 5), BC6H_F(BC6H_BZ, 3, 1), BC6H_F(BC6H_D, 0, 5)},
    /* 4 */ {BC6H_F(BC6H_RW, 0, 10), BC6H_F(BC6H_GW, 0, 10), BC6H_F(BC6H_BW, 0, 10), BC6H_F(BC6H_RX, 0, 4), BC6H_F(BC6H_RW, 10, 1), BC6H_F(BC6H_GZ, 4, 1), BC6H_F(BC6H_GY, 0, 4),
             BC6H_F(BC6H_GX, 0, 5), BC6H_F(BC6H_GW, 10, 1), BC6H_F(BC6H_GZ, 0, 4), BC6H_F(BC6H_BX, 0, 4), BC6H_F(BC6H_BW, 10, 1), BC6H_F(BC6H_BZ, 1, 1), BC6H_F(BC6H_BY, 0, 4),
             BC6H_F(BC6H_RY, 0, 4), BC6H_F(BC6H_BZ, 0, 1), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_RZ, 0, 4), BC6H_F(BC6H_GY, 4, 1), BC6H_F(BC6H_BZ, 3, 1), BC6H_F(BC6H_D, 0, 5)},
    /* 5 */ {BC6H_F(BC6H_RW, 0, 10), BC6H_F(BC6H_GW, 0, 10), BC6H_F(BC6H_BW, 0, 10), BC6H_F(BC6H_RX, 0, 4), BC6H_F(BC6H_RW, 10, 1), BC6H_F(BC6H_BY, 4, 1), BC6H_F(BC6H_GY, 0, 4),
             BC6H_F(BC6H_GX, 0, 4), BC6H_F(BC6H_GW, 10, 1), BC6H_F(BC6H_BZ, 0, 1), BC6H_F(BC6H_GZ, 0, 4), BC6H_F(BC6H_BX, 0, 5), BC6H_F(BC6H_BW, 10, 1), BC6H_F(BC6H_BY, 0, 4),
             BC6H_F(BC6H_RY, 0, 4), BC6H_F(BC6H_BZ, 1, 1), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_RZ, 0, 4), BC6H_F(BC6H_BZ, 4, 1), BC6H_F(BC6H_BZ, 3, 1), BC6H_F(BC6H_D, 0, 5)},
    /* 6 */ {BC6H_F(BC6H_RW, 0, 9), BC6H_F(BC6H_BY, 4, 1), BC6H_F(BC6H_GW, 0, 9), BC6H_F(BC6H_GY, 4, 1), BC6H_F(BC6H_BW, 0, 9), BC6H_F(BC6H_BZ, 4, 1), BC6H_F(BC6H_RX, 0, 5),
             BC6H_F(BC6H_GZ, 4, 1), BC6H_F(BC6H_GY, 0, 4), BC6H_F(BC6H_GX, 0, 5), BC6H_F(BC6H_BZ, 0, 1), BC6H_F(BC6H_GZ, 0, 4), BC6H_F(BC6H_BX, 0, 5), BC6H_F(BC6H_BZ, 1, 1),
             BC6H_F(BC6H_BY, 0, 4), BC6H_F(BC6H_RY, 0, 5), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_RZ, 0, 5), BC6H_F(BC6H_BZ, 3, 1), BC6H_F(BC6H_D, 0, 5)},
    /* 7 */ {BC6H_F(BC6H_RW, 0, 8), BC6H_F(BC6H_GZ, 4, 1), BC6H_F(BC6H_BY, 4, 1), BC6H_F(BC6H_GW, 0, 8), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_GY, 4, 1), BC6H_F(BC6H_BW, 0, 8),
             BC6H_F(BC6H_BZ, 3, 1), BC6H_F(BC6H_BZ, 4, 1), BC6H_F(BC6H_RX, 0, 6), BC6H_F(BC6H_GY, 0, 4), BC6H_F(BC6H_GX, 0, 5), BC6H_F(BC6H_BZ, 0, 1), BC6H_F(BC6H_GZ, 0, 4),
             BC6H_F(BC6H_BX, 0, 5), BC6H_F(BC6H_BZ, 1, 1), BC6H_F(BC6H_BY, 0, 4), BC6H_F(BC6H_RY, 0, 6), BC6H_F(BC6H_RZ, 0, 6), BC6H_F(BC6H_D, 0, 5)},
    /* 8 */ {BC6H_F(BC6H_RW, 0, 8), BC6H_F(BC6H_BZ, 0, 1), BC6H_F(BC6H_BY, 4, 1), BC6H_F(BC6H_GW, 0, 8), BC6H_F(BC6H_GY, 5, 1), BC6H_F(BC6H_GY, 4, 1), BC6H_F(BC6H_BW, 0, 8),
             BC6H_F(BC6H_GZ, 5, 1), BC6H_F(BC6H_BZ, 4, 1), BC6H_F(BC6H_RX, 0, 5), BC6H_F(BC6H_GZ, 4, 1), BC6H_F(BC6H_GY, 0, 4), BC6H_F(BC6H_GX, 0, 6), BC6H_F(BC6H_GZ, 0, 4),
             BC6H_F(BC6H_BX, 0, 5), BC6H_F(BC6H_BZ, 1, 1), BC6H_F(BC6H_BY, 0, 4), BC6H_F(BC6H_RY, 0, 5), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_RZ, 0, 5), BC6H_F(BC6H_BZ, 3, 1),
             BC6H_F(BC6H_D, 0, 5)},
    /* 9 */ {BC6H_F(BC6H_RW, 0, 8), BC6H_F(BC6H_BZ, 1, 1), BC6H_F(BC6H_BY, 4, 1), BC6H_F(BC6H_GW, 0, 8), BC6H_F(BC6H_BY, 5, 1), BC6H_F(BC6H_GY, 4, 1), BC6H_F(BC6H_BW, 0, 8),
             BC6H_F(BC6H_BZ, 5, 1), BC6H_F(BC6H_BZ, 4, 1), BC6H_F(BC6H_RX, 0, 5), BC6H_F(BC6H_GZ, 4, 1), BC6H_F(BC6H_GY, 0, 4), BC6H_F(BC6H_GX, 0, 5), BC6H_F(BC6H_BZ, 0, 1),
             BC6H_F(BC6H_GZ, 0, 4), BC6H_F(BC6H_BX, 0, 6), BC6H_F(BC6H_BY, 0, 4), BC6H_F(BC6H_RY, 0, 5), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_RZ, 0, 5), BC6H_F(BC6H_BZ, 3, 1),
             BC6H_F(BC6H_D, 0, 5)},
    /* 10 */ {BC6H_F(BC6H_RW, 0, 6), BC6H_F(BC6H_GZ, 4, 1), BC6H_F(BC6H_BZ, 0, 1), BC6H_F(BC6H_BZ, 1, 1), BC6H_F(BC6H_BY, 4, 1), BC6H_F(BC6H_GW, 0, 6), BC6H_F(BC6H_GY, 5, 1),
              BC6H_F(BC6H_BY, 5, 1), BC6H_F(BC6H_BZ, 2, 1), BC6H_F(BC6H_GY, 4, 1), BC6H_F(BC6H_BW, 0, 6), BC6H_F(BC6H_GZ, 5, 1), BC6H_F(BC6H_BZ, 3, 1), BC6H_F(BC6H_BZ, 5, 1),
              BC6H_F(BC6H_BZ, 4, 1), BC6H_F(BC6H_RX, 0, 6), BC6H_F(BC6H_GY, 0, 4), BC6H_F(BC6H_GX, 0, 6), BC6H_F(BC6H_GZ, 0, 4), BC6H_F(BC6H_BX, 0, 6), BC6H_F(BC6H_BY, 0, 4),
              BC6H_F(BC6H_RY, 0, 6), BC6H_F(BC6H_RZ, 0, 6), BC6H_F(BC6H_D, 0, 5)},
    /* 11 */ {BC6H_F(BC6H_RW, 0, 10), BC6H_F(BC6H_GW, 0, 10), BC6H_F(BC6H_BW, 0, 10), BC6H_F(BC6H_RX, 0, 10), BC6H_F(BC6H_GX, 0, 10), BC6H_F(BC6H_BX, 0, 10)},
    /* 12 */ {BC6H_F(BC6H_RW, 0, 10), BC6H_F(BC6H_GW, 0, 10), BC6H_F(BC6H_BW, 0, 10), BC6H_F(BC6H_RX, 0, 9), BC6H_F(BC6H_RW, 10, 1), BC6H_F(BC6H_GX, 0, 9), BC6H_F(BC6H_GW, 10, 1),
              BC6H_F(BC6H_BX, 0, 9), BC6H_F(BC6H_BW, 10, 1)},
    /* 13 */ {BC6H_F(BC6H_RW, 0, 10), BC6H_F(BC6H_GW, 0, 10), BC6H_F(BC6H_BW, 0, 10), BC6H_F(BC6H_RX, 0, 8), BC6H_FR(BC6H_RW, 10, 2), BC6H_F(BC6H_GX, 0, 8), BC6H_FR(BC6H_GW, 10, 2),
              BC6H_F(BC6H_BX, 0, 8), BC6H_FR(BC6H_BW, 10, 2)},
    /* 14 */ {BC6H_F(BC6H_RW, 0, 10), BC6H_F(BC6H_GW, 0, 10), BC6H_F(BC6H_BW, 0, 10), BC6H_F(BC6H_RX, 0, 4), BC6H_FR(BC6H_RW, 10, 6), BC6H_F(BC6H_GX, 0, 4), BC6H_FR(BC6H_GW, 10, 6),
              BC6H_F(BC6H_BX, 0, 4), BC6H_FR(BC6H_BW, 10, 6)}};

// ---- the file: the blocks of one face of a level of edge e, and of the chain
static inline uint32_t bc6h_level_blocks(int e) { const uint32_t n = e >= 4 ? (uint32_t)e / 4u : 1u; return n * n; }
static inline uint32_t bc6h_face_blocks(int E, int L) { uint32_t s = 0; for (int l = 0; l < L; ++l) s += bc6h_level_blocks(E >> l); return s; }
static inline size_t bc6h_payload_bytes(int E, int L) { return (size_t)bc6h_face_blocks(E, L) * 6 * 16; }
// nullptr: the settings are in range (struct_bytes is the caller's to compare)
static inline const char* bc6h_settings_fault(int on, int quality) {
    if (on != 0 && on != 1) return "de_ibl_bc6h.on must be 0 or 1";
    if (quality != 0 && quality != 1) return "de_ibl_bc6h.quality must be 0 or 1";
    return nullptr;
}
// The 148 bytes in front of the blocks: ibl_dds_header's with DXGI format 95, LINEARSIZE for PITCH and the byte size of level 0 of one face.
static inline void bc6h_dds_header(int E, int L, uint8_t* out) {
    ibl_dds_header(E, L, IBL_PIXEL_HALF, out);
    const uint32_t flags = 0x000A1007u, linear = 16u * bc6h_level_blocks(E), format = BC6H_DXGI_FORMAT;
    const uint32_t at[3] = {2, 5, 32}, v[3] = {flags, linear, format};
    for (int k = 0; k < 3; ++k) for (int b = 0; b < 4; ++b) out[4 * at[k] + (uint32_t)b] = (uint8_t)(v[k] >> (8 * b));
}

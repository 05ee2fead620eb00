// jpeg_tables.h — the host side of the JPEG output (include/digital_earth_jpeg.h), plain C++ with no HIP in it: the tables of ITU-T T.81
// Annex K, the IJG quality rule, the integer DCT matrix, the Huffman codes the kernels look up, the geometry (MCUs, intervals, the worst-case slot and
// the capacity) and the framing that de_set_jpeg writes once.  jpeg_kernels.hip's header derives the worst case these sizes come from.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define JP_BLOCK_BITS 1660           // worst case of one block before stuffing: 22 (DC) + 63 * 26 (AC): jpeg_kernels.hip
#define JP_FRAMING_BYTES 629         // SOI .. SOS: jp_write_framing answers it

// zigzag position k -> natural index v * 8 + u (T.81 Figure 5)
static const uint8_t JP_ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1 (luminance) and K.2 (chrominance), natural order
static const uint8_t JP_BASE_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3 - K.6: BITS (codes of length 1 .. 16) and HUFFVAL; index 0 = DC luminance, 1 = AC luminance, 2 = DC chrominance, 3 = AC chrominance
static const uint8_t JP_BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                       {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t JP_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t JP_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// What the kernels read, built on the host once per de_set_jpeg and uploaded.
struct JpegTables {
    int32_t M[64];            // the DCT matrix, M[u * 8 + x] = rint(2^14 * 1/2 c(u) cos((2 x + 1) u pi / 16))
    uint16_t Q[2][64];        // the quantiser's steps, natural order: [0] luminance, [1] chrominance
    uint8_t zzpos[64];        // natural index -> zigzag position
    uint32_t dc[2][12];       // Huffman code of a DC category: length << 16 | code; [0] luminance, [1] chrominance
    uint32_t ac[2][256];      // of an AC (run << 4 | size) symbol; 0 where the table has none
};

static inline void jp_huffman_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {      // T.81 Annex C: codes in order of length, counting up
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}
static inline void jp_make_tables(int quality, JpegTables* t) {
    memset(t, 0, sizeof(*t));
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x) t->M[u * 8 + x] = (int32_t)rint(16384.0 * 0.5 * (u ? 1.0 : sqrt(0.5)) * cos((2 * x + 1) * u * pi / 16.0));
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;      // the IJG rule
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            const int q = (JP_BASE_Q[c][i] * scale + 50) / 100;
            t->Q[c][i] = (uint16_t)(q < 1 ? 1 : q > 255 ? 255 : q);
        }
    for (int k = 0; k < 64; ++k) t->zzpos[JP_ZIGZAG[k]] = (uint8_t)k;
    jp_huffman_codes(JP_BITS[0], JP_DC_VALS, t->dc[0]);
    jp_huffman_codes(JP_BITS[2], JP_DC_VALS, t->dc[1]);
    jp_huffman_codes(JP_BITS[1], JP_AC_VALS[0], t->ac[0]);
    jp_huffman_codes(JP_BITS[3], JP_AC_VALS[1], t->ac[1]);
}

// ---- geometry of a W x H frame (both even) at a restart interval of `restart` MCUs
struct JpegGeometry {
    int W, H, mcus_x, mcus_y, restart;       // restart: as set, clipped to the frame's MCU count (a slot never needs more)
    size_t mcus, blocks, intervals;
    size_t slot_bytes;                       // the worst case of one interval's entropy-coded bytes, a multiple of 16
    size_t capacity;                         // of the whole stream: framing + intervals * slot_bytes + the RSTm between them + EOI
};
static inline JpegGeometry jp_geometry(int W, int H, int restart) {
    JpegGeometry g;
    g.W = W; g.H = H; g.mcus_x = (W + 15) / 16; g.mcus_y = (H + 15) / 16;
    g.mcus = (size_t)g.mcus_x * (size_t)g.mcus_y; g.blocks = g.mcus * 6;
    g.restart = (size_t)restart < g.mcus ? restart : (int)(g.mcus < 65535 ? g.mcus : 65535);
    g.intervals = (g.mcus + (size_t)g.restart - 1) / (size_t)g.restart;
    const size_t bits = (size_t)g.restart * 6 * JP_BLOCK_BITS;
    g.slot_bytes = (2 * ((bits + 7) / 8) + 15) & ~(size_t)15;      // every byte stuffed, the last one padded
    g.capacity = JP_FRAMING_BYTES + g.intervals * g.slot_bytes + 2 * (g.intervals - 1) + 2;
    return g;
}

// ---- the framing: SOI, APP0 "JFIF" 1.02, DQT x 2, SOF0, DHT x 4, DRI, SOS.  `out` takes JP_FRAMING_BYTES; the entropy-coded data follows directly.
static inline size_t jp_write_framing(const JpegTables& t, int W, int H, int restart, uint8_t* out) {
    uint8_t* p = out;
    auto u8 = [&](int v) { *p++ = (uint8_t)v; };
    auto u16 = [&](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
    u16(0xFFD8);
    u16(0xFFE0); u16(16); u8('J'); u8('F'); u8('I'); u8('F'); u8(0); u8(1); u8(2); u8(0); u16(1); u16(1); u8(0); u8(0);
    for (int c = 0; c < 2; ++c) {
        u16(0xFFDB); u16(67); u8(c);
        for (int k = 0; k < 64; ++k) u8(t.Q[c][JP_ZIGZAG[k]]);
    }
    u16(0xFFC0); u16(17); u8(8); u16(H); u16(W); u8(3);
    u8(1); u8(0x22); u8(0); u8(2); u8(0x11); u8(1); u8(3); u8(0x11); u8(1);
    for (int i = 0; i < 4; ++i) {      // DC luminance, AC luminance, DC chrominance, AC chrominance
        const bool ac = (i & 1) != 0;
        const int n = ac ? 162 : 12;
        u16(0xFFC4); u16(2 + 1 + 16 + n); u8((ac ? 0x10 : 0x00) | (i >> 1));
        for (int k = 0; k < 16; ++k) u8(JP_BITS[i][k]);
        const uint8_t* vals = ac ? JP_AC_VALS[i >> 1] : JP_DC_VALS;
        for (int k = 0; k < n; ++k) u8(vals[k]);
    }
    u16(0xFFDD); u16(4); u16(restart);
    u16(0xFFDA); u16(12); u8(3); u8(1); u8(0x00); u8(2); u8(0x11); u8(3); u8(0x11); u8(0); u8(63); u8(0);
    return (size_t)(p - out);
}

// png_tables.h — the host side of the PNG output (include/digital_earth_png.h), plain C++ with no HIP in it: the tables the kernels look
// up (the CRC-32 byte table and its shift-by-2^k-bytes operators, deflate's length codes), the geometry (filtered bytes, chunks, the proven slot and
// capacity) and the front of the file (signature, IHDR, cICP) that the host writes once per setting and size.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define PNG_HD __host__ __device__      // png_gf2_times is the host's and the deflate kernel's
#else
#define PNG_HD
#endif

#define PNG_FRONT_MAX 64             // the front is 33 bytes (signature + IHDR), 49 with cICP
#define PNG_TRAILER_BYTES 28         // the IDAT that holds the Adler-32 (16) and IEND (12)
#define PNG_CHUNK_OVERHEAD 24        // per deflate chunk: IDAT length, type, CRC (12), CMF / FLG (2, the first only), a stored block's header (5), the sync block (5)
#define PNG_SHIFT_OPS 17             // shift by 2^k bytes, k = 0 .. 16: an IDAT is shorter than 2^17 bytes
#define PNG_MAX_FILTERED (1ull << 27)
#define PNG_ADLER 65521u

// What the kernels read, built on the host once and uploaded.
struct PngTables {
    uint32_t crc[256];                       // the reflected CRC-32 (polynomial 0xEDB88320) of one byte
    uint32_t shift[PNG_SHIFT_OPS][32];       // shift[k][i]: the register that bit i becomes behind 2^k zero bytes (a GF(2) matrix, one column per word)
    uint8_t len_code[256];                   // match length L - 3 -> index of its length code (symbol 257 + index)
    uint16_t len_base[29];
    uint8_t len_extra[29];
};

static inline PNG_HD uint32_t png_gf2_times(const uint32_t* mat, uint32_t vec) {
    uint32_t sum = 0;
    for (int i = 0; vec; vec >>= 1, ++i)
        if (vec & 1u) sum ^= mat[i];
    return sum;
}
// The Adler-32 of a concatenation: (A, B) the state behind the bytes so far, (a, b) the sums of the next n < 2^28 bytes from (0, 0), all below 65521.
static inline PNG_HD void png_adler_join(unsigned long long* A, unsigned long long* B, unsigned long long n, uint32_t a, uint32_t b) {
    *B = (*B + n * *A + b) % PNG_ADLER;
    *A = (*A + a) % PNG_ADLER;
}
static inline void png_gf2_square(uint32_t* square, const uint32_t* mat) {
    for (int i = 0; i < 32; ++i) square[i] = png_gf2_times(mat, mat[i]);
}
static inline void png_make_tables(PngTables* t) {
    memset(t, 0, sizeof(*t));
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t c = n;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        t->crc[n] = c;
    }
    uint32_t bit1[32], bit2[32], bit4[32];      // the operator of one zero BIT, squared three times: one zero byte
    bit1[0] = 0xedb88320u;
    for (int i = 1; i < 32; ++i) bit1[i] = 1u << (i - 1);
    png_gf2_square(bit2, bit1);
    png_gf2_square(bit4, bit2);
    png_gf2_square(t->shift[0], bit4);
    for (int k = 1; k < PNG_SHIFT_OPS; ++k) png_gf2_square(t->shift[k], t->shift[k - 1]);
    static const uint16_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    for (int i = 0; i < 29; ++i) { t->len_base[i] = base[i]; t->len_extra[i] = extra[i]; }
    for (int L = 3; L <= 258; ++L) {
        int i = 28;
        while (base[i] > L) --i;
        t->len_code[L - 3] = (uint8_t)i;
    }
}
// the CRC-32 of `n` bytes, for the front's chunks (the device computes the IDATs' and the trailer's)
static inline uint32_t png_crc(const PngTables& t, const uint8_t* p, size_t n) {
    uint32_t r = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) r = t.crc[(r ^ p[i]) & 0xffu] ^ (r >> 8);
    return r ^ 0xffffffffu;
}

// ---- geometry of a W x H frame of `channels` samples of `depth` bits, cut every `chunk_bytes`
struct PngGeometry {
    int W, H, channels, depth, bpp, chunk_bytes;
    size_t row_bytes;                        // W * bpp, without the filter byte
    size_t filtered;                         // N = H (1 + W bpp)
    size_t chunks;
    size_t slot_bytes;                       // the proven bound of one chunk's IDAT, a multiple of 16
    size_t front;                            // 33, or 49 with cICP (depth 16)
    size_t capacity;                         // front + N + 24 chunks + trailer
};
static inline PngGeometry png_geometry(int W, int H, int channels, int depth, int chunk_bytes) {
    PngGeometry g;
    g.W = W; g.H = H; g.channels = channels; g.depth = depth; g.bpp = channels * (depth / 8); g.chunk_bytes = chunk_bytes;
    g.row_bytes = (size_t)W * (size_t)g.bpp;
    g.filtered = (size_t)H * (1 + g.row_bytes);
    g.chunks = (g.filtered + (size_t)chunk_bytes - 1) / (size_t)chunk_bytes;
    g.slot_bytes = ((size_t)chunk_bytes + PNG_CHUNK_OVERHEAD + 15) & ~(size_t)15;
    g.front = depth == 16 ? 49 : 33;
    g.capacity = g.front + g.filtered + PNG_CHUNK_OVERHEAD * g.chunks + PNG_TRAILER_BYTES;
    return g;
}

// ---- the front: signature, IHDR and, for depth 16, cICP {primaries, transfer, matrix 0, full range 1}.  `out` takes PNG_FRONT_MAX; returns its length.
static inline size_t png_write_front(const PngTables& t, const PngGeometry& g, const uint8_t cicp[4], uint8_t* out) {
    uint8_t* p = out;
    auto u32 = [&](uint32_t v) { *p++ = (uint8_t)(v >> 24); *p++ = (uint8_t)(v >> 16); *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    memcpy(p, sig, 8); p += 8;
    u32(13);
    uint8_t* body = p;
    memcpy(p, "IHDR", 4); p += 4;
    u32((uint32_t)g.W); u32((uint32_t)g.H);
    *p++ = (uint8_t)g.depth; *p++ = (uint8_t)(g.channels == 4 ? 6 : 2); *p++ = 0; *p++ = 0; *p++ = 0;
    u32(png_crc(t, body, (size_t)(p - body)));
    if (g.depth == 16) {
        u32(4);
        body = p;
        memcpy(p, "cICP", 4); p += 4;
        memcpy(p, cicp, 4); p += 4;
        u32(png_crc(t, body, (size_t)(p - body)));
    }
    return (size_t)(p - out);
}

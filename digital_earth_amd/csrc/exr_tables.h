// exr_tables.h — the host side of the OpenEXR output (include/digital_earth_exr.h), plain C++ with no HIP in it: the geometry (blocks,
// chunks, the proven slot and capacity), the front of the file that the host writes once per setting and size, and the two leaves the kernels and
// the host check (tools/exr_host_check.cpp) share: the sample conversion and the reorder / predictor.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define EXR_HD __host__ __device__
#else
#define EXR_HD
#endif

#define EXR_FRONT_FIXED 313          // magic, version, the eight attributes, the header's closing byte; the offset table follows
#define EXR_FRONT_MAX 320
#define EXR_BLOCK_HEADER 8           // int32 y0, int32 dataSize
#define EXR_MAX_RAW (1ull << 27)     // H W 3 bps
#define EXR_CHUNK_OVERHEAD 24        // per deflate chunk, at most: the block header (8) and CMF / FLG (2) in a block's first, a stored block's header (5), the sync
                                     // block (5) behind every chunk but a block's last, which carries the Adler-32 (4) instead: the PNG slot's bound
#define EXR_PIXEL_HALF 1
#define EXR_PIXEL_FLOAT 2
#define EXR_COMPRESSION_NONE 0
#define EXR_COMPRESSION_ZIPS 2
#define EXR_COMPRESSION_ZIP 3

// ---- the sample (the header's THE SAMPLE)
static inline EXR_HD uint32_t exr_float_bits(float v) { uint32_t x; memcpy(&x, &v, 4); return x; }
// steps 1 to 3: the float32 product's bits, a NaN as +0
static inline EXR_HD uint32_t exr_sample_bits(float mean, float scale) {
    const uint32_t x = exr_float_bits(mean * scale);
    return (x & 0x7fffffffu) > 0x7f800000u ? 0u : x;
}
// step 4: the binary16 of a float32 that is not a NaN, clamped to +-65504, nearest even, subnormals kept
static inline EXR_HD uint32_t exr_half_bits(uint32_t x) {
    const uint32_t s = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
    if (a >= 0x477fe000u) return s | 0x7bffu;
    if (a >= 0x38800000u) return s | ((a + 0xfffu + ((a >> 13) & 1u) - 0x38000000u) >> 13);
    if (a <= 0x33000000u) return s;
    const uint32_t e = a >> 23, m = (a & 0x7fffffu) | 0x800000u, k = 126u - e;      // k = 14 ... 24
    uint32_t h = m >> k;
    const uint32_t r = m & ((1u << k) - 1u), half = 1u << (k - 1u);
    if (r > half || (r == half && (h & 1u))) ++h;
    return s | h;
}

// ---- the reorder and the predictor: byte i of the payload's input p, from a block's raw bytes r[0 .. P)
static inline EXR_HD uint32_t exr_reordered(const uint8_t* r, uint32_t P, uint32_t i) {
    const uint32_t h = (P + 1u) / 2u;
    return i < h ? r[2u * i] : r[2u * (i - h) + 1u];
}
static inline EXR_HD uint32_t exr_predicted(const uint8_t* r, uint32_t P, uint32_t i) {
    const uint32_t t = exr_reordered(r, P, i);
    return i == 0u ? t : (t - exr_reordered(r, P, i - 1u) + 128u) & 0xffu;
}

// ---- geometry of a W x H frame
struct ExrGeometry {
    int W, H, bps, pixel_type, compression, L;
    size_t line_bytes;                       // W 3 bps
    size_t block_bytes;                      // P of a full block: L line_bytes
    size_t raw;                              // H W 3 bps
    size_t blocks;                           // nb
    size_t chunk;                            // bytes of p per piece: chunk_bytes, or the whole block under NONE
    size_t cpb;                              // pieces per block (the last block may use fewer)
    size_t pieces;                           // blocks cpb
    size_t slot_bytes;                       // the proven bound of one chunk's piece, a multiple of 16
    size_t r_stride, p_stride;               // of a block in the framed raw buffer (header + r) and in the predicted buffer, multiples of 16
    size_t front;                            // 313 + 8 nb
    size_t capacity;                         // front + 8 nb + raw
};
static inline ExrGeometry exr_geometry(int W, int H, int pixel_type, int compression, int chunk_bytes) {
    ExrGeometry g;
    g.W = W; g.H = H; g.pixel_type = pixel_type; g.compression = compression;
    g.bps = pixel_type == EXR_PIXEL_FLOAT ? 4 : 2;
    g.L = compression == EXR_COMPRESSION_ZIP ? 16 : 1;
    g.line_bytes = (size_t)W * 3 * (size_t)g.bps;
    g.block_bytes = (size_t)(H < g.L ? H : g.L) * g.line_bytes;
    g.raw = (size_t)H * g.line_bytes;
    g.blocks = ((size_t)H + (size_t)g.L - 1) / (size_t)g.L;
    g.chunk = compression == EXR_COMPRESSION_NONE ? g.block_bytes : (size_t)chunk_bytes;
    g.cpb = (g.block_bytes + g.chunk - 1) / g.chunk;
    g.pieces = g.blocks * g.cpb;
    g.slot_bytes = compression == EXR_COMPRESSION_NONE ? 16 : ((size_t)chunk_bytes + EXR_CHUNK_OVERHEAD + 15) & ~(size_t)15;
    g.r_stride = (EXR_BLOCK_HEADER + g.block_bytes + 15) & ~(size_t)15;
    g.p_stride = (g.block_bytes + 15) & ~(size_t)15;
    g.front = EXR_FRONT_FIXED + 8 * g.blocks;
    g.capacity = g.front + EXR_BLOCK_HEADER * g.blocks + g.raw;
    return g;
}

// ---- the front without the offset table.  `out` takes EXR_FRONT_MAX; returns its length, EXR_FRONT_FIXED.
static inline size_t exr_write_front(const ExrGeometry& g, uint8_t* out) {
    uint8_t* p = out;
    auto i32 = [&](int32_t v) { const uint32_t u = (uint32_t)v; *p++ = (uint8_t)u; *p++ = (uint8_t)(u >> 8); *p++ = (uint8_t)(u >> 16); *p++ = (uint8_t)(u >> 24); };
    auto str = [&](const char* s) { const size_t n = strlen(s) + 1; memcpy(p, s, n); p += n; };
    auto attr = [&](const char* name, const char* type, int32_t size) { str(name); str(type); i32(size); };
    auto f32 = [&](float v) { uint32_t u; memcpy(&u, &v, 4); i32((int32_t)u); };
    static const uint8_t magic[8] = {0x76, 0x2f, 0x31, 0x01, 0x02, 0x00, 0x00, 0x00};
    memcpy(p, magic, 8); p += 8;
    attr("channels", "chlist", 3 * 18 + 1);
    for (const char* name : {"B", "G", "R"}) { str(name); i32(g.pixel_type); *p++ = 0; *p++ = 0; *p++ = 0; *p++ = 0; i32(1); i32(1); }
    *p++ = 0;
    attr("compression", "compression", 1); *p++ = (uint8_t)g.compression;
    attr("dataWindow", "box2i", 16); i32(0); i32(0); i32(g.W - 1); i32(g.H - 1);
    attr("displayWindow", "box2i", 16); i32(0); i32(0); i32(g.W - 1); i32(g.H - 1);
    attr("lineOrder", "lineOrder", 1); *p++ = 0;
    attr("pixelAspectRatio", "float", 4); f32(1.0f);
    attr("screenWindowCenter", "v2f", 8); f32(0.0f); f32(0.0f);
    attr("screenWindowWidth", "float", 4); f32(1.0f);
    *p++ = 0;
    return (size_t)(p - out);
}

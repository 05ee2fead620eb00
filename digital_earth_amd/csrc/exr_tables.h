// exr_tables.h — the host side of the OpenEXR output (include/digital_earth_exr.h), plain C++ with no HIP in it: the geometry (blocks,
// chunks, the proven slot and capacity), the front of the file that the host writes once per setting and size, and the two leaves the kernels and
// the host check (tools/exr_host_check.cpp) share: the sample conversion and the reorder / predictor.  The AOV channels (include/digital_earth_exr_aovs.h,
// DESIGN.md §24) add the channel descriptors, the byte-wise sort of a mask's channels, their planes' offsets within a line, and the leaf of one thread
// of exr_aov_layout_kernel (tools/exr_aov_host_check.cpp runs it for every thread on the CPU).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define EXR_HD __host__ __device__
#else
#define EXR_HD
#endif

#define EXR_FRONT_FIXED 313          // with B, G, R alone: magic, version, the eight attributes, the header's closing byte; the offset table follows
#define EXR_FRONT_MAX 640            // with all 16 channels the header is 626 bytes
#define EXR_BLOCK_HEADER 8           // int32 y0, int32 dataSize
#define EXR_MAX_RAW (1ull << 27)     // H W sum(bps): the coded tail counts bytes in 32 bits.  B, G, R alone: 3840 x 2160 at FLOAT fits.  Every AOV on is 42 B
                                     // per pixel at HALF (1920 x 1080 fits, 3840 x 2160 does not) and 64 B at FLOAT (1920 x 1080 is 132 710 400, just under)
#define EXR_MAX_CHANNELS 16
#define EXR_MAX_AOV_PLANES 13
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

// ---- the channels.  The AOV groups' bits (DE_EXR_AOV_* of include/digital_earth_exr_aovs.h) and where a channel's samples come from.
#define EXR_AOV_DEPTH 1u
#define EXR_AOV_NORMAL 2u
#define EXR_AOV_ALBEDO 4u
#define EXR_AOV_COVERAGE 8u
#define EXR_AOV_TRANSMITTANCE 16u
#define EXR_AOV_VARIANCE 32u
#define EXR_AOV_SAMPLES 64u
#define EXR_AOV_ALL 127u
enum ExrSlot { EXR_SLOT_R, EXR_SLOT_G, EXR_SLOT_B, EXR_SLOT_Z, EXR_SLOT_NX, EXR_SLOT_NY, EXR_SLOT_NZ, EXR_SLOT_ALBEDO_R, EXR_SLOT_ALBEDO_G, EXR_SLOT_ALBEDO_B,
               EXR_SLOT_COVERAGE, EXR_SLOT_TRANSMITTANCE, EXR_SLOT_VARIANCE_R, EXR_SLOT_VARIANCE_G, EXR_SLOT_VARIANCE_B, EXR_SLOT_SAMPLES, EXR_SLOTS };
// what a slot reads (ExrAov::need): the two float4 and the float of the guides, the sums with S2, the divisor
#define EXR_NEED_NC 1u
#define EXR_NEED_AT 2u
#define EXR_NEED_DIST 4u
#define EXR_NEED_MOMENTS 8u
#define EXR_NEED_DIVISOR 16u
struct ExrChannel {
    const char* name;
    int pixel_type, bps, slot;
    size_t offset;                           // of its plane within a line: W times the bps of the channels sorted before it
};
// Every channel this output knows, in slot order: its name, the group's bit (0: always there), whether it is FLOAT whatever the file's pixel type.
struct ExrChannelKind { const char* name; uint32_t bit; int always_float; };
static inline const ExrChannelKind* exr_channel_kinds() {
    static const ExrChannelKind kinds[EXR_SLOTS] = {
        {"R", 0u, 0}, {"G", 0u, 0}, {"B", 0u, 0}, {"Z", EXR_AOV_DEPTH, 1}, {"N.X", EXR_AOV_NORMAL, 0}, {"N.Y", EXR_AOV_NORMAL, 0}, {"N.Z", EXR_AOV_NORMAL, 0},
        {"albedo.R", EXR_AOV_ALBEDO, 0}, {"albedo.G", EXR_AOV_ALBEDO, 0}, {"albedo.B", EXR_AOV_ALBEDO, 0}, {"coverage", EXR_AOV_COVERAGE, 0},
        {"transmittance", EXR_AOV_TRANSMITTANCE, 0}, {"variance.R", EXR_AOV_VARIANCE, 1}, {"variance.G", EXR_AOV_VARIANCE, 1}, {"variance.B", EXR_AOV_VARIANCE, 1},
        {"samples", EXR_AOV_SAMPLES, 1}};
    return kinds;
}
static inline uint32_t exr_slot_need(int slot) {
    switch (slot) {
    case EXR_SLOT_Z: return EXR_NEED_DIST;
    case EXR_SLOT_NX: case EXR_SLOT_NY: case EXR_SLOT_NZ: case EXR_SLOT_COVERAGE: return EXR_NEED_NC;
    case EXR_SLOT_ALBEDO_R: case EXR_SLOT_ALBEDO_G: case EXR_SLOT_ALBEDO_B: case EXR_SLOT_TRANSMITTANCE: return EXR_NEED_AT;
    case EXR_SLOT_VARIANCE_R: case EXR_SLOT_VARIANCE_G: case EXR_SLOT_VARIANCE_B: return EXR_NEED_MOMENTS | EXR_NEED_DIVISOR;
    case EXR_SLOT_SAMPLES: return EXR_NEED_DIVISOR;
    default: return 0u;
    }
}
// The channels of a mask in the file's order — sorted by name as bytes, which OpenEXR requires (uppercase before lowercase) — with their types, bps
// and plane offsets in a line of W pixels.  The one place where the order is made: an insertion sort on strcmp, which compares unsigned bytes.
static inline int exr_channel_list(uint32_t mask, int pixel_type, int W, ExrChannel out[EXR_MAX_CHANNELS]) {
    const ExrChannelKind* kinds = exr_channel_kinds();
    int n = 0;
    for (int slot = 0; slot < EXR_SLOTS; ++slot) {
        if (kinds[slot].bit && !(mask & kinds[slot].bit)) continue;
        ExrChannel c;
        c.name = kinds[slot].name; c.slot = slot; c.offset = 0;
        c.pixel_type = kinds[slot].always_float ? EXR_PIXEL_FLOAT : pixel_type;
        c.bps = c.pixel_type == EXR_PIXEL_FLOAT ? 4 : 2;
        int at = n++;
        for (; at > 0 && strcmp(out[at - 1].name, c.name) > 0; --at) out[at] = out[at - 1];
        out[at] = c;
    }
    size_t offset = 0;
    for (int k = 0; k < n; ++k) { out[k].offset = offset; offset += (size_t)W * (size_t)out[k].bps; }
    return n;
}

// ---- geometry of a W x H frame
struct ExrGeometry {
    int W, H, bps, pixel_type, compression, L;
    uint32_t mask;                           // the AOV groups
    int channels;                            // 3 ... 16
    ExrChannel ch[EXR_MAX_CHANNELS];         // in the file's order
    size_t sum_bps;                          // of a pixel over all channels: 3 bps with B, G, R alone
    size_t front_fixed;                      // the header's length: 313 with B, G, R alone
    size_t line_bytes;                       // W sum_bps
    size_t block_bytes;                      // P of a full block: L line_bytes
    size_t raw;                              // H W sum_bps
    size_t blocks;                           // nb
    size_t chunk;                            // bytes of p per piece: chunk_bytes, or the whole block under NONE
    size_t cpb;                              // pieces per block (the last block may use fewer)
    size_t pieces;                           // blocks cpb
    size_t slot_bytes;                       // the proven bound of one chunk's piece, a multiple of 16
    size_t r_stride, p_stride;               // of a block in the framed raw buffer (header + r) and in the predicted buffer, multiples of 16
    size_t front;                            // front_fixed + 8 nb
    size_t capacity;                         // front + 8 nb + raw
};
static inline ExrGeometry exr_geometry(int W, int H, int pixel_type, int compression, int chunk_bytes, uint32_t mask = 0u) {
    ExrGeometry g;
    g.W = W; g.H = H; g.pixel_type = pixel_type; g.compression = compression; g.mask = mask;
    g.bps = pixel_type == EXR_PIXEL_FLOAT ? 4 : 2;
    g.L = compression == EXR_COMPRESSION_ZIP ? 16 : 1;
    g.channels = exr_channel_list(mask, pixel_type, W, g.ch);
    g.sum_bps = 0;
    g.front_fixed = EXR_FRONT_FIXED - 3 * 18;      // without the channels' entries
    for (int k = 0; k < g.channels; ++k) { g.sum_bps += (size_t)g.ch[k].bps; g.front_fixed += strlen(g.ch[k].name) + 17; }
    g.line_bytes = (size_t)W * g.sum_bps;
    g.block_bytes = (size_t)(H < g.L ? H : g.L) * g.line_bytes;
    g.raw = (size_t)H * g.line_bytes;
    g.blocks = ((size_t)H + (size_t)g.L - 1) / (size_t)g.L;
    g.chunk = compression == EXR_COMPRESSION_NONE ? g.block_bytes : (size_t)chunk_bytes;
    g.cpb = (g.block_bytes + g.chunk - 1) / g.chunk;
    g.pieces = g.blocks * g.cpb;
    g.slot_bytes = compression == EXR_COMPRESSION_NONE ? 16 : ((size_t)chunk_bytes + EXR_CHUNK_OVERHEAD + 15) & ~(size_t)15;
    g.r_stride = (EXR_BLOCK_HEADER + g.block_bytes + 15) & ~(size_t)15;
    g.p_stride = (g.block_bytes + 15) & ~(size_t)15;
    g.front = g.front_fixed + 8 * g.blocks;
    g.capacity = g.front + EXR_BLOCK_HEADER * g.blocks + g.raw;
    return g;
}

// ---- the front without the offset table.  `out` takes EXR_FRONT_MAX; returns its length, g.front_fixed (EXR_FRONT_FIXED with B, G, R alone).
static inline size_t exr_write_front(const ExrGeometry& g, uint8_t* out) {
    uint8_t* p = out;
    auto i32 = [&](int32_t v) { const uint32_t u = (uint32_t)v; *p++ = (uint8_t)u; *p++ = (uint8_t)(u >> 8); *p++ = (uint8_t)(u >> 16); *p++ = (uint8_t)(u >> 24); };
    auto str = [&](const char* s) { const size_t n = strlen(s) + 1; memcpy(p, s, n); p += n; };
    auto attr = [&](const char* name, const char* type, int32_t size) { str(name); str(type); i32(size); };
    auto f32 = [&](float v) { uint32_t u; memcpy(&u, &v, 4); i32((int32_t)u); };
    static const uint8_t magic[8] = {0x76, 0x2f, 0x31, 0x01, 0x02, 0x00, 0x00, 0x00};
    memcpy(p, magic, 8); p += 8;
    int32_t chlist = 1;
    for (int k = 0; k < g.channels; ++k) chlist += (int32_t)strlen(g.ch[k].name) + 17;
    attr("channels", "chlist", chlist);
    for (int k = 0; k < g.channels; ++k) { str(g.ch[k].name); i32(g.ch[k].pixel_type); *p++ = 0; *p++ = 0; *p++ = 0; *p++ = 0; i32(1); i32(1); }
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

// ---- the AOV planes: what one thread of exr_aov_layout_kernel does, as a leaf of plain C++
struct alignas(16) ExrF4 { float x, y, z, w; };      // a guide's float4, loaded as 16 aligned bytes
struct ExrPlane { uint32_t slot, bps, offset; };     // an AOV channel: its source, its bytes per sample, its plane's offset within a line
struct ExrAov {
    const ExrF4* nc;            // [H][W]: normal x, y, z, land coverage           (null unless need & EXR_NEED_NC)
    const ExrF4* at;            // [H][W]: albedo r, g, b, cloud transmittance     (null unless need & EXR_NEED_AT)
    const float* dist;          // [H][W]: distance in metres, 0 without a hit     (null unless need & EXR_NEED_DIST)
    const float* s1;            // [H][W][3] sums                                  (null unless need & EXR_NEED_MOMENTS)
    const float* s2;            // [H][W][3] sums of squares                       (the same)
    const int32_t* tile_spp;    // the divisor: a tile's own count inside an adaptive frame, else null
    const float* counts;        // the divisor per pixel, [H][W] (de_debug_exr_aovs), else null
    int samples;                // the divisor otherwise: the frame's count
    uint32_t need;              // EXR_NEED_* over the planes
    uint32_t planes;
    ExrPlane plane[EXR_MAX_AOV_PLANES];
};
static inline EXR_HD float exr_divisor(const int32_t* tile_spp, const float* counts, int samples, uint32_t W, uint32_t x, uint32_t j) {
    if (counts) return counts[(size_t)j * W + x];
    return tile_spp ? (float)tile_spp[(size_t)(j >> 3) * (W >> 3) + (x >> 3)] : (float)samples;
}
// THE VARIANCE of the mean, float32 at every step, nothing fused: mean = S1 / n; prod = S1 * mean; d = S2 - prod; q = d / (n - 1); sample variance
// sv = q if q > 0 else 0 (a NaN too); the result sv / n.  0 where n < 2 (or n is a NaN).
static inline EXR_HD float exr_variance_of_mean(float s1, float s2, float n) {
    if (!(n >= 2.0f)) return 0.0f;
    const float mean = s1 / n;
#ifdef __HIP_DEVICE_COMPILE__
    const float prod = __fmul_rn(s1, mean), d = __fsub_rn(s2, prod);
#else
    volatile float prod_v = s1 * mean;      // the host: kept apart from the subtraction
    const float prod = prod_v, d = s2 - prod;
#endif
    const float q = d / (n - 1.0f);
    const float sv = q > 0.0f ? q : 0.0f;
    return sv / n;
}
// Thread (x0 = 4 g, file row of `row`, source row j): the up to four pixels' values of every selected plane, converted (a channel at the file's
// pixel type as B, G, R are, with scale 1; a FLOAT channel its 32 bits, a NaN +0) and stored.  `row` is the line's first byte; a sample that would
// pass line_bytes is not stored and the function answers false.  VEC: W is a multiple of 4 and dist, s1, s2 are 16-byte aligned; the four samples
// of a plane then leave as one 8-byte store (HALF) or two (FLOAT) where their address is 8-byte aligned, which it is behind a block's 8-byte header.
// Every loop over the four pixels has a constant trip count under a predicate, so that the values stay in registers.
#define EXR_UNROLL _Pragma("unroll")
struct alignas(8) ExrU2 { uint32_t x, y; };
static inline EXR_HD float exr_aov_value(uint32_t slot, const ExrF4& nc, const ExrF4& at, float dist, const float* s1, const float* s2, float div) {
    switch (slot) {
    case EXR_SLOT_Z: return dist;
    case EXR_SLOT_NX: return nc.x;
    case EXR_SLOT_NY: return nc.y;
    case EXR_SLOT_NZ: return nc.z;
    case EXR_SLOT_COVERAGE: return nc.w;
    case EXR_SLOT_ALBEDO_R: return at.x;
    case EXR_SLOT_ALBEDO_G: return at.y;
    case EXR_SLOT_ALBEDO_B: return at.z;
    case EXR_SLOT_TRANSMITTANCE: return at.w;
    case EXR_SLOT_VARIANCE_R: return exr_variance_of_mean(s1[0], s2[0], div);
    case EXR_SLOT_VARIANCE_G: return exr_variance_of_mean(s1[1], s2[1], div);
    case EXR_SLOT_VARIANCE_B: return exr_variance_of_mean(s1[2], s2[2], div);
    case EXR_SLOT_SAMPLES: return div;
    default: return 0.0f;
    }
}
template <bool VEC>
static inline EXR_HD bool exr_aov_thread(const ExrAov& v, uint8_t* row, uint32_t line_bytes, uint32_t W, uint32_t x0, uint32_t j) {
    const uint32_t n = W - x0 < 4u ? W - x0 : 4u;
    const size_t p = (size_t)j * W + x0;
    ExrF4 nc[4] = {}, at[4] = {};
    float dist[4] = {}, s1[12] = {}, s2[12] = {}, div[4] = {};
    if (v.need & EXR_NEED_NC) { EXR_UNROLL for (uint32_t k = 0u; k < 4u; ++k) if (k < n) nc[k] = v.nc[p + k]; }
    if (v.need & EXR_NEED_AT) { EXR_UNROLL for (uint32_t k = 0u; k < 4u; ++k) if (k < n) at[k] = v.at[p + k]; }
    if (v.need & EXR_NEED_DIST) {
        if (VEC) { const ExrF4 d = *reinterpret_cast<const ExrF4*>(v.dist + p); dist[0] = d.x; dist[1] = d.y; dist[2] = d.z; dist[3] = d.w; }
        else { EXR_UNROLL for (uint32_t k = 0u; k < 4u; ++k) if (k < n) dist[k] = v.dist[p + k]; }
    }
    if (v.need & EXR_NEED_MOMENTS) {
        if (VEC) {
            EXR_UNROLL for (uint32_t q = 0u; q < 3u; ++q) {
                const ExrF4 a = reinterpret_cast<const ExrF4*>(v.s1 + 3u * p)[q], b = reinterpret_cast<const ExrF4*>(v.s2 + 3u * p)[q];
                s1[4u * q] = a.x; s1[4u * q + 1u] = a.y; s1[4u * q + 2u] = a.z; s1[4u * q + 3u] = a.w;
                s2[4u * q] = b.x; s2[4u * q + 1u] = b.y; s2[4u * q + 2u] = b.z; s2[4u * q + 3u] = b.w;
            }
        } else {
            EXR_UNROLL for (uint32_t k = 0u; k < 12u; ++k) if (k < 3u * n) { s1[k] = v.s1[3u * p + k]; s2[k] = v.s2[3u * p + k]; }
        }
    }
    if (v.need & EXR_NEED_DIVISOR) { EXR_UNROLL for (uint32_t k = 0u; k < 4u; ++k) if (k < n) div[k] = exr_divisor(v.tile_spp, v.counts, v.samples, W, x0 + k, j); }
    bool ok = true;
    for (uint32_t i = 0u; i < v.planes && i < EXR_MAX_AOV_PLANES; ++i) {
        const ExrPlane pl = v.plane[i];
        if (pl.bps != 2u && pl.bps != 4u) { ok = false; continue; }
        uint32_t bits[4];
        EXR_UNROLL for (uint32_t k = 0u; k < 4u; ++k) {
            bits[k] = exr_sample_bits(exr_aov_value(pl.slot, nc[k], at[k], dist[k], s1 + 3u * k, s2 + 3u * k, div[k]), 1.0f);
            if (pl.bps == 2u) bits[k] = exr_half_bits(bits[k]);
        }
        const size_t at0 = (size_t)pl.offset + (size_t)x0 * pl.bps;
        uint8_t* dst = row + at0;
        if (VEC && at0 + 4u * (size_t)pl.bps <= (size_t)line_bytes && (reinterpret_cast<uintptr_t>(dst) & 7u) == 0u) {      // (VEC: n == 4)
            ExrU2* out = reinterpret_cast<ExrU2*>(dst);
            if (pl.bps == 2u) { const ExrU2 w = {bits[0] | (bits[1] << 16), bits[2] | (bits[3] << 16)}; out[0] = w; }
            else { const ExrU2 lo = {bits[0], bits[1]}, hi = {bits[2], bits[3]}; out[0] = lo; out[1] = hi; }
            continue;
        }
        EXR_UNROLL for (uint32_t k = 0u; k < 4u; ++k) {
            if (k >= n) continue;
            const size_t at_byte = at0 + (size_t)k * pl.bps;
            if (at_byte + pl.bps > (size_t)line_bytes) { ok = false; continue; }
            if (pl.bps == 2u) { const uint16_t h = (uint16_t)bits[k]; memcpy(row + at_byte, &h, 2); }
            else memcpy(row + at_byte, &bits[k], 4);
        }
    }
    return ok;
}

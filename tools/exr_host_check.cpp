// exr_host_check.cpp — the host side and the plain leaves of the OpenEXR output (csrc/exr_tables.h: the front, the geometry and capacity, the sample
// conversion, the reorder and the predictor; csrc/coded_stream.h: the compaction from a piece's alternative source) compiled for the
// HOST under the address and undefined-behaviour sanitizers.  No GPU, no library.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/exr_host_check.cpp -o exr_host_check && ./exr_host_check
// Checked, each against a serial statement written apart from the leaf: the front's 313 bytes field by field at several sizes and settings, into a
// heap buffer of exactly its size; the geometry's counts, strides and capacity; the HALF conversion against a statement in double arithmetic (the clamped value in
// units of its binary16 quantum, rounded by nearbyint) on every 101st float32 bit pattern and on every pattern within 64 of a boundary; the reorder and the predictor for
// every thread in turn on heap buffers of exactly P bytes, undone again; and the tail with raw pieces — every piece from its slot or from `alt`,
// one alt piece that would pass alt_bytes refused.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#define DE_DEV static inline
#include "../digital_earth_amd/csrc/exr_tables.h"
#include "../digital_earth_amd/csrc/coded_stream.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// ---- the front, once more as a string built field by field
static void put_i32(std::string& s, int32_t v) { for (int k = 0; k < 4; ++k) s.push_back((char)(((uint32_t)v >> (8 * k)) & 0xff)); }
static void put_str(std::string& s, const char* t) { s.append(t); s.push_back('\0'); }
static std::string front_serial(int W, int H, int pixel_type, int compression) {
    std::string s("\x76\x2f\x31\x01\x02\x00\x00\x00", 8);
    put_str(s, "channels"); put_str(s, "chlist"); put_i32(s, 55);
    for (const char* n : {"B", "G", "R"}) { put_str(s, n); put_i32(s, pixel_type); s.append(4, '\0'); put_i32(s, 1); put_i32(s, 1); }
    s.push_back('\0');
    put_str(s, "compression"); put_str(s, "compression"); put_i32(s, 1); s.push_back((char)compression);
    for (const char* n : {"dataWindow", "displayWindow"}) { put_str(s, n); put_str(s, "box2i"); put_i32(s, 16); put_i32(s, 0); put_i32(s, 0); put_i32(s, W - 1); put_i32(s, H - 1); }
    put_str(s, "lineOrder"); put_str(s, "lineOrder"); put_i32(s, 1); s.push_back('\0');
    put_str(s, "pixelAspectRatio"); put_str(s, "float"); put_i32(s, 4); put_i32(s, 0x3f800000);
    put_str(s, "screenWindowCenter"); put_str(s, "v2f"); put_i32(s, 8); put_i32(s, 0); put_i32(s, 0);
    put_str(s, "screenWindowWidth"); put_str(s, "float"); put_i32(s, 4); put_i32(s, 0x3f800000);
    s.push_back('\0');
    return s;
}

static void check_front_and_geometry() {
    static const int sizes[][2] = {{1, 1}, {3, 17}, {700, 33}, {8, 1100}, {1920, 1080}, {3840, 2160}, {65536, 341}};
    for (const auto& wh : sizes)
        for (int pt : {EXR_PIXEL_HALF, EXR_PIXEL_FLOAT})
            for (int comp : {EXR_COMPRESSION_NONE, EXR_COMPRESSION_ZIPS, EXR_COMPRESSION_ZIP})
                for (int chunk : {1024, 32768, 65535}) {
                    const int W = wh[0], H = wh[1];
                    const ExrGeometry g = exr_geometry(W, H, pt, comp, chunk);
                    std::vector<uint8_t> out(EXR_FRONT_MAX);      // (the writer's contract: EXR_FRONT_MAX)
                    const size_t n = exr_write_front(g, out.data());
                    const std::string want = front_serial(W, H, pt, comp);
                    CHECK(n == EXR_FRONT_FIXED && want.size() == EXR_FRONT_FIXED && memcmp(out.data(), want.data(), n) == 0, "front of %d x %d type %d compression %d", W, H, pt, comp);
                    const size_t bps = pt == EXR_PIXEL_FLOAT ? 4 : 2, L = comp == EXR_COMPRESSION_ZIP ? 16 : 1, nb = ((size_t)H + L - 1) / L;
                    const size_t raw = (size_t)W * H * 3 * bps, P = (size_t)(H < (int)L ? H : (int)L) * W * 3 * bps;
                    CHECK(g.blocks == nb && g.raw == raw && g.block_bytes == P && g.front == 313 + 8 * nb && g.capacity == 313 + 16 * nb + raw, "geometry of %d x %d", W, H);
                    CHECK(g.r_stride % 16 == 0 && g.r_stride >= 8 + P && g.p_stride % 16 == 0 && g.p_stride >= P && g.slot_bytes % 16 == 0, "strides of %d x %d", W, H);
                    if (comp == EXR_COMPRESSION_NONE) CHECK(g.cpb == 1 && g.chunk == P && g.pieces == nb, "NONE: one piece per block");
                    else CHECK(g.chunk == (size_t)chunk && g.cpb == (P + chunk - 1) / chunk && g.pieces == nb * g.cpb && g.slot_bytes >= (size_t)chunk + EXR_CHUNK_OVERHEAD, "pieces of %d x %d", W, H);
                    CHECK(raw > EXR_MAX_RAW || g.capacity + 16 < (1ull << 32), "the capacity fits 32 bits");
                }
}

// ---- the conversion
static uint32_t half_by_rounding(uint32_t x) {      // in double: the clamped value in units of its binary16 quantum, nearbyint's ties to even
    float v;
    memcpy(&v, &x, 4);
    if (v > 65504.0f) v = 65504.0f;
    if (v < -65504.0f) v = -65504.0f;
    const uint32_t sign = (x >> 16) & 0x8000u;
    const double a = fabs((double)v);
    if (a == 0.0) return sign;
    int e;
    (void)frexp(a, &e);                        // a = m 2^e, m in [0.5, 1): the leading bit is 2^(e - 1)
    int E = e - 1 < -14 ? -14 : e - 1;         // the quantum is 2^(E - 10); below 2^-14 it stays 2^-24
    double q = nearbyint(ldexp(a, 10 - E));    // exact scaling, then the default rounding mode: to nearest, ties to even
    if (E == -14 && q < 1024.0) return sign | (uint32_t)q;      // a subnormal half
    if (q == 2048.0) { q = 1024.0; ++E; }
    return sign | ((uint32_t)(E + 15) << 10) | ((uint32_t)q - 1024u);
}
static void check_conversion() {
    unsigned long long checked = 0;
    auto one = [&](uint32_t x) {
        if ((x & 0x7fffffffu) > 0x7f800000u) return;      // a NaN never reaches exr_half_bits
        const uint32_t got = exr_half_bits(x), want = half_by_rounding(x);
        CHECK(got == want, "half of %08x is %04x, not %04x", x, got, want);
        ++checked;
    };
    for (uint64_t x = 0; x < (1ull << 32); x += 101) one((uint32_t)x);
    static const uint32_t edges[] = {0u, 0x33000000u, 0x33800000u, 0x38800000u, 0x387fe000u, 0x3f800000u, 0x3f801000u, 0x3f803000u, 0x477fe000u, 0x477ff000u, 0x7f800000u, 0x7f7fffffu};
    for (uint32_t e : edges)
        for (int d = -64; d <= 64; ++d)
            for (uint32_t sign : {0u, 0x80000000u}) one(((e + (uint32_t)d) & 0x7fffffffu) | sign);
    for (uint32_t e = 0x32800000u; e <= 0x39000000u; e += 0x00001000u) { one(e); one(e + 0xfffu); one(e - 1u); }      // every half-ulp boundary of the subnormal range
    // steps 1 to 3
    const float nan = nanf("");
    CHECK(exr_sample_bits(nan, 1.0f) == 0u && exr_sample_bits(-nan, 2.0f) == 0u, "a NaN does not become +0");
    CHECK(exr_sample_bits(INFINITY, 0.5f) == 0x7f800000u && exr_sample_bits(-0.0f, 1.0f) == 0x80000000u && exr_sample_bits(1.5f, 3.0f) == 0x40900000u, "the product's bits");
    CHECK(exr_sample_bits(INFINITY - INFINITY, 1.0f) == 0u, "inf - inf");
    CHECK(exr_half_bits(exr_sample_bits(-INFINITY, 1.0f)) == 0xfbffu, "-inf clamps to -65504");
    printf("  conversion: %llu bit patterns against the statement in double\n", checked);
}

// ---- the reorder and the predictor, every thread in turn, on buffers of exactly P bytes
static void check_predictor() {
    uint32_t seed = 99u;
    for (uint32_t P : {1u, 2u, 3u, 6u, 7u, 12u, 255u, 256u, 1000u, 4801u, 67200u}) {
        uint8_t* r = (uint8_t*)malloc(P);
        uint8_t* p = (uint8_t*)malloc(P);
        for (uint32_t i = 0; i < P; ++i) { seed = seed * 1664525u + 1013904223u; r[i] = (uint8_t)(seed >> 24); }
        for (uint32_t i = 0; i < P; ++i) { const uint32_t v = exr_predicted(r, P, i); CHECK(v < 256u, "a predicted byte above 255"); p[i] = (uint8_t)v; }
        // undo: the running sum, then the interleave
        std::vector<uint8_t> t(P), back(P);
        t[0] = p[0];
        for (uint32_t i = 1; i < P; ++i) t[i] = (uint8_t)(t[i - 1] + p[i] - 128);
        const uint32_t h = (P + 1) / 2;
        for (uint32_t i = 0; i < P; ++i) back[i] = (i & 1u) ? t[h + i / 2] : t[i / 2];
        CHECK(memcmp(back.data(), r, P) == 0, "the predictor of %u bytes does not undo", P);
        for (uint32_t i = 0; i < P; ++i) CHECK(exr_reordered(r, P, i) == t[i], "the reorder of %u bytes at %u", P, i);
        free(r); free(p);
    }
}

// ---- the tail with pieces in `alt`
static void check_alt_compaction() {
    const uint32_t count = 9, SLOT = 32, FRONT = 21;
    std::vector<uint32_t> len(count), offset(count), alt_at(count), status(1, 0u), sums(CS_SCAN_THREADS);
    std::vector<uint8_t> slots((size_t)count * SLOT), alt(500);
    for (size_t k = 0; k < slots.size(); ++k) slots[k] = (uint8_t)(k * 3 + 1);
    for (size_t k = 0; k < alt.size(); ++k) alt[k] = (uint8_t)(200 - k);
    uint32_t total = FRONT, at = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const bool from_alt = (i % 3) != 1;
        len[i] = from_alt ? 40 + i : (i * 5) % (SLOT + 1);      // an alt piece may be longer than a slot
        alt_at[i] = from_alt ? at : CS_NO_ALT;
        if (from_alt) at += len[i];
        total += len[i];
    }
    CodedTail a;
    a.slots = slots.data(); a.len = len.data(); a.offset = offset.data(); a.status = status.data();
    a.count = count; a.slot_bytes = SLOT; a.front = FRONT; a.extra = 0; a.trailer = 0; a.capacity = total;
    a.alt = alt.data(); a.alt_at = alt_at.data(); a.alt_bytes = at;      // exactly what the pieces use
    std::vector<uint8_t> out(CS_WORD_BYTES + total, 0xA5);
    a.out = out.data();
    for (int t = 0; t < CS_SCAN_THREADS; ++t) cs_scan_sum(a, sums.data(), t);
    for (int t = 0; t < CS_SCAN_THREADS; ++t) cs_scan_total(a, sums.data(), t);
    for (int t = 0; t < CS_SCAN_THREADS; ++t) cs_scan_offsets(a, sums.data(), t);
    for (uint32_t i = 0; i < count + 1; ++i)
        for (int t = 0; t < 256; ++t) { const bool moved = cs_compact(a, i, t, 256); CHECK(moved == (i < count), "piece %u moved: %d", i, (int)moved); }
    uint32_t want = FRONT;
    for (uint32_t i = 0; i < count; ++i) {
        CHECK(offset[i] == want, "offset[%u]", i);
        const uint8_t* src = alt_at[i] == CS_NO_ALT ? slots.data() + (size_t)i * SLOT : alt.data() + alt_at[i];
        CHECK(memcmp(out.data() + CS_WORD_BYTES + want, src, len[i]) == 0, "the bytes of piece %u", i);
        want += len[i];
    }
    a.alt_bytes = at - 1;      // the last alt piece would read one byte past `alt`
    uint32_t last_alt = count - 1;
    while (alt_at[last_alt] == CS_NO_ALT) --last_alt;
    for (int t = 0; t < 256; ++t) CHECK(!cs_compact(a, last_alt, t, 256), "a piece that passes alt_bytes was moved");
}

int main() {
    check_front_and_geometry();
    check_conversion();
    check_predictor();
    check_alt_compaction();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("exr_host_check: front, geometry and capacity, conversion, reorder and predictor, compaction from alt: no sanitizer report\n");
    return 0;
}

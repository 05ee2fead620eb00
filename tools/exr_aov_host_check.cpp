// exr_aov_host_check.cpp — the host side and the plain leaf of the EXR output's AOV channels (csrc/exr_tables.h: the channel list and its byte-wise
// sort, the front with that list, the planes' offsets, the capacity, and exr_aov_thread, the body of one thread of exr_aov_layout_kernel;
// include/digital_earth_exr_aovs.h) compiled for the HOST under the address and undefined-behaviour sanitizers.  No GPU, no library.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/exr_aov_host_check.cpp -o exr_aov_host_check && ./exr_aov_host_check
// Checked, each against a serial statement written apart from the leaf: for all 128 masks and both pixel types the channel order (std::sort on
// strings compared as unsigned bytes), the front field by field into a heap buffer of exactly its size, the offsets and the capacity; the layout
// leaf for every thread of the grid at 1 x 1, 5 x 3, 37 x 17, 1029 x 2 and 1032 x 1, on heap buffers of exactly the bytes it may touch — the source
// buffers of an unselected slot are null — with a sentinel behind every line; and the refusal of a plane that would pass the line.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#define DE_DEV static inline
#include "../digital_earth_amd/csrc/exr_tables.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

struct Kind { const char* name; uint32_t bit; bool always_float; };
static const Kind KINDS[] = {{"R", 0, false}, {"G", 0, false}, {"B", 0, false}, {"Z", 1, true}, {"N.X", 2, false}, {"N.Y", 2, false}, {"N.Z", 2, false},
                             {"albedo.R", 4, false}, {"albedo.G", 4, false}, {"albedo.B", 4, false}, {"coverage", 8, false}, {"transmittance", 16, false},
                             {"variance.R", 32, true}, {"variance.G", 32, true}, {"variance.B", 32, true}, {"samples", 64, true}};

static void put_i32(std::string& s, int32_t v) { for (int k = 0; k < 4; ++k) s.push_back((char)(((uint32_t)v >> (8 * k)) & 0xff)); }
static void put_str(std::string& s, const char* t) { s.append(t); s.push_back('\0'); }
static bool bytes_less(const std::string& a, const std::string& b) {
    return std::lexicographical_compare(a.begin(), a.end(), b.begin(), b.end(), [](char x, char y) { return (unsigned char)x < (unsigned char)y; });
}

static void check_lists_fronts_and_capacity() {
    int lists = 0;
    for (uint32_t mask = 0; mask < 128; ++mask)
        for (int pt : {EXR_PIXEL_HALF, EXR_PIXEL_FLOAT})
            for (int comp : {EXR_COMPRESSION_NONE, EXR_COMPRESSION_ZIP}) {
                const int W = 37, H = 17;
                std::vector<std::string> names;
                for (const Kind& k : KINDS) if (!k.bit || (mask & k.bit)) names.push_back(k.name);
                std::sort(names.begin(), names.end(), bytes_less);
                const ExrGeometry g = exr_geometry(W, H, pt, comp, 4096, mask);
                CHECK(g.channels == (int)names.size() && g.channels <= EXR_MAX_CHANNELS, "mask %u: %d channels", mask, g.channels);
                size_t offset = 0, sum = 0;
                std::string chlist;
                for (int i = 0; i < g.channels && i < (int)names.size(); ++i) {
                    const Kind* kind = nullptr;
                    for (const Kind& k : KINDS) if (names[i] == k.name) kind = &k;
                    const int type = kind->always_float ? EXR_PIXEL_FLOAT : pt, bps = type == EXR_PIXEL_FLOAT ? 4 : 2;
                    CHECK(names[i] == g.ch[i].name && g.ch[i].pixel_type == type && g.ch[i].bps == bps && g.ch[i].offset == offset && g.ch[i].slot == (int)(kind - KINDS),
                          "mask %u channel %d: %s", mask, i, g.ch[i].name);
                    offset += (size_t)W * bps; sum += bps;
                    put_str(chlist, names[i].c_str()); put_i32(chlist, type); chlist.append(4, '\0'); put_i32(chlist, 1); put_i32(chlist, 1);
                }
                chlist.push_back('\0');
                std::string want("\x76\x2f\x31\x01\x02\x00\x00\x00", 8);
                put_str(want, "channels"); put_str(want, "chlist"); put_i32(want, (int32_t)chlist.size()); want += chlist;
                put_str(want, "compression"); put_str(want, "compression"); put_i32(want, 1); want.push_back((char)comp);
                for (const char* n : {"dataWindow", "displayWindow"}) { put_str(want, n); put_str(want, "box2i"); put_i32(want, 16); put_i32(want, 0); put_i32(want, 0); put_i32(want, W - 1); put_i32(want, H - 1); }
                put_str(want, "lineOrder"); put_str(want, "lineOrder"); put_i32(want, 1); want.push_back('\0');
                put_str(want, "pixelAspectRatio"); put_str(want, "float"); put_i32(want, 4); put_i32(want, 0x3f800000);
                put_str(want, "screenWindowCenter"); put_str(want, "v2f"); put_i32(want, 8); put_i32(want, 0); put_i32(want, 0);
                put_str(want, "screenWindowWidth"); put_str(want, "float"); put_i32(want, 4); put_i32(want, 0x3f800000);
                want.push_back('\0');
                CHECK(g.front_fixed == want.size() && g.front_fixed <= EXR_FRONT_MAX, "mask %u: a front of %zu bytes, not %zu", mask, g.front_fixed, want.size());
                if (g.front_fixed == want.size()) {
                    uint8_t* out = (uint8_t*)malloc(g.front_fixed);      // exactly its size: a byte more is a sanitizer report
                    const size_t n = exr_write_front(g, out);
                    CHECK(n == want.size() && memcmp(out, want.data(), n) == 0, "mask %u: the front", mask);
                    free(out);
                }
                const size_t L = comp == EXR_COMPRESSION_ZIP ? 16 : 1, nb = (H + L - 1) / L;
                CHECK(g.sum_bps == sum && g.line_bytes == W * sum && g.raw == (size_t)H * W * sum && g.front == want.size() + 8 * nb && g.capacity == g.front + 8 * nb + g.raw,
                      "mask %u: geometry", mask);
                CHECK(g.r_stride % 16 == 0 && g.r_stride >= 8 + g.block_bytes && g.block_bytes == (H < (int)L ? H : L) * g.line_bytes, "mask %u: strides", mask);
                if (mask == 0) CHECK(g.front_fixed == EXR_FRONT_FIXED && g.sum_bps == (size_t)(pt == EXR_PIXEL_FLOAT ? 12 : 6), "mask 0 is the three-channel file");
                if (mask == 127) CHECK(g.front_fixed == 626 && g.sum_bps == (size_t)(pt == EXR_PIXEL_FLOAT ? 64 : 42), "everything on: 626 bytes, 42 / 64 per pixel");
                ++lists;
            }
    printf("  channel lists, fronts, offsets and capacity: 128 masks, %d geometries\n", lists);
}

// ---- the leaf, every thread of the grid
static float rnd(uint32_t& seed) {
    seed = seed * 1664525u + 1013904223u;
    static const float special[] = {NAN, INFINITY, -INFINITY, -1.5f, 65504.0f, 65520.0f, 1e9f, 3e-6f, -5.9e-8f, 6.1e-5f, 0.0f, -0.0f};
    if ((seed >> 28) == 0u) return special[(seed >> 20) % 12u];
    return (float)((int32_t)(seed >> 8) % 200000) * 0.01f;
}
static float variance_serial(float s1, float s2, float n) {
    if (!(n >= 2.0f)) return 0.0f;
    volatile float mean = s1 / n, prod = s1 * mean, d = s2 - prod, q = d / (n - 1.0f);
    const float sv = q > 0.0f ? (float)q : 0.0f;
    return sv / n;
}
template <class T> static T* exact_copy(const std::vector<T>& v) {      // a 16-byte aligned heap buffer of exactly the vector's bytes: one more is a report
    void* p = nullptr;
    if (posix_memalign(&p, 16, v.size() * sizeof(T)) != 0) { fprintf(stderr, "out of memory\n"); exit(2); }
    memcpy(p, v.data(), v.size() * sizeof(T));
    return (T*)p;
}
static void check_layout(int W, int H, uint32_t mask, int pt, bool vec) {
    const ExrGeometry g = exr_geometry(W, H, pt, EXR_COMPRESSION_ZIP, 4096, mask);
    const size_t npx = (size_t)W * H;
    uint32_t seed = (uint32_t)(W * 131 + H * 7 + mask);
    std::vector<ExrF4> nc(npx), at(npx);
    std::vector<float> dist(npx), s1(npx * 3), s2(npx * 3), counts(npx);
    for (size_t p = 0; p < npx; ++p) {
        nc[p] = {rnd(seed), rnd(seed), rnd(seed), rnd(seed)}; at[p] = {rnd(seed), rnd(seed), rnd(seed), rnd(seed)}; dist[p] = rnd(seed) * 300.0f;
        counts[p] = (float)(1 + (seed >> 13) % 4u);
        for (int c = 0; c < 3; ++c) { s1[3 * p + c] = rnd(seed); s2[3 * p + c] = s1[3 * p + c] * s1[3 * p + c] / counts[p] * (0.9f + 0.001f * (float)((seed >> 9) % 2000u)); }
    }
    ExrAov v = ExrAov();
    for (int k = 0; k < g.channels; ++k) {
        if (g.ch[k].slot <= EXR_SLOT_B) continue;
        ExrPlane& pl = v.plane[v.planes++];
        pl.slot = (uint32_t)g.ch[k].slot; pl.bps = (uint32_t)g.ch[k].bps; pl.offset = (uint32_t)g.ch[k].offset;
        v.need |= exr_slot_need(g.ch[k].slot);
    }
    ExrF4* d_nc = (v.need & EXR_NEED_NC) ? exact_copy(nc) : nullptr;      // an unselected slot's buffer is null: a read of it is a report
    ExrF4* d_at = (v.need & EXR_NEED_AT) ? exact_copy(at) : nullptr;
    float* d_dist = (v.need & EXR_NEED_DIST) ? exact_copy(dist) : nullptr;
    float* d_s1 = (v.need & EXR_NEED_MOMENTS) ? exact_copy(s1) : nullptr;
    float* d_s2 = (v.need & EXR_NEED_MOMENTS) ? exact_copy(s2) : nullptr;
    float* d_counts = (v.need & EXR_NEED_DIVISOR) ? exact_copy(counts) : nullptr;
    v.nc = d_nc; v.at = d_at; v.dist = d_dist; v.s1 = d_s1; v.s2 = d_s2; v.counts = d_counts; v.samples = 1;
    const size_t SENTINEL = 16, stride = g.line_bytes + SENTINEL;
    uint8_t* lines = (uint8_t*)malloc((size_t)H * stride);
    memset(lines, 0xA5, (size_t)H * stride);
    const uint32_t groups = ((uint32_t)W + 3u) / 4u, threads = (groups + 255u) / 256u * 256u;      // the grid: whole workgroups of 256
    for (uint32_t y = 0; y < (uint32_t)H; ++y)
        for (uint32_t t = 0; t < threads; ++t) {
            const uint32_t x0 = 4u * t;
            if (x0 >= (uint32_t)W) continue;      // the kernel's own guard
            const bool ok = vec ? exr_aov_thread<true>(v, lines + y * stride, (uint32_t)g.line_bytes, (uint32_t)W, x0, y)
                                : exr_aov_thread<false>(v, lines + y * stride, (uint32_t)g.line_bytes, (uint32_t)W, x0, y);
            CHECK(ok, "%d x %d mask %u: a store was refused", W, H, mask);
        }
    for (int y = 0; y < H; ++y) {
        const uint8_t* row = lines + (size_t)y * stride;
        for (size_t k = 0; k < SENTINEL; ++k) CHECK(row[g.line_bytes + k] == 0xA5, "%d x %d mask %u: the sentinel behind line %d", W, H, mask, y);
        for (int k = 0; k < g.channels; ++k) {
            const ExrChannel& ch = g.ch[k];
            for (int x = 0; x < W; ++x) {
                const size_t p = (size_t)y * W + x;
                const uint8_t* sample = row + ch.offset + (size_t)x * ch.bps;
                if (ch.slot <= EXR_SLOT_B) { CHECK(sample[0] == 0xA5 && sample[ch.bps - 1] == 0xA5, "a colour plane was touched"); continue; }
                float value = 0.0f;
                switch (ch.slot) {
                case EXR_SLOT_Z: value = dist[p]; break;
                case EXR_SLOT_NX: value = nc[p].x; break; case EXR_SLOT_NY: value = nc[p].y; break; case EXR_SLOT_NZ: value = nc[p].z; break;
                case EXR_SLOT_COVERAGE: value = nc[p].w; break;
                case EXR_SLOT_ALBEDO_R: value = at[p].x; break; case EXR_SLOT_ALBEDO_G: value = at[p].y; break; case EXR_SLOT_ALBEDO_B: value = at[p].z; break;
                case EXR_SLOT_TRANSMITTANCE: value = at[p].w; break;
                case EXR_SLOT_SAMPLES: value = counts[p]; break;
                default: value = variance_serial(s1[3 * p + (ch.slot - EXR_SLOT_VARIANCE_R)], s2[3 * p + (ch.slot - EXR_SLOT_VARIANCE_R)], counts[p]); break;
                }
                uint32_t bits;
                memcpy(&bits, &value, 4);
                if ((bits & 0x7fffffffu) > 0x7f800000u) bits = 0u;
                if (ch.bps == 2) { uint16_t got; memcpy(&got, sample, 2); CHECK(got == (uint16_t)exr_half_bits(bits), "%d x %d mask %u %s at (%d, %d)", W, H, mask, ch.name, x, y); }
                else { uint32_t got; memcpy(&got, sample, 4); CHECK(got == bits, "%d x %d mask %u %s at (%d, %d): %08x, not %08x", W, H, mask, ch.name, x, y, got, bits); }
            }
        }
    }
    // a plane whose offset would pass the line: refused, nothing stored behind the line
    if (v.planes) {
        ExrAov bad = v;
        bad.plane[0].offset = (uint32_t)g.line_bytes - (uint32_t)(W - 1) * bad.plane[0].bps - 1u;      // its last sample would end one byte past the line
        memset(lines, 0xA5, stride);
        bool all = true;
        for (uint32_t t = 0; 4u * t < (uint32_t)W; ++t) all = exr_aov_thread<false>(bad, lines, (uint32_t)g.line_bytes, (uint32_t)W, 4u * t, 0u) && all;
        CHECK(!all, "%d x %d mask %u: a plane past the line was stored", W, H, mask);
        for (size_t k = 0; k < SENTINEL; ++k) CHECK(lines[g.line_bytes + k] == 0xA5, "a refused plane reached the sentinel");
    }
    free(lines); free(d_nc); free(d_at); free(d_dist); free(d_s1); free(d_s2); free(d_counts);
}

int main() {
    check_lists_fronts_and_capacity();
    static const int shapes[][2] = {{1, 1}, {5, 3}, {37, 17}, {1029, 2}, {1032, 1}};
    int runs = 0;
    for (const auto& wh : shapes)
        for (int pt : {EXR_PIXEL_HALF, EXR_PIXEL_FLOAT})
            for (uint32_t mask : {1u, 2u, 4u, 8u, 16u, 32u, 64u, 127u, 3u}) {
                check_layout(wh[0], wh[1], mask, pt, false);
                if ((wh[0] & 3) == 0) check_layout(wh[0], wh[1], mask, pt, true);
                ++runs;
            }
    printf("  layout leaf: every thread of %d grids\n", runs);
    CHECK(exr_variance_of_mean(3.0f, 6.0f, 2.0f) == 0.75f && exr_variance_of_mean(3.0f, 4.0f, 2.0f) == 0.0f && exr_variance_of_mean(3.0f, 6.0f, 1.0f) == 0.0f &&
          exr_variance_of_mean(3.0f, 6.0f, NAN) == 0.0f, "the variance's fixed points");
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("exr_aov_host_check: channel sort, front, offsets and capacity for 128 masks and both pixel types; the AOV layout leaf: no sanitizer report\n");
    return 0;
}

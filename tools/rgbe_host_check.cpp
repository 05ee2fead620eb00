// rgbe_host_check.cpp — the host side and the plain leaves of the Radiance HDR output (csrc/rgbe_tables.h: the sample in integers, the front, the
// geometry and capacity, the three rounds of the run-length coder) compiled for the HOST under the address and undefined-behaviour
// sanitizers.  No GPU, no library.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rgbe_host_check.cpp -o rgbe_host_check && ./rgbe_host_check
// Checked, each against a serial statement written apart from the leaf: the known answers of the header; the sample against a statement in double
// arithmetic (frexp, ldexp, floor) on random and special values in both rounding modes; the front as a string built line by line; the geometry's
// counts and capacity; and the coder — every thread's three rounds in turn, the scans as plain loops, on heap buffers of exactly W bytes and slots
// of exactly the proven bound — against a serial encoder, decoded again, on the widths of tests/rgbe_cases.py and five kinds of content.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#define DE_DEV static inline
#include "../digital_earth_amd/csrc/rgbe_tables.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint32_t lcg = 12345u;
static uint32_t rnd() { lcg = lcg * 1664525u + 1013904223u; return lcg >> 8; }

// ---- the sample, once more in double
static uint32_t pixel_serial(const float in[3], int rounding) {
    double v[3], m = 0.0;
    for (int c = 0; c < 3; ++c) {
        double x = (double)in[c];
        if (isnan(x) || x < 0.0) x = 0.0;
        if (x > ldexp(255.0, 119)) x = ldexp(255.0, 119);
        v[c] = x;
        if (x > m) m = x;
    }
    if (m < (double)1e-32f) return 0u;
    int e;
    (void)frexp(m, &e);
    uint32_t q[3];
    bool up = false;
    for (int c = 0; c < 3; ++c) { q[c] = (uint32_t)floor(ldexp(v[c], 8 - e) + (rounding ? 0.5 : 0.0)); up = up || q[c] == 256u; }
    if (up) { ++e; for (int c = 0; c < 3; ++c) q[c] = (uint32_t)floor(ldexp(v[c], 8 - e) + 0.5); }
    return q[0] | (q[1] << 8) | (q[2] << 16) | ((uint32_t)(e + 128) << 24);
}
static void check_sample() {
    CHECK(rgbe_float_bits(1e-32f) == 0x0A4FB11Fu, "the bits of 1e-32f");
    CHECK(rgbe_float_bits(ldexpf(255.0f, 119)) == RGBE_CLAMP_BITS, "the bits of 255 2^119");
    struct { float v[3]; int rounding; uint32_t want; } known[] = {
        {{1, 1, 1}, 0, 0x81808080u}, {{0.5f, 0.25f, 0.125f}, 0, 0x80204080u}, {{0.18f, 0.18f, 0.18f}, 0, 0x7EB8B8B8u}, {{65504, 1, 0}, 0, 0x900000FFu},
        {{ldexpf(255.0f, 119), 0, 0}, 0, 0xFF0000FFu}, {{0.9999999f, 0, 0}, 0, 0x800000FFu}, {{0.9999999f, 0, 0}, 1, 0x81000080u}};
    for (const auto& k : known) CHECK(rgbe_pixel(k.v[0], k.v[1], k.v[2], k.rounding) == k.want, "known answer (%g, %g, %g): %08x", k.v[0], k.v[1], k.v[2], rgbe_pixel(k.v[0], k.v[1], k.v[2], k.rounding));
    const float special[] = {NAN, INFINITY, -INFINITY, -1.0f, 1e-33f, 1e-45f, ldexpf(1.0f, 127), ldexpf(255.0f, 119), 0.9999999f, 1.0f, 1e-32f, 0.99e-32f, -0.0f, 0.0f, 3.4e38f, 1.17549435e-38f};
    unsigned long long checked = 0;
    for (int rounding = 0; rounding < 2; ++rounding) {
        for (float a : special) for (float b : special) for (float c : special) {
            const float v[3] = {a, b, c};
            CHECK(rgbe_pixel(a, b, c, rounding) == pixel_serial(v, rounding), "special (%g, %g, %g) mode %d", a, b, c, rounding);
            ++checked;
        }
        for (int i = 0; i < 2000000; ++i) {
            float v[3];
            const int base = (int)(rnd() % 250u) - 120;
            for (int c = 0; c < 3; ++c) {      // components within 2^12 of each other, mantissas random or just under a carry
                const uint32_t mant = (rnd() & 7u) == 0u ? 0x7fffffu - (rnd() & 0xffu) : rnd() & 0x7fffffu;
                uint32_t bits = ((uint32_t)(base + 127 - (int)(rnd() % 12u)) << 23) | mant;
                if ((int32_t)bits < 0) bits = 0u;
                memcpy(&v[c], &bits, 4);
            }
            const uint32_t got = rgbe_pixel(v[0], v[1], v[2], rounding), want = pixel_serial(v, rounding);
            CHECK(got == want, "pixel (%a, %a, %a) mode %d: %08x, not %08x", v[0], v[1], v[2], rounding, got, want);
            ++checked;
        }
    }
    printf("  sample: %llu pixels against the statement in double\n", checked);
}

// ---- the front and the geometry
static void check_front_and_geometry() {
    static const int sizes[][2] = {{1, 1}, {7, 3}, {8, 1100}, {1920, 1080}, {4096, 2048}, {32767, 1}, {32768, 1}};
    for (const auto& wh : sizes)
        for (int rle = 0; rle < 2; ++rle)
            for (float scale : {1.0f, 0.25f, 3.0f}) {
                const int W = wh[0], H = wh[1];
                const RgbeGeometry g = rgbe_geometry(W, H, rle, scale);
                std::string want = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nPRIMARIES=0.64 0.33 0.3 0.6 0.15 0.06 0.3127 0.329\n";
                if (scale != 1.0f) want += std::string("EXPOSURE=") + (scale == 0.25f ? "0.25" : "3") + "\n";
                want += "\n-Y " + std::to_string(H) + " +X " + std::to_string(W) + "\n";
                CHECK(g.header == want.size() && g.header <= RGBE_FRONT_MAX && memcmp(g.text, want.data(), g.header) == 0, "front of %d x %d", W, H);
                const bool coded = rle && W >= 8 && W <= 32767;
                const size_t plane = (size_t)W + ((size_t)W + 127) / 128;
                CHECK(g.rle == (coded ? 1 : 0) && g.plane_bound == plane, "coding of %d x %d", W, H);
                CHECK(g.capacity == g.header + (size_t)H * (coded ? 4 + 4 * plane : 4 * (size_t)W), "capacity of %d x %d", W, H);
                CHECK(g.pieces == (coded ? 4 * (size_t)H : 0) && g.slot_bytes % 16 == 0 && g.slot_bytes >= plane + 4 && g.plane_stride % 16 == 0 && g.plane_stride >= (size_t)W, "pieces of %d x %d", W, H);
                CHECK(g.front == (coded ? g.header : g.header + 4 * (size_t)W * H) && g.capacity + 16 < (1ull << 32), "front of %d x %d", W, H);
            }
}

// ---- the coder
static std::vector<uint8_t> code_serial(const uint8_t* p, uint32_t W) {
    std::vector<uint8_t> out, lit;
    auto flush = [&] {
        for (size_t k = 0; k < lit.size(); k += 128) { const size_t n = lit.size() - k < 128 ? lit.size() - k : 128; out.push_back((uint8_t)n); out.insert(out.end(), lit.begin() + k, lit.begin() + k + n); }
        lit.clear();
    };
    for (uint32_t i = 0; i < W;) {
        uint32_t j = i;
        while (j < W && p[j] == p[i]) ++j;
        if (j - i >= 4) {
            flush();
            for (uint32_t L = j - i; L > 0;) { const uint32_t n = L < 127 ? L : 127; out.push_back((uint8_t)(0x80 + n)); out.push_back(p[i]); L -= n; }
        } else lit.insert(lit.end(), p + i, p + j);
        i = j;
    }
    flush();
    return out;
}
static bool decodes_to(const std::vector<uint8_t>& code, const uint8_t* p, uint32_t W) {
    uint32_t x = 0;
    for (size_t at = 0; at < code.size();) {
        uint32_t n = code[at];
        if (n > 128) { n -= 128; if (at + 2 > code.size() || x + n > W) return false; for (uint32_t k = 0; k < n; ++k) if (p[x + k] != code[at + 1]) return false; at += 2; }
        else { if (!n || at + 1 + n > code.size() || x + n > W || memcmp(p + x, &code[at + 1], n)) return false; at += 1 + n; }
        x += n;
    }
    return x == W;
}
static void code_by_leaves(const uint8_t* p, uint32_t W, uint32_t threads, std::vector<uint8_t>* out, bool* ok) {
    std::vector<uint32_t> last(threads), first(threads), before(threads), next(threads), region(threads), behind(threads), n(threads);
    auto scans = [&](std::vector<uint32_t>& up, std::vector<uint32_t>& down) {      // exclusive maximum from the left, exclusive minimum from the right
        uint32_t m = 0u;
        for (uint32_t t = 0; t < threads; ++t) { const uint32_t v = last[t]; up[t] = m; m = v > m ? v : m; }
        m = W;
        for (uint32_t t = threads; t-- > 0;) { const uint32_t v = first[t]; down[t] = m; m = v < m ? v : m; }
    };
    for (uint32_t t = 0; t < threads; ++t) rgbe_round1(p, W, rgbe_span(W, t, threads), &last[t], &first[t]);
    scans(before, next);
    for (uint32_t t = 0; t < threads; ++t) rgbe_round2(p, W, rgbe_span(W, t, threads), before[t], next[t], &last[t], &first[t]);
    scans(region, behind);
    uint32_t total = 0;
    for (uint32_t t = 0; t < threads; ++t) { n[t] = rgbe_round3(p, W, rgbe_span(W, t, threads), before[t], next[t], region[t], behind[t], nullptr, 0u, 0u, ok); total += n[t]; }
    const uint32_t room = W + (W + 127u) / 128u;      // exactly the proven bound
    uint8_t* slot = (uint8_t*)malloc(room);
    memset(slot, 0xA5, room);
    uint32_t at = 0;
    for (uint32_t t = 0; t < threads; ++t) {
        const uint32_t wrote = rgbe_round3(p, W, rgbe_span(W, t, threads), before[t], next[t], region[t], behind[t], slot, at, room, ok);
        CHECK(wrote == n[t], "thread %u counted %u and wrote %u", t, n[t], wrote);
        at += wrote;
    }
    out->assign(slot, slot + (total < room ? total : room));
    CHECK(total <= room, "a plane of %u bytes coded to %u, above the bound %u", W, total, room);
    free(slot);
}
static void check_coder() {
    static const uint32_t widths[] = {8, 9, 127, 128, 129, 254, 255, 257, 300, 1023, 4097, 32767};
    unsigned long long planes = 0;
    for (uint32_t W : widths)
        for (int kind = 0; kind < 7; ++kind)
            for (int rep = 0; rep < (W > 5000 ? 1 : 6); ++rep) {
                uint8_t* p = (uint8_t*)malloc(W);
                for (uint32_t i = 0; i < W;) {
                    uint32_t n;
                    switch (kind) {
                    case 0: n = W; break;                                             // constant
                    case 1: n = 3u + (rnd() & 1u); break;                             // stretches of 3 and 4 side by side
                    case 2: { static const uint32_t l[] = {127, 128, 254, 1, 2}; n = l[rnd() % 5u]; break; }
                    case 3: n = 1; break;                                             // noise
                    case 4: n = 1u + rnd() % 6u; break;                               // short stretches around the threshold
                    case 5: n = (rnd() & 3u) ? 1u + rnd() % 3u : 100u + rnd() % 400u; break;      // long literal regions between long runs
                    default: n = 1u + rnd() % 300u; break;
                    }
                    const uint8_t v = kind == 3 ? (uint8_t)rnd() : (uint8_t)(rnd() % 3u);      // few values: neighbours often merge into one stretch
                    for (uint32_t k = 0; k < n && i < W; ++k) p[i++] = v;
                }
                const std::vector<uint8_t> want = code_serial(p, W);
                for (uint32_t threads : {(uint32_t)RGBE_THREADS, 7u}) {
                    std::vector<uint8_t> got;
                    bool ok = true;
                    code_by_leaves(p, W, threads, &got, &ok);
                    CHECK(ok, "W %u kind %d: a store did not fit the bound", W, kind);
                    CHECK(got == want, "W %u kind %d threads %u: %zu bytes, not the serial coder's %zu", W, kind, threads, got.size(), want.size());
                    CHECK(decodes_to(got, p, W), "W %u kind %d: the code does not decode to the plane", W, kind);
                }
                ++planes;
                free(p);
            }
    // a slot one byte short: the store is refused, nothing is written past it
    {
        const uint32_t W = 300;
        std::vector<uint8_t> p(W);
        for (uint32_t i = 0; i < W; ++i) p[i] = (uint8_t)rnd();
        bool ok = true;
        const RgbeSpan all = rgbe_span(W, 0, 1);
        const uint32_t n = rgbe_round3(p.data(), W, all, 0u, W, 0u, W, nullptr, 0u, 0u, &ok);
        uint8_t* slot = (uint8_t*)malloc(n - 1);
        (void)rgbe_round3(p.data(), W, all, 0u, W, 0u, W, slot, 0u, n - 1, &ok);
        CHECK(!ok && n == W + 3, "a slot one byte short was not refused");
        free(slot);
    }
    printf("  coder: %llu planes, 256 and 7 threads, against the serial coder and decoded again\n", planes);
}

int main() {
    check_sample();
    check_front_and_geometry();
    check_coder();
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("rgbe_host_check: sample, front, geometry and capacity, run-length coder: no sanitizer report\n");
    return 0;
}

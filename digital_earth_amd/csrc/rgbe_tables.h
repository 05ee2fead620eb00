// rgbe_tables.h — the Radiance HDR output (include/digital_earth_rgbe.h) as plain C++ with no HIP in it: the sample in integers, the
// geometry (rows, pieces, the proven slot and capacity), the front the host composes, and the leaves of the run-length coder that the kernels
// (rgbe_kernels.hip) and the host check (tools/rgbe_host_check.cpp) share.  The includer brings DE_DEV.
//
// THE CODER OF ONE PLANE, as the kernel runs it: W bytes p[0 .. W), `threads` threads, thread t owns the span [t span, (t + 1) span) with
// span = ceil(W / threads).  Three rounds, each a walk of a thread over its own span between two workgroup scans of one word per thread:
//   1. STRETCHES.  i starts a stretch where i == 0 or p[i] != p[i - 1].  A thread reports the last and the first start in its span; the exclusive
//      max-scan of the one and the exclusive reverse min-scan of the other tell it where the stretch that reaches into its span began and where the
//      stretch that leaves it ends.  A stretch of L >= 4 is a RUN.
//   2. LITERAL REGIONS.  With every stretch's length known to the threads it touches, a thread reports the last position in its span behind a run's end
//      (or 0) at which a literal region begins, and the first position of its span that lies in a run; the same two scans tell it where the literal
//      region that reaches into its span began and where the one that leaves it ends.
//   3. POSITIONS.  Position i emits: in a run, at j = i - start, 2 bytes where j is a multiple of 127 (the packet of min(127, L - j): 80 + count, value),
//      else none; in a literal region, at k = i - start, its byte and, where k is a multiple of 128, the count byte min(128, n - k) in front of it.
//      The exclusive sum-scan of the spans' totals is where a span's bytes go.
// Every leaf below is one thread's walk of one round; the scans are the caller's (LDS in the kernel, loops in the host check).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define RGBE_FRONT_MAX 192           // 11 + 23 + 51 + at most 26 + 1 + at most 28 bytes
#define RGBE_MAX_FLAT (1ull << 27)   // 4 W H: the coded tail counts bytes in 32 bits.  4096 x 2048 and 3840 x 2160 fit
#define RGBE_MIN_RLE_W 8             // the format's own limits of a run-length coded row
#define RGBE_MAX_RLE_W 32767
#define RGBE_THREADS 256             // of the coder's workgroup: a span is at most 128 bytes
#define RGBE_ROUND_TRUNC 0
#define RGBE_ROUND_NEAREST 1
#define RGBE_CLAMP_BITS 0x7EFF0000u  // 255 2^119, the largest RGBE value
#define RGBE_NONE 0xffffffffu        // "no such position" in a max-scan (as -1: every position + 1 is above it, see the leaves)

// ---- the sample (the header's THE SAMPLE): three float32 products -> R | G << 8 | B << 16 | E << 24
DE_DEV uint32_t rgbe_float_bits(float v) { uint32_t x; memcpy(&x, &v, 4); return x; }
// steps 1 and 2: a NaN or a negative value (its sign bit: -0 too) is +0; above 255 2^119, +inf included, is 255 2^119.  What is left orders as its bits.
DE_DEV uint32_t rgbe_clamped_bits(float v) {
    const uint32_t x = rgbe_float_bits(v);
    if ((x >> 31) || x > 0x7f800000u) return 0u;
    return x > RGBE_CLAMP_BITS ? RGBE_CLAMP_BITS : x;
}
// steps 6 and 7 for one component of bits x under the shift of the pixel's exponent, sh = 16 + Em - Ec + (1 after the carry): floor(M / 2^sh), or
// floor(M / 2^sh + 1/2) = (M + 2^(sh - 1)) >> sh, in integers.  M < 2^24: from sh = 25 on (24 when truncating) the answer is 0.
DE_DEV uint32_t rgbe_component(uint32_t x, uint32_t em, uint32_t carry, int rounding) {
    const uint32_t ec = x >> 23;
    if (ec == 0u) return 0u;      // +0 or a denormal: below 2^-126, and the pixel's step is at least 2^-114
    const uint32_t M = (x & 0x7fffffu) | 0x800000u, sh = 16u + em - ec + carry;
    if (rounding == RGBE_ROUND_NEAREST) return sh > 24u ? 0u : (M + (1u << (sh - 1u))) >> sh;
    return sh > 23u ? 0u : M >> sh;
}
DE_DEV uint32_t rgbe_pixel(float r, float g, float b, int rounding) {
    const uint32_t x[3] = {rgbe_clamped_bits(r), rgbe_clamped_bits(g), rgbe_clamped_bits(b)};
    uint32_t m = x[0] > x[1] ? x[0] : x[1];
    m = m > x[2] ? m : x[2];
    if (m < 0x0A4FB11Fu) return 0u;      // step 4: below 1e-32f, whose bits these are (tools/rgbe_host_check.cpp compares them with the literal)
    const uint32_t em = m >> 23;         // step 5: m = f 2^e with f in [0.5, 1) and e = em - 126; E = e + 128 = em + 2
    uint32_t q[3], carry = 0u;
    for (int c = 0; c < 3; ++c) q[c] = rgbe_component(x[c], em, 0u, rounding);
    if (q[0] == 256u || q[1] == 256u || q[2] == 256u) {      // only when rounding: the largest rounds up to 2^8, so e + 1 and all three again
        carry = 1u;
        for (int c = 0; c < 3; ++c) q[c] = rgbe_component(x[c], em, 1u, rounding);
    }
    uint32_t E = em + 2u + carry;
    if (E > 255u) {      // (the clamp of step 2 keeps every pixel below this: at em = 253 the largest mantissa rounds to 255)
        E = 255u;
        for (int c = 0; c < 3; ++c) { q[c] = rgbe_component(x[c], em, 0u, RGBE_ROUND_TRUNC); }
    }
    for (int c = 0; c < 3; ++c) if (q[c] > 255u) q[c] = 255u;
    return q[0] | (q[1] << 8) | (q[2] << 16) | (E << 24);
}

// ---- geometry of a W x H file
struct RgbeGeometry {
    int W, H;
    int rle;                     // the rows are run-length coded: the setting is on and 8 <= W <= 32767.  Else FLAT
    float scale;
    size_t header;               // the front's text
    size_t plane_bound;          // W + ceil(W / 128): the proven bound of one coded plane
    size_t row_bound;            // 4 + 4 plane_bound, or 4 W when flat
    size_t plane_stride;         // of a plane in the planar buffer: W rounded up to 16
    size_t pieces;               // 4 H; 0 when flat
    size_t slot_bytes;           // of a piece: plane_bound, + 4 for the row's header in plane R's piece, rounded up to 16
    size_t front;                // what lies in front of the first piece: the header; when flat the pixels too
    size_t capacity;             // header + H row_bound
    uint8_t text[RGBE_FRONT_MAX];
};
// The front: #?RADIANCE, FORMAT, PRIMARIES (Rec.709 / D65: Radiance's own default white is equal-energy), EXPOSURE unless the scale is 1, an empty
// line, the resolution.  `out` takes RGBE_FRONT_MAX; returns the length.
static inline size_t rgbe_write_front(int W, int H, float scale, uint8_t* out) {
    char text[RGBE_FRONT_MAX];
    int n = snprintf(text, sizeof(text), "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nPRIMARIES=0.64 0.33 0.3 0.6 0.15 0.06 0.3127 0.329\n");
    if (scale != 1.0f) n += snprintf(text + n, sizeof(text) - (size_t)n, "EXPOSURE=%.9g\n", (double)scale);
    n += snprintf(text + n, sizeof(text) - (size_t)n, "\n-Y %d +X %d\n", H, W);
    memcpy(out, text, (size_t)n);
    return (size_t)n;
}
static inline RgbeGeometry rgbe_geometry(int W, int H, int rle, float scale) {
    RgbeGeometry g;
    g.W = W; g.H = H; g.scale = scale;
    g.rle = rle && W >= RGBE_MIN_RLE_W && W <= RGBE_MAX_RLE_W ? 1 : 0;
    memset(g.text, 0, sizeof(g.text));
    g.header = rgbe_write_front(W, H, scale, g.text);
    g.plane_bound = (size_t)W + ((size_t)W + 127) / 128;
    g.row_bound = g.rle ? 4 + 4 * g.plane_bound : 4 * (size_t)W;
    g.plane_stride = ((size_t)W + 15) & ~(size_t)15;
    g.pieces = g.rle ? 4 * (size_t)H : 0;
    g.slot_bytes = (g.plane_bound + 4 + 15) & ~(size_t)15;
    g.front = g.rle ? g.header : g.header + 4 * (size_t)W * (size_t)H;
    g.capacity = g.header + (size_t)H * g.row_bound;
    return g;
}

// ---- the coder's leaves.  What a thread reports to a scan and takes from it:
struct RgbeSpan { uint32_t lo, hi; };      // the thread's positions [lo, hi); empty (lo == hi) behind the plane's end
DE_DEV RgbeSpan rgbe_span(uint32_t W, uint32_t t, uint32_t threads) {
    const uint32_t span = (W + threads - 1u) / threads, lo = t * span < W ? t * span : W, hi = lo + span < W ? lo + span : W;
    RgbeSpan s = {lo, hi};
    return s;
}
DE_DEV bool rgbe_starts(const uint8_t* p, uint32_t i) { return i == 0u || p[i] != p[i - 1u]; }
// round 1: *last = the last stretch start in the span + 1, or 0 (for a max-scan); *first = the first, or W (for a min-scan)
DE_DEV void rgbe_round1(const uint8_t* p, uint32_t W, RgbeSpan s, uint32_t* last, uint32_t* first) {
    *last = 0u; *first = W;
    for (uint32_t i = s.lo; i < s.hi; ++i)
        if (rgbe_starts(p, i)) { *last = i + 1u; if (*first == W) *first = i; }
}
// The stretches a span touches, walked in order: `begin` of the first comes from the max-scan (the start + 1 of the last stretch begun in front of the
// span; position 0 always starts one, so it is never 0 where lo > 0), the end of the last from the min-scan (`next`: the first start behind the span, or W).
struct RgbeWalk { uint32_t begin, end; };      // the stretch [begin, end) holding a position
DE_DEV RgbeWalk rgbe_stretch_at(const uint8_t* p, uint32_t W, RgbeSpan s, uint32_t i, uint32_t before, uint32_t next) {
    RgbeWalk w;
    uint32_t b = i;
    while (b > s.lo && !rgbe_starts(p, b)) --b;
    w.begin = rgbe_starts(p, b) ? b : before - 1u;      // b == lo and no start there: the stretch came in from the left
    uint32_t e = i + 1u;
    while (e < s.hi && !rgbe_starts(p, e)) ++e;
    w.end = e < s.hi ? e : next;
    (void)W;
    return w;
}
DE_DEV bool rgbe_is_run(RgbeWalk w) { return w.end - w.begin >= 4u; }
// round 2: *last = the last position + 1 in the span at which a literal region begins, or 0; *first = the first position of the span in a run, or W.
// `left_run`: the stretch that ends at lo (the one in front of a span that begins with a start) is a run — the caller knows it from round 1's scan:
// it is the stretch [before - 1, lo).
DE_DEV void rgbe_round2(const uint8_t* p, uint32_t W, RgbeSpan s, uint32_t before, uint32_t next, uint32_t* last, uint32_t* first) {
    *last = 0u; *first = W;
    uint32_t i = s.lo;
    bool prev_run = true;      // position 0 begins a region if it is a literal
    if (i > 0u && i < s.hi) prev_run = rgbe_starts(p, i) ? (i - (before - 1u) >= 4u) : rgbe_is_run(rgbe_stretch_at(p, W, s, i, before, next));
    while (i < s.hi) {
        const RgbeWalk w = rgbe_stretch_at(p, W, s, i, before, next);
        const bool run = rgbe_is_run(w);
        if (run && *first == W) *first = i;
        if (!run && prev_run) *last = i + 1u;      // (a stretch that came in from the left has prev_run == run: no region begins inside a stretch)
        prev_run = run;
        i = w.end < s.hi ? w.end : s.hi;
    }
}
// round 3, counting and writing in one walk.  `region` = the max-scan's answer (start + 1 of the literal region that reaches into the span, 0: none does),
// `region_end` = the min-scan's (the first run position behind the span, or W).  out == nullptr: the bytes the span emits are counted only.  Else they
// go to out[at ..) and every store is checked against `room`; returns the count either way, and *ok stays true while every store fitted.
DE_DEV uint32_t rgbe_round3(const uint8_t* p, uint32_t W, RgbeSpan s, uint32_t before, uint32_t next, uint32_t region, uint32_t first_run_behind,
                            uint8_t* out, uint32_t at, uint32_t room, bool* ok) {
    uint32_t n = 0u, i = s.lo;
    uint32_t lit_begin = region ? region - 1u : 0u;      // of the literal region in force; renewed where one begins in the span
    uint32_t lit_end = W;
    bool prev_run = true, end_known = false;
    if (i > 0u && i < s.hi) prev_run = rgbe_starts(p, i) ? (i - (before - 1u) >= 4u) : rgbe_is_run(rgbe_stretch_at(p, W, s, i, before, next));
    auto put = [&](uint32_t v) {
        if (out) { if (at + n < room) out[at + n] = (uint8_t)v; else *ok = false; }
        ++n;
    };
    while (i < s.hi) {
        const RgbeWalk w = rgbe_stretch_at(p, W, s, i, before, next);
        const uint32_t stop = w.end < s.hi ? w.end : s.hi;
        if (rgbe_is_run(w)) {
            const uint32_t L = w.end - w.begin;
            for (uint32_t j = i - w.begin; j < stop - w.begin; ++j) {      // the packets begin at j = 0, 127, 254, ...
                if (j % 127u) continue;
                put(0x80u + (L - j < 127u ? L - j : 127u)); put(p[i]);
            }
            prev_run = true; end_known = false;
        } else {
            if (prev_run) lit_begin = i;
            if (!end_known) {      // where this literal region ends, once per region: the first run position behind `stop` — in the span the walk finds it, behind it the min-scan has
                lit_end = first_run_behind;
                for (uint32_t k = stop; k < s.hi;) {
                    const RgbeWalk v = rgbe_stretch_at(p, W, s, k, before, next);
                    if (rgbe_is_run(v)) { lit_end = k; break; }
                    k = v.end < s.hi ? v.end : s.hi;
                }
                end_known = true;
            }
            for (uint32_t k = i; k < stop; ++k) {
                const uint32_t j = k - lit_begin;
                if (j % 128u == 0u) put(lit_end - k < 128u ? lit_end - k : 128u);
                put(p[k]);
            }
            prev_run = false;
        }
        i = stop;
    }
    return n;
}

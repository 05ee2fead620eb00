// bc6h_body.h — the per-block body of the BC6H_UF16 encoder (bc6h_kernels.hip, include/digital_earth_ibl_bc6h.h) and its arguments, free
// of anything of the device, so that a host build (tools/bc6h_host_check.cpp) replays it thread by thread under the sanitizers.  The includer brings
// DE_DEV.  Integers only: the header carries the definition, digital_earth_amd/bc6h.py and tests/bc6h_ref.py restate it, and the GPU equals them byte
// for byte.  A block's 48 half integers live in 32 words (R | G << 16, and B) whose indices are compile-time constants once the texel loops are
// unrolled: registers, no scratch.  Every load is of a texel whose coordinates are clamped into its image; every store is the caller's.
#pragma once
#include <stdint.h>
#include "exr_tables.h"
#include "bc6h_tables.h"

#define BC6H_THREADS 256
#define BC6H_Q0_GROUP_BLOCKS 256      // quality 0: one block per lane
#define BC6H_Q1_LANES 32              // quality 1: half a wave per block, lane k takes partition k (lane 0 also mode 11)
#define BC6H_Q1_GROUP_BLOCKS (BC6H_THREADS / BC6H_Q1_LANES)
#if defined(__HIP_DEVICE_COMPILE__)
#define BC6H_UNROLL _Pragma("unroll")
#define BC6H_NO_UNROLL _Pragma("unroll 1")
#else
#define BC6H_UNROLL
#define BC6H_NO_UNROLL
#endif

// One launch: `images` images per face (the levels of a chain; 1 for a lone image), image m of w[m] x h[m] texels at src[m] + face * w * h * 3 floats,
// its blocks at first[m] ... first[m + 1] - 1 of the face's per_face blocks.  Block b of the launch is block b % per_face of face b / per_face, and
// goes to out + 16 b: the file's order.
struct Bc6hArgs {
    const float* src[BC6H_MAX_IMAGES];
    uint32_t w[BC6H_MAX_IMAGES], h[BC6H_MAX_IMAGES], first[BC6H_MAX_IMAGES + 1];
    uint32_t images, per_face, total;
    uint8_t* out;
};

// TEXEL TO HALF
DE_DEV uint32_t bc6h_half(float v) {
    const uint32_t h = exr_half_bits(exr_sample_bits(v, 1.0f));
    return (h & 0x8000u) ? 0u : h;
}

// the 16 texels of block b, coordinates clamped to the image
DE_DEV void bc6h_load_block(const Bc6hArgs& a, uint32_t b, uint32_t* rg, uint32_t* bb) {
    const uint32_t face = b / a.per_face, r = b - face * a.per_face;
    uint32_t m = 0;
    while (m + 1 < a.images && r >= a.first[m + 1]) ++m;
    const uint32_t w = a.w[m], h = a.h[m], across = (w + 3u) / 4u, pos = r - a.first[m], bx = pos % across, by = pos / across;
    const float* image = a.src[m] + (size_t)face * (size_t)w * (size_t)h * 3;
    BC6H_UNROLL for (uint32_t t = 0; t < 16u; ++t) {
        uint32_t x = bx * 4u + (t & 3u), y = by * 4u + (t >> 2);
        x = x < w - 1u ? x : w - 1u;
        y = y < h - 1u ? y : h - 1u;
        const float* v = image + ((size_t)y * (size_t)w + (size_t)x) * 3;
        rg[t] = bc6h_half(v[0]) | (bc6h_half(v[1]) << 16);
        bb[t] = bc6h_half(v[2]);
    }
}

DE_DEV uint32_t bc6h_quantise(uint32_t h, uint32_t p) {
    const uint32_t q = ((h * 64u) / 31u) >> (16u - p), top = (1u << p) - 1u;
    return q < top ? q : top;
}
DE_DEV uint32_t bc6h_unquantise(uint32_t x, uint32_t p) {
    if (p >= 15u) return x;
    if (x == 0u) return 0u;
    if (x == (1u << p) - 1u) return 0xFFFFu;
    return ((x << 16) + 0x8000u) >> p;
}
// one palette value: the interpolation, then the final step
DE_DEV uint32_t bc6h_decoded(uint32_t a, uint32_t b, uint32_t w) { return (((a * (64u - w) + b * w + 32u) >> 6) * 31u) >> 6; }

// A candidate: the quantised ends q[3 e + c] (e = 0 ... 3: W X Y Z), the indices (4 bits a texel), the error.
struct Bc6hCand { uint32_t q[12]; uint64_t idx; uint64_t err; };

// Steps 1 - 4 for the regions `part` (bit t: the region of texel t; 0 with regions = 1), region 1's anchor, precision p and index_bits 3 or 4.
DE_DEV void bc6h_candidate(const uint32_t* rg, const uint32_t* bb, uint32_t part, uint32_t regions, uint32_t anchor1, uint32_t p, uint32_t index_bits, Bc6hCand* out) {
    uint32_t u[12];      // the unquantised ends
    BC6H_UNROLL for (uint32_t r = 0; r < 2u; ++r) {
        const uint32_t mask = r ? part : ~part & 0xFFFFu;
        uint32_t lo[3] = {0xFFFFu, 0xFFFFu, 0xFFFFu}, hi[3] = {0u, 0u, 0u}, s[3] = {0u, 0u, 0u}, n = 0u;
        uint64_t srg = 0u, srb = 0u;
        BC6H_UNROLL for (uint32_t t = 0; t < 16u; ++t) {
            if (!((mask >> t) & 1u)) continue;
            const uint32_t v[3] = {rg[t] & 0xFFFFu, rg[t] >> 16, bb[t]};
            for (int c = 0; c < 3; ++c) { lo[c] = v[c] < lo[c] ? v[c] : lo[c]; hi[c] = v[c] > hi[c] ? v[c] : hi[c]; s[c] += v[c]; }
            srg += (uint64_t)(v[0] * v[1]); srb += (uint64_t)(v[0] * v[2]);      // each product is below 2^30
            ++n;
        }
        if (r >= regions) { for (int c = 0; c < 3; ++c) { lo[c] = 0u; hi[c] = 0u; } }
        // the diagonal: n sum(R C) - sum(R) sum(C) < 0 exchanges C's ends
        const int64_t cg = (int64_t)((uint64_t)n * srg) - (int64_t)((uint64_t)s[0] * (uint64_t)s[1]);
        const int64_t cb = (int64_t)((uint64_t)n * srb) - (int64_t)((uint64_t)s[0] * (uint64_t)s[2]);
        if (cg < 0) { const uint32_t x = lo[1]; lo[1] = hi[1]; hi[1] = x; }
        if (cb < 0) { const uint32_t x = lo[2]; lo[2] = hi[2]; hi[2] = x; }
        for (int c = 0; c < 3; ++c) {
            out->q[6 * r + c] = bc6h_quantise(lo[c], p);
            out->q[6 * r + 3 + c] = bc6h_quantise(hi[c], p);
            u[6 * r + c] = bc6h_unquantise(out->q[6 * r + c], p);
            u[6 * r + 3 + c] = bc6h_unquantise(out->q[6 * r + 3 + c], p);
        }
    }
    // the indices: palette entries outside, texels inside; strictly less: ties stay with the lower index
    uint32_t best[16];
    BC6H_UNROLL for (uint32_t t = 0; t < 16u; ++t) best[t] = 0xFFFFFFFFu;
    uint64_t idx = 0u;
    const uint32_t per_region = 1u << index_bits;
    BC6H_NO_UNROLL for (uint32_t k = 0; k < 16u; ++k) {
        const uint32_t r = regions == 2u ? k >> 3 : 0u, i = regions == 2u ? k & 7u : k;
        const uint32_t w = index_bits == 3u ? BC6H_WEIGHT3[i & 7u] : BC6H_WEIGHT4[i];
        const uint32_t mask = r ? part : ~part & 0xFFFFu;
        const uint32_t pr = bc6h_decoded(r ? u[6] : u[0], r ? u[9] : u[3], w), pg = bc6h_decoded(r ? u[7] : u[1], r ? u[10] : u[4], w), pb = bc6h_decoded(r ? u[8] : u[2], r ? u[11] : u[5], w);
        BC6H_UNROLL for (uint32_t t = 0; t < 16u; ++t) {
            const int32_t dr = (int32_t)pr - (int32_t)(rg[t] & 0xFFFFu), dg = (int32_t)pg - (int32_t)(rg[t] >> 16), db = (int32_t)pb - (int32_t)bb[t];
            const uint32_t d = (uint32_t)(dr * dr) + (uint32_t)(dg * dg) + (uint32_t)(db * db);      // 3 * 0x7BFF^2 < 2^32
            if (((mask >> t) & 1u) && d < best[t]) { best[t] = d; idx = (idx & ~(0xFull << (4u * t))) | ((uint64_t)i << (4u * t)); }
        }
    }
    uint64_t err = 0u;
    BC6H_UNROLL for (uint32_t t = 0; t < 16u; ++t) err += best[t];
    // the anchors: a set top bit exchanges the region's ends and complements its indices
    BC6H_UNROLL for (uint32_t r = 0; r < 2u; ++r) {
        if (r >= regions) continue;
        const uint32_t anchor = r ? anchor1 : 0u, mask = r ? part : ~part & 0xFFFFu;
        if (!(((uint32_t)(idx >> (4u * anchor)) >> (index_bits - 1u)) & 1u)) continue;
        uint64_t flip = 0u;
        BC6H_UNROLL for (uint32_t t = 0; t < 16u; ++t) if ((mask >> t) & 1u) flip |= (uint64_t)(per_region - 1u) << (4u * t);
        idx ^= flip;
        for (int c = 0; c < 3; ++c) { const uint32_t x = out->q[6 * r + c]; out->q[6 * r + c] = out->q[6 * r + 3 + c]; out->q[6 * r + 3 + c] = x; }
    }
    out->idx = idx;
    out->err = err;
}

// Step 5: every delta against region 0's first end fits a signed field of `bits` bits (0: a direct mode, always feasible)
DE_DEV bool bc6h_feasible(const Bc6hCand& c, uint32_t bits) {
    if (bits == 0u) return true;
    const int32_t half = 1 << (bits - 1u);
    bool ok = true;
    BC6H_UNROLL for (int k = 3; k < 12; ++k) {
        const int32_t d = (int32_t)c.q[k] - (int32_t)c.q[k % 3];
        ok = ok && d >= -half && d < half;
    }
    return ok;
}

DE_DEV void bc6h_put(uint64_t* lo, uint64_t* hi, uint32_t pos, uint64_t v, uint32_t n) {
    if (pos < 64u) { *lo |= v << pos; if (pos + n > 64u) *hi |= v >> (64u - pos); }
    else *hi |= v << (pos - 64u);
}
// The block of mode `mode` (1 ... 14) from the ends themselves: the deltas of a transformed mode are made here, and the fields go where the mode's
// layout table says.
DE_DEV void bc6h_pack(uint32_t mode, const Bc6hCand& c, uint32_t partition, uint32_t* words) {
    const Bc6hMode& m = BC6H_MODE[mode - 1u];
    uint64_t f[4] = {0u, 0u, 0u, 0u};      // 16 bits a field, four fields a word
    BC6H_UNROLL for (uint32_t k = 0; k < 12u; ++k) {
        const uint32_t bits = m.delta[k % 3u];
        const uint32_t v = (k < 3u || bits == 0u) ? c.q[k] : (c.q[k] - c.q[k % 3u]) & ((1u << bits) - 1u);
        f[k >> 2] |= (uint64_t)v << (16u * (k & 3u));
    }
    f[3] |= (uint64_t)partition;      // field 12
    uint64_t lo = m.value, hi = 0u;
    uint32_t pos = m.count;
    BC6H_NO_UNROLL for (uint32_t k = 0; k < (uint32_t)BC6H_LAYOUT_RUNS; ++k) {
        const uint32_t run = BC6H_LAYOUT[mode - 1u][k];
        if (run == 0u) break;
        const uint32_t field = run & 15u, low = (run >> 4) & 15u, count = (run >> 8) & 15u, word = field >> 2;
        const uint64_t from = word == 0u ? f[0] : word == 1u ? f[1] : word == 2u ? f[2] : f[3];
        uint32_t v = ((uint32_t)(from >> (16u * (field & 3u))) & 0xFFFFu) >> low & ((1u << count) - 1u);
        if (run & 0x1000u) { uint32_t rev = 0u; for (uint32_t b = 0; b < count; ++b) rev |= ((v >> b) & 1u) << (count - 1u - b); v = rev; }
        bc6h_put(&lo, &hi, pos, v, count);
        pos += count;
    }
    const uint32_t index_bits = m.regions == 2u ? 3u : 4u, anchor1 = m.regions == 2u ? BC6H_ANCHOR[partition & 31u] : 0u;
    BC6H_UNROLL for (uint32_t t = 0; t < 16u; ++t) {
        const uint32_t n = index_bits - ((t == 0u || (m.regions == 2u && t == anchor1)) ? 1u : 0u);
        bc6h_put(&lo, &hi, pos, (uint32_t)(c.idx >> (4u * t)) & ((1u << n) - 1u), n);
        pos += n;
    }
    words[0] = (uint32_t)lo; words[1] = (uint32_t)(lo >> 32); words[2] = (uint32_t)hi; words[3] = (uint32_t)(hi >> 32);
}

// QUALITY 0: mode 11 alone.
DE_DEV void bc6h_encode_q0(const uint32_t* rg, const uint32_t* bb, uint32_t* words) {
    Bc6hCand c;
    bc6h_candidate(rg, bb, 0u, 1u, 0u, 10u, 4u, &c);
    bc6h_pack(11u, c, 0u, words);
}

// QUALITY 1, lane k = 0 ... 31 of a block's half wave: partition k in the feasible mode of highest precision among 1, 6, 2, 10 (and, in lane 0, mode
// 11 ahead of it).  The lane's key is (error, order) with order 0 for mode 11 and k + 1 for partition k; the block takes the least key of its 32
// lanes, and that lane's words.
DE_DEV void bc6h_lane_q1(const uint32_t* rg, const uint32_t* bb, uint32_t k, uint64_t* err, uint32_t* order, uint32_t* words) {
    static constexpr uint8_t choice[4][3] = {{1, 10, 5}, {6, 9, 5}, {2, 7, 6}, {10, 6, 0}};      // mode, precision, delta bits
    Bc6hCand c;
    uint32_t mode = 10u;
    BC6H_NO_UNROLL for (uint32_t o = 0; o < 4u; ++o) {
        bc6h_candidate(rg, bb, BC6H_PARTITION[k], 2u, BC6H_ANCHOR[k], choice[o][1], 3u, &c);
        mode = choice[o][0];
        if (bc6h_feasible(c, choice[o][2])) break;
    }
    bc6h_pack(mode, c, k, words);
    *err = c.err;
    *order = k + 1u;
    if (k == 0u) {
        uint32_t one[4];
        bc6h_candidate(rg, bb, 0u, 1u, 0u, 10u, 4u, &c);
        if (c.err <= *err) {
            bc6h_pack(11u, c, 0u, one);
            for (int j = 0; j < 4; ++j) words[j] = one[j];
            *err = c.err;
            *order = 0u;
        }
    }
}

// ibl_body.h — the per-texel bodies of the IBL kernels (ibl_kernels.hip, include/digital_earth_ibl.h) and their arguments, free of
// anything of the device, so that a host build (tools/ibl_host_check.cpp) replays them thread by thread under the sanitizers.  The includer brings
// DE_DEV and panorama_body.h's leaves PANO_SQRT(x), PANO_FLOOR(x) (and PANO_SINCOS, which nothing here calls).  Every operation is a float32
// operation rounded on its own (the unit is compiled with -ffp-contract=off); the header carries the definition and tests/ibl_ref.py restates it.
// Every index is clamped into its buffer before its load: a tap into [0, e - 1]^2 of one of six faces of a level 0 ... M - 1 (the sample table's
// levels are made by ibl_tables.h inside that range), a texel by the caller's range check.  No atomics, no scratch.
#pragma once
#include <stdint.h>
#include "panorama_body.h"
#include "exr_tables.h"
#include "ibl_tables.h"

#define IBL_TILE 16               // one workgroup = one 16 x 16 tile of one face; a wave = an 8 x 8 block of it
#define IBL_THREADS 256

struct IblLevelArgs {             // the mip chain, and what one launch writes
    const float* mips;            // [M] blocks of [6][e][e][3], level-major
    float* out;                   // the block of the level being written: [6][e][e][3]
    const IblSample* tab;         // ibl_spec_texel: the level's kept samples
    const float* omega;           // ibl_sh_terms: [es][es]
    int n;                        // kept samples
    int E, M, e;                  // the chain's edge and levels; the edge of `out`
    uint32_t off[IBL_MAX_LEVELS]; // floats in front of level m of `mips`
};

// thread t of a tile -> its texel in the tile: wave t >> 6 owns the 8 x 8 block (wave & 1, wave >> 1), lane l the texel (l & 7, l >> 3) of it
DE_DEV void ibl_tile_texel(int t, int* il, int* jl) {
    const int wave = t >> 6, lane = t & 63;
    *il = (wave & 1) * 8 + (lane & 7);
    *jl = (wave >> 1) * 8 + (lane >> 3);
}

// the header's face table: (a, b) of face k -> direction, not normalised
DE_DEV void ibl_face_dir(int face, float a, float b, float* d) {
    switch (face) {
        case 0: d[0] = 1.0f; d[1] = -b; d[2] = -a; break;
        case 1: d[0] = -1.0f; d[1] = -b; d[2] = a; break;
        case 2: d[0] = a; d[1] = 1.0f; d[2] = b; break;
        case 3: d[0] = a; d[1] = -1.0f; d[2] = -b; break;
        case 4: d[0] = a; d[1] = -b; d[2] = 1.0f; break;
        default: d[0] = -a; d[1] = -b; d[2] = -1.0f; break;
    }
}
DE_DEV float ibl_coord(int k, int n) { return (float)(2 * k + 1) / (float)n - 1.0f; }
DE_DEV void ibl_normal(int face, int i, int j, int e, float* n) {
    float d[3];
    ibl_face_dir(face, ibl_coord(i, e), ibl_coord(j, e), d);
    const float len = PANO_SQRT((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    n[0] = d[0] / len; n[1] = d[1] / len; n[2] = d[2] / len;
}

// THE LOOKUP: a direction in one level of the chain, `level` = [6][e][e][3], bilinear with taps clamped at the face's edge.
DE_DEV void ibl_lookup(const float* level, int e, float x, float y, float z, float* rgb) {
    const float ax_ = x < 0.0f ? -x : x, ay_ = y < 0.0f ? -y : y, az_ = z < 0.0f ? -z : z;
    int face;
    float s, t;
    if (ax_ >= ay_ && ax_ >= az_) { face = x < 0.0f ? 1 : 0; s = (x < 0.0f ? z : -z) / ax_; t = -y / ax_; }
    else if (ay_ >= az_) { face = y < 0.0f ? 3 : 2; s = x / ay_; t = (y < 0.0f ? -z : z) / ay_; }
    else { face = z < 0.0f ? 5 : 4; s = (z < 0.0f ? -x : x) / az_; t = -y / az_; }
    const float half = (float)e * 0.5f, top = (float)(e - 1);
    float X = (s + 1.0f) * half - 0.5f, Y = (t + 1.0f) * half - 0.5f;
    X = X > 0.0f ? (X < top ? X : top) : 0.0f;      // NaN gives 0
    Y = Y > 0.0f ? (Y < top ? Y : top) : 0.0f;
    const int i0 = (int)PANO_FLOOR(X), j0 = (int)PANO_FLOOR(Y);
    const int i1 = i0 + 1 < e - 1 ? i0 + 1 : e - 1, j1 = j0 + 1 < e - 1 ? j0 + 1 : e - 1;
    const float ax = X - (float)i0, ay = Y - (float)j0;
    const float* f = level + (size_t)face * (size_t)e * (size_t)e * 3;
    const float* c00 = f + ((size_t)j0 * (size_t)e + (size_t)i0) * 3;
    const float* c10 = f + ((size_t)j0 * (size_t)e + (size_t)i1) * 3;
    const float* c01 = f + ((size_t)j1 * (size_t)e + (size_t)i0) * 3;
    const float* c11 = f + ((size_t)j1 * (size_t)e + (size_t)i1) * 3;
    for (int ch = 0; ch < 3; ++ch) {
        const float t0 = c00[ch] + ax * (c10[ch] - c00[ch]);
        const float t1 = c01[ch] + ax * (c11[ch] - c01[ch]);
        rgb[ch] = t0 + ay * (t1 - t0);
    }
}

// 1. the base level: texel (i, j) of face `face` at edge E from the six linear slots of `p`, S x S sub-positions, the panorama's running mean
DE_DEV void ibl_base_texel(const PanoArgs& p, float* out, int E, int S, int face, int i, int j) {
    float mean[3] = {0.0f, 0.0f, 0.0f};
    int k = 0;
    for (int q = 0; q < S; ++q)
        for (int s = 0; s < S; ++s) {
            float d[3], v[3];
            ibl_face_dir(face, ibl_coord(i * S + s, E * S), ibl_coord(j * S + q, E * S), d);
            pano_sample(p, d[0], d[1], d[2], v);
            ++k;
            if (k == 1) { mean[0] = v[0]; mean[1] = v[1]; mean[2] = v[2]; }
            else {
                const float w = 1.0f / (float)k;
                for (int ch = 0; ch < 3; ++ch) mean[ch] = mean[ch] + (v[ch] - mean[ch]) * w;
            }
        }
    float* o = out + (((size_t)face * (size_t)E + (size_t)j) * (size_t)E + (size_t)i) * 3;
    o[0] = mean[0]; o[1] = mean[1]; o[2] = mean[2];
}

// 2. the mip chain: texel (i, j) of face `face` of a level of edge e from `src`, the level above (edge 2 e)
DE_DEV void ibl_mip_texel(const float* src, float* dst, int e, int face, int i, int j) {
    const size_t e2 = (size_t)e * 2;
    const float* a = src + (((size_t)face * e2 + (size_t)j * 2) * e2 + (size_t)i * 2) * 3;
    const float* c = a + e2 * 3;
    float* o = dst + (((size_t)face * (size_t)e + (size_t)j) * (size_t)e + (size_t)i) * 3;
    for (int ch = 0; ch < 3; ++ch) o[ch] = ((a[ch] + a[3 + ch]) + (c[ch] + c[3 + ch])) * 0.25f;
}

// 3. a specular level: texel (i, j) of face `face` of a.out (edge a.e), the weighted running mean over the level's kept samples
DE_DEV void ibl_spec_texel(const IblLevelArgs& a, int face, int i, int j) {
    float N[3], T[3], B[3];
    ibl_normal(face, i, j, a.e, N);
    const float au = N[1] < 0.0f ? -N[1] : N[1];
    if (au < 0.999f) {
        const float tl = PANO_SQRT(N[2] * N[2] + N[0] * N[0]);
        T[0] = N[2] / tl; T[1] = 0.0f; T[2] = -N[0] / tl;
    } else {
        const float tl = PANO_SQRT(N[2] * N[2] + N[1] * N[1]);
        T[0] = 0.0f; T[1] = -N[2] / tl; T[2] = N[1] / tl;
    }
    B[0] = N[1] * T[2] - N[2] * T[1];
    B[1] = N[2] * T[0] - N[0] * T[2];
    B[2] = N[0] * T[1] - N[1] * T[0];
    float m[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < a.n; ++k) {
        const IblSample s = a.tab[k];                 // the same entry in every lane: a scalar load
        const float two = 2.0f * s.hz;
        float L[3];
        for (int c = 0; c < 3; ++c) {
            const float H = (T[c] * s.hx + B[c] * s.hy) + N[c] * s.hz;
            L[c] = two * H - N[c];
        }
        float v[3];
        ibl_lookup(a.mips + a.off[s.l0], a.E >> s.l0, L[0], L[1], L[2], v);
        if (s.frac != 0.0f) {
            float v1[3];
            ibl_lookup(a.mips + a.off[s.l1], a.E >> s.l1, L[0], L[1], L[2], v1);
            for (int c = 0; c < 3; ++c) v[c] = v[c] + s.frac * (v1[c] - v[c]);
        }
        for (int c = 0; c < 3; ++c) m[c] = m[c] + (v[c] - m[c]) * s.coef;
    }
    float* o = a.out + (((size_t)face * (size_t)a.e + (size_t)j) * (size_t)a.e + (size_t)i) * 3;
    o[0] = m[0]; o[1] = m[1]; o[2] = m[2];
}

// 4. SH9: the 27 terms [c][b] of texel t = (face es + j) es + i of `level` (edge es), with the solid-angle table omega [es][es]
DE_DEV void ibl_sh_terms(const float* level, const float* omega, int es, int t, float* terms) {
    const int i = t % es, j = (t / es) % es, face = t / (es * es);
    float n[3], y[9];
    ibl_normal(face, i, j, es, n);
    const float x = n[0], yy = n[1], z = n[2];
    y[0] = (float)0.28209479177387814;
    y[1] = (float)0.4886025119029199 * yy;
    y[2] = (float)0.4886025119029199 * z;
    y[3] = (float)0.4886025119029199 * x;
    y[4] = (float)1.0925484305920792 * (x * yy);
    y[5] = (float)1.0925484305920792 * (yy * z);
    y[6] = (float)0.31539156525252005 * (3.0f * (z * z) - 1.0f);
    y[7] = (float)1.0925484305920792 * (x * z);
    y[8] = (float)0.5462742152960396 * (x * x - yy * yy);
    const float dw = omega[j * es + i];
    const float* v = level + (size_t)t * 3;
    for (int b = 0; b < 9; ++b) {
        const float wy = y[b] * dw;
        for (int c = 0; c < 3; ++c) terms[c * 9 + b] = v[c] * wy;
    }
}
// the cosine lobe's factor of coefficient b
DE_DEV float ibl_sh_band_factor(int b) {
    return b == 0 ? (float)3.14159265358979323846 : b < 4 ? (float)(2.0 * 3.14159265358979323846 / 3.0) : (float)(3.14159265358979323846 / 4.0);
}

// 5. the file: texel `idx` of the payload, face-major, each face followed by its L levels.  level 0 comes from `mips`, level l >= 1 from `spec`, the
// specular levels' blocks [l - 1] at spec_off[l] floats.  RGBA, A = 1; half: 8 bytes, float: 16.
struct IblPackArgs { const float* mips; const float* spec; uint8_t* out; int E, L, half; uint32_t texels_per_face; uint32_t spec_off[IBL_MAX_LEVELS]; };
DE_DEV void ibl_pack_texel(const IblPackArgs& a, uint32_t idx) {
    const uint32_t face = idx / a.texels_per_face;
    uint32_t r = idx - face * a.texels_per_face;
    int l = 0;
    while (l < a.L - 1 && r >= (uint32_t)(a.E >> l) * (uint32_t)(a.E >> l)) { r -= (uint32_t)(a.E >> l) * (uint32_t)(a.E >> l); ++l; }
    const size_t e = (size_t)(a.E >> l);
    const float* v = (l == 0 ? a.mips : a.spec + a.spec_off[l]) + ((size_t)face * e * e + (size_t)r) * 3;
    if (a.half) {
        uint16_t* o = (uint16_t*)(a.out + (size_t)idx * 8);
        for (int c = 0; c < 3; ++c) o[c] = (uint16_t)exr_half_bits(exr_sample_bits(v[c], 1.0f));
        o[3] = (uint16_t)0x3c00u;
    } else {
        float* o = (float*)(a.out + (size_t)idx * 16);
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = 1.0f;
    }
}

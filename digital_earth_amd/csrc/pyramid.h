// pyramid.h — the tent pyramid that the bloom (bloom_kernels.hip) and local exposure (local_exposure_kernels.hip, §15) share: the plan
// of its levels on the host, and one level down on the device — a workgroup makes 16 x 16 outputs from a 34 x 34 tile of the level above, staged in
// LDS, in a row pass and a column pass.  The users differ in the number of planes NC (3: rgb; 2: (l w, w)) and in the element a level stores (float4
// with w = 0; float2).  Every phase between two barriers is a function of (thread, workgroup), so a kernel reads "phase, __syncthreads(), phase" and a
// host build (tools/local_exposure_host_check.cpp) runs the phases one workgroup at a time under the sanitizers.  The includer brings DE_DEV and the
// vector types.
#pragma once
#include <stddef.h>

#define PYR_MAX_LEVELS 10

// The pyramid of a W x H image: level l is ((w + 1) >> 1, (h + 1) >> 1) of level l - 1; L = `levels`, reduced so that halving stops before a level
// whose smaller side would be below 2, never less than 1.  off[l]: where level l starts in a buffer that holds the levels 1 .. L back to back, in
// elements; the offsets of a level do not depend on `levels`.  Host code.
struct PyramidPlan { int L; int w[PYR_MAX_LEVELS + 1], h[PYR_MAX_LEVELS + 1]; size_t off[PYR_MAX_LEVELS + 1]; size_t total; };
inline PyramidPlan pyr_plan(int W, int H, int levels) {
    PyramidPlan p;
    p.L = 0; p.w[0] = W; p.h[0] = H; p.off[0] = 0; p.total = 0;
    while (p.L < levels) {
        const int w = (p.w[p.L] + 1) >> 1, h = (p.h[p.L] + 1) >> 1;
        if (p.L >= 1 && (w < h ? w : h) < 2) break;
        ++p.L;
        p.w[p.L] = w; p.h[p.L] = h; p.off[p.L] = p.total;
        p.total += (size_t)w * (size_t)h;
    }
    return p;
}

#define PYR_SRC_COLS 40      // stage 0: the 34 source columns 32 bx - 1 .. 32 bx + 32 lie in the ten groups of 4 pixels from 32 bx - 4 on
#define PYR_SRC_STRIDE 41    // odd row strides: the 16 lanes of the next row start on an odd bank, so the stride-2 reads of the row pass do not collide
#define PYR_LVL_STRIDE 35
#define PYR_H_STRIDE 24      // two rows down is 48 = 16 mod 32 banks on: the column pass of lanes (x, y) and (x, y + 1) covers all 32 banks once

DE_DEV int pyr_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
DE_DEV float pyr_tent4(float p0, float p1, float p2, float p3) { return (0.125f * p0 + 0.375f * p1) + (0.375f * p2 + 0.125f * p3); }
// far neighbour of fine index x on the coarse level of n entries: near - 1 for even x, near + 1 for odd x, clamped
DE_DEV int pyr_far(int x, int n) { return pyr_clampi((x & 1) ? (x >> 1) + 1 : (x >> 1) - 1, 0, n - 1); }

// An element of a level <-> its planes.
DE_DEV void pyr_planes(const float4& v, float* c) { c[0] = v.x; c[1] = v.y; c[2] = v.z; }
DE_DEV void pyr_planes(const float2& v, float* c) { c[0] = v.x; c[1] = v.y; }
DE_DEV void pyr_element(const float* c, float4* v) { v->x = c[0]; v->y = c[1]; v->z = c[2]; v->w = 0.0f; }
DE_DEV void pyr_element(const float* c, float2* v) { v->x = c[0]; v->y = c[1]; }

// A level (Ws, Hs) -> its staged tile.  src: NC planes of 34 rows; plane row r is source row 32 by - 1 + r, plane column k is source column
// 32 bx - 1 + k; only rows and columns inside the level are staged, and the passes' clamped indices read only those.
template <int NC, class T>
DE_DEV void pyr_stage_level(const T* in, int Ws, int Hs, float (*src)[34][PYR_LVL_STRIDE], int t, int bx, int by) {
    const int c0 = bx * 32 - 1, r0 = by * 32 - 1;
    for (int it = t; it < 34 * 34; it += 256) {
        const int row = it / 34, col = it - row * 34;
        const int j = r0 + row, i = c0 + col;
        if (j < 0 || j >= Hs || i < 0 || i >= Ws) continue;
        float v[NC];
        pyr_planes(in[(size_t)j * Ws + i], v);
        for (int c = 0; c < NC; ++c) src[c][row][col] = v[c];
    }
}
// Row pass: 34 x 16 values per plane.  c0: the source column of plane column 0 (32 bx - 4 from stage 0, 32 bx - 1 from a level).
template <int NC, int STRIDE>
DE_DEV void pyr_row_pass(const float (*src)[34][STRIDE], float (*hb)[34][PYR_H_STRIDE], int t, int bx, int by, int c0, int Ws, int Hs, int Wd) {
    const int X0 = bx * 16, r0 = by * 32 - 1;
    for (int it = t; it < 34 * 16; it += 256) {
        const int row = it >> 4, x = it & 15, X = X0 + x, j = r0 + row;
        if (j < 0 || j >= Hs || X >= Wd) continue;
        const int k0 = pyr_clampi(2 * X - 1, 0, Ws - 1) - c0, k1 = 2 * X - c0, k2 = pyr_clampi(2 * X + 1, 0, Ws - 1) - c0, k3 = pyr_clampi(2 * X + 2, 0, Ws - 1) - c0;
        for (int c = 0; c < NC; ++c) hb[c][row][x] = pyr_tent4(src[c][row][k0], src[c][row][k1], src[c][row][k2], src[c][row][k3]);
    }
}
// Column pass: 16 x 16 outputs of (Wd, Hd) = ((Ws + 1) >> 1, (Hs + 1) >> 1).
template <int NC, class T>
DE_DEV void pyr_col_pass(const float (*hb)[34][PYR_H_STRIDE], int t, int bx, int by, int Hs, int Wd, int Hd, T* out) {
    const int r0 = by * 32 - 1;
    const int x = t & 15, y = t >> 4, X = bx * 16 + x, Y = by * 16 + y;
    if (X >= Wd || Y >= Hd) return;
    const int q0 = pyr_clampi(2 * Y - 1, 0, Hs - 1) - r0, q1 = 2 * Y - r0, q2 = pyr_clampi(2 * Y + 1, 0, Hs - 1) - r0, q3 = pyr_clampi(2 * Y + 2, 0, Hs - 1) - r0;
    float v[NC];
    for (int c = 0; c < NC; ++c) v[c] = pyr_tent4(hb[c][q0][x], hb[c][q1][x], hb[c][q2][x], hb[c][q3][x]);
    T o;
    pyr_element(v, &o);
    out[(size_t)Y * Wd + X] = o;
}

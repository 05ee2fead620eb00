/* digital_earth_ibl.h — opt-in image-based-lighting output of libdigitalearth_hip.so: a GGX-prefiltered cube map chain and the nine spherical-harmonic
 * coefficients of the irradiance, baked on the GPU from the six LINEAR face slots of include/digital_earth_environment.h (same library, ABI 6,
 * additions only).  A context that never calls de_ibl_build allocates and runs nothing new, and every other fetch returns the bytes
 * it returned before this header existed.
 *
 * ARITHMETIC.  float32, every operation rounded on its own, no fused operation, no hardware transcendental: the contract of digital_earth.h.  The
 * kernels use +, -, *, IEEE division, the correctly rounded square root and floor; everything transcendental (the GGX sample set, the level of
 * detail of a sample, the texel solid angles) is a TABLE computed in double on the host and rounded once, as the panorama's longitude tables are.
 * tests/ibl_ref.py restates all of this in numpy, and the GPU equals it bit for bit.
 *
 * CUBE FACES, in the panorama's frame basis[9] = r, u, f (de_panorama).  Face 0 ... 5 = +r, -r, +u, -u, +f, -f: the DDS order +X -X +Y -Y +Z -Z with
 * X = r, Y = u, Z = f (a left-handed frame, as the format's).  A face of edge e is e rows of e texels, row j = 0 at the TOP, column i = 0 at the LEFT
 * seen from inside the cube: index (j e + i) 3 + c.  With a = s(i), b = s(j) and s(k) = (float)(2 k + 1) / (float)e - 1 (IEEE division), the
 * direction (dr, du, df) of texel (i, j), not normalised, is
 *     +r ( 1, -b, -a)    -r (-1, -b,  a)    +u ( a,  1,  b)    -u ( a, -1, -b)    +f ( a, -b,  1)    -f (-a, -b, -1).
 * Back: the face of a direction is the component of largest magnitude, ties to r, then u, then f (digital_earth_panorama.h's rule); with ma that
 * magnitude, (sc, tc) = +r (-df, -du), -r (df, -du), +u (dr, df), -u (dr, -df), +f (dr, -du), -f (-dr, -du), and s = sc / ma, t = tc / ma.
 *
 * 1. BASE LEVEL, edge E.  Texel (i, j) of face k takes S x S sub-positions (S = supersample), sub-position (p, q) at a = (float)(2 (i S + p) + 1) /
 *    (float)(E S) - 1, b likewise with j and q; its direction by the table above is sampled from the six linear slots by the panorama's per-direction
 *    sample (digital_earth_panorama.h: face, in-face coordinates, pixel coordinates, four taps; the slots' apron makes it seamless).  The
 *    sub-positions are averaged in the order p ascending inside q ascending by the panorama's running mean m_k = m_(k-1) + (v_k - m_(k-1)) fl32(1/k).
 * 2. MIP CHAIN, levels 1 ... M - 1 with M = log2(E) + 1, level m of edge E >> m, per face: texel (i, j) = ((A + B) + (C + D)) * 0.25 with
 *    A = (2i, 2j), B = (2i + 1, 2j), C = (2i, 2j + 1), D = (2i + 1, 2j + 1) of the level above, (column, row).  A constant survives exactly.
 * 3. SPECULAR LEVELS l = 1 ... L - 1, level l of edge e = E >> l and roughness rho = l / (L - 1), alpha = rho^2.  Level 0 IS the base level.
 *    THE SAMPLE TABLE of a level, in double: for k = 0 ... K - 1, xi1 = (k + 0.5) / K, xi2 = the base-2 radical inverse of k, c2 = (1 - xi1) /
 *    (1 + (alpha^2 - 1) xi1), ct = sqrt(c2), st = sqrt(1 - c2), phi = 2 pi xi2; the half-vector in the tangent frame h = (st cos phi, st sin phi, ct);
 *    since N = V, N.L = w = 2 c2 - 1, and a sample with w <= 0 is DROPPED; D = alpha^2 / (pi (c2 (alpha^2 - 1) + 1)^2), pdf = D / 4,
 *    Omega_s = 1 / (K pdf), Omega_p = 4 pi / (6 E^2); lod = max(0, log2(Omega_s / Omega_p) / 2) + lod_bias clamped to [0, M - 1]; l0 = floor(lod),
 *    frac = lod - l0 (l0 = M - 1: frac = 0), l1 = min(l0 + 1, M - 1); W = the running sum of the kept w, coef = w / W.  Rounded once to float32:
 *    h, frac, coef.  The first kept sample has coef = 1.
 *    THE TEXEL: d = its direction by the table above, len = sqrt((dr dr + du du) + df df), N = d / len (three divisions).  The tangent frame:
 *    |N.u| < 0.999: T' = (N.f, 0, -N.r), else T' = (0, -N.f, N.u); T = T' / sqrt(sum of the squares of its two non-zero components, in the order
 *    written); B = N x T, each component x y - z w with both products rounded.  Per kept sample in table order: H = (T hx + B hy) + N hz per
 *    component; Ld = (2 hz) H - N; the value v = the lookup of Ld at level l0, and where frac != 0, v = v0 + frac (v1 - v0) with v1 the lookup at
 *    l1; the mean m = m + (v - m) coef from m = 0.  K equal values give back that value exactly.  One thread owns one texel and walks the
 *    table in order: no partial sums are combined, no atomics.
 *    THE LOOKUP of a direction in a level of edge e: face, s, t as above; X = (s + 1) (e / 2) - 0.5, Y likewise with t; both clamped to [0, e - 1]
 *    (NaN gives 0); i0 = floor(X), i1 = min(i0 + 1, e - 1), ax = X - i0, the same along the rows; per channel t0 = c00 + ax (c10 - c00),
 *    t1 = c01 + ax (c11 - c01) (c10: column i1, row j0), then t0 + ay (t1 - t0).  Levels have no apron: taps CLAMP at the face's edge — a documented
 *    limit, seams between the faces of the rough levels are not stitched.
 * 4. SH9 of the irradiance, from mip level log2(E / Es) with Es = min(E, 64).  Texel t = (k Es + j) Es + i of that level: n = its normalised
 *    direction as in 3., (x, y, z) = (n.r, n.u, n.f); the real basis, each constant the double value rounded once: y0 = 0.28209479177387814,
 *    y1 = 0.4886025119029199 y, y2 = ... z, y3 = ... x, y4 = 1.0925484305920792 (x y), y5 = ... (y z), y6 = 0.31539156525252005 (3 (z z) - 1),
 *    y7 = 1.0925484305920792 (x z), y8 = 0.5462742152960396 (x x - y y); the texel's weight wy = y_b dw with dw the solid-angle table's entry
 *    [j][i], computed in double by the corner formula A(x1, y1) - A(x0, y1) - A(x1, y0) + A(x0, y0), A(x, y) = atan2(x y, sqrt(x x + y y + 1)),
 *    corners at 2 i / Es - 1, and rounded once; the term of channel c is v_c * wy.  Workgroup g sums the terms of texels 256 g ... 256 g + 255
 *    (absent ones count as +0) by the tree s[t] += s[t + h], h = 128, 64, ... 1; the partials are added in ascending g, ((p0 + p1) + p2) + ...;
 *    the sum of band l is multiplied by the cosine lobe's factor fl32(pi), fl32(2 pi / 3), fl32(pi / 4).  Output [c][b]: 9 of R, 9 of G, 9 of B.
 * 5. THE FILE: "DDS " + DDS_HEADER (124 bytes) + DDS_HEADER_DXT10 (20 bytes) = 148 bytes written by the host, then the payload, packed on the GPU in
 *    file order: face-major, each face followed by its L levels, rows top first, texels R G B A with A = 1.  DXGI format 10
 *    (R16G16B16A16_FLOAT; the conversion is digital_earth_exr.h's HALF: NaN to 0, clamped to 65504, nearest even) or 2 (R32G32B32A32_FLOAT).
 *    Header fields: flags 0x0002100F, height = width = E, pitch = E bytes-per-texel, mipMapCount = L, pixel format FOURCC "DX10", caps 0x00401008,
 *    caps2 0x0000FE00; DXT10: dimension 3 (TEXTURE2D), miscFlag 4 (TEXTURECUBE), arraySize 1.
 */
#ifndef DIGITAL_EARTH_IBL_H
#define DIGITAL_EARTH_IBL_H
#include "digital_earth_environment.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DE_IBL_SH_FLOATS 27
#define DE_IBL_DDS_HEADER 148
#define DE_IBL_MAX_PAYLOAD (1u << 27)

typedef struct de_ibl {
    uint32_t struct_bytes;               /* sizeof(de_ibl) of the caller */
    int32_t edge;                        /* E: a power of two, 8 ... 1024; default 128 */
    int32_t levels;                      /* L: 2 ... log2(E) + 1; level l has edge E >> l and roughness l / (L - 1); default 6 */
    int32_t samples;                     /* K per texel: a power of two, 8 ... 1024; default 256 */
    int32_t supersample;                 /* S of the base level: 1 ... 4; default 2 */
    float lod_bias;                      /* added to a sample's level of detail before the clamp; finite; default 0 */
    int32_t pixel_type;                  /* of the DDS file: DE_EXR_PIXEL_HALF (default) or DE_EXR_PIXEL_FLOAT */
} de_ibl;

/* Set the bake's settings.  DE_ERR_INVALID: a mismatched struct_bytes, a field outside the table above, or a payload beyond DE_IBL_MAX_PAYLOAD bytes
 * (with E <= 1024 the largest payload, E = 1024, L = 11, float, is 32 bytes short of it: the check is kept for the day the range grows).  A call that
 * succeeds drops what an earlier de_ibl_build made.  A refused call changes nothing.  Nothing is allocated here. */
int de_set_ibl(de_ctx* ctx, const de_ibl* settings);
/* The current settings (before any de_set_ibl: the defaults above). */
int de_get_ibl(de_ctx* ctx, de_ibl* out);
/* Run the bake on the six linear slots as they stand, into buffers of the context's own (allocated by the first call that succeeds).  DE_ERR_STATE
 * unless the panorama stage is on and all six linear slots are held (de_environment_capture).  The panorama's settings are read for the slots'
 * geometry alone (apron, basis); its projection and size play no part.  A refused call changes nothing. */
int de_ibl_build(de_ctx* ctx);
/* The nine coefficients of R, then of G, then of B.  DE_ERR_STATE before a de_ibl_build under the current settings. */
int de_fetch_ibl_sh(de_ctx* ctx, float* out27);
/* Face `face` of specular level `level` (0: the base level) as (e, e, 3) float32, e = E >> level, rows top first.  DE_ERR_INVALID for a level
 * outside 0 ... L - 1 or a face outside 0 ... 5; DE_ERR_STATE before a build. */
int de_fetch_ibl_face(de_ctx* ctx, int level, int face, float* out);
/* The DDS file's length under the current settings: 148 + the payload.  No build is needed. */
int de_ibl_file_bytes(de_ctx* ctx, uint64_t* bytes);
/* The whole file into `out` (out_bytes of room, at least de_ibl_file_bytes: DE_ERR_INVALID otherwise).  DE_ERR_STATE before a build. */
int de_fetch_ibl_dds(de_ctx* ctx, void* out, uint64_t out_bytes);
/* The bake once on six host-given linear faces, faces[6][n][n][3] as de_debug_environment_exr takes them (n in 4 ... 16384), with `panorama` as
 * de_set_panorama takes it (apron and basis are read; projection, size, supersample and `on` are checked and not used) and `ibl` as de_set_ibl.
 * Each output may be NULL: sh[27]; levels: every level's six faces, level-major ([L] blocks of [6][e][e][3]); dds with dds_bytes of room.  Buffers
 * and tables of its own; the context's settings, slots and product are untouched.  Every argument and setting refusal answers before the
 * context is read. */
int de_debug_ibl(de_ctx* ctx, const float* faces, int n, const de_panorama* panorama, const de_ibl* ibl, float* sh, float* levels, void* dds, uint64_t dds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DIGITAL_EARTH_IBL_H */

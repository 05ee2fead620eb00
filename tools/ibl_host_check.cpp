// ibl_host_check.cpp — the IBL bake's bodies (csrc/ibl_body.h, csrc/ibl_tables.h; include/digital_earth_ibl.h) replayed on the CPU, thread
// by thread in the kernels' own launch shapes, on heap blocks of EXACTLY the sizes the library allocates, so that the address sanitizer sees any tap,
// table entry or store outside its buffer and the undefined-behaviour sanitizer any bad shift, cast or index.  A stand-alone program, no GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ibl_host_check.cpp -o ibl_host_check && ./ibl_host_check
// It also checks what needs no device: a constant environment survives every stage exactly, the file's front, the settings' refusals.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_DEV static inline
static inline void host_sincos(float x, float* s, float* c) { *s = sinf(x); *c = cosf(x); }
#define PANO_SINCOS(x, s, c) host_sincos((x), (s), (c))
#define PANO_SQRT(x) sqrtf(x)
#define PANO_FLOOR(x) floorf(x)
#include "../digital_earth_amd/csrc/ibl_body.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Heap {      // one exact-size block per buffer: anything beyond it is the sanitizer's
    float* p; size_t n;
    explicit Heap(size_t floats) : p((float*)malloc((floats ? floats : 1) * sizeof(float))), n(floats) { for (size_t k = 0; k < n; ++k) p[k] = NAN; }
    ~Heap() { free(p); }
};

// every thread of a launch over a level of edge e: the kernels' block and tile decode
template <class Body>
static void for_each_thread(int e, Body body) {
    const int tiles = (e + IBL_TILE - 1) / IBL_TILE;
    for (int block = 0; block < 6 * tiles * tiles; ++block)
        for (int t = 0; t < IBL_THREADS; ++t) {
            int il, jl;
            ibl_tile_texel(t, &il, &jl);
            const int b = block % (tiles * tiles), face = block / (tiles * tiles), i = (b % tiles) * IBL_TILE + il, j = (b / tiles) * IBL_TILE + jl;
            if (i < e && j < e) body(face, i, j);
        }
}

static void bake(int N, int apron, int E, int L, int K, int S, float lod_bias, int pixel_type, float constant, bool is_constant) {
    const int M = ibl_log2(E) + 1;
    Heap faces((size_t)6 * N * N * 3), mips(ibl_level_offset(E, M)), spec(ibl_level_offset(E, L) - ibl_level_offset(E, 1));
    uint32_t seed = 12345u + (uint32_t)E;
    for (size_t k = 0; k < faces.n; ++k) { seed = seed * 1664525u + 1013904223u; faces.p[k] = is_constant ? constant : (float)(seed >> 8) * (1e4f / 16777216.0f); }
    if (!is_constant) faces.p[((size_t)(4 * N + N / 2 + 1) * N + N / 3) * 3] = 1e7f;      // a sun
    PanoArgs p;
    memset(&p, 0, sizeof p);
    p.faces = faces.p; p.N = N; p.S = S;
    p.fov = (float)((double)N / (double)(N - 2 * apron)); p.scale = (float)((double)N / (2.0 * (double)p.fov));
    for (int face = 0; face < 6; ++face) {      // digital_earth_panorama.h's m of the identity basis: du = look x up, dv = du x look
        static const int look_of[6] = {0, 0, 1, 1, 2, 2}, up_of[6] = {1, 1, 2, 2, 1, 1};
        static const double look_sign[6] = {1, -1, 1, -1, 1, -1}, up_sign[6] = {1, 1, -1, 1, 1, 1};
        double d[3] = {0, 0, 0}, up[3] = {0, 0, 0};
        d[look_of[face]] = look_sign[face]; up[up_of[face]] = up_sign[face];
        const double du[3] = {d[1] * up[2] - d[2] * up[1], d[2] * up[0] - d[0] * up[2], d[0] * up[1] - d[1] * up[0]};
        const double dv[3] = {du[1] * d[2] - du[2] * d[1], du[2] * d[0] - du[0] * d[2], du[0] * d[1] - du[1] * d[0]};
        const int axis = face / 2, e1 = axis == 0 ? 1 : 0, e2 = axis == 2 ? 1 : 2;
        p.m[face][0] = (float)du[e1]; p.m[face][1] = (float)du[e2]; p.m[face][2] = (float)dv[e1]; p.m[face][3] = (float)dv[e2];
    }
    for_each_thread(E, [&](int face, int i, int j) { ibl_base_texel(p, mips.p, E, S, face, i, j); });
    for (int m = 1; m < M; ++m)
        for_each_thread(E >> m, [&](int face, int i, int j) { ibl_mip_texel(mips.p + ibl_level_offset(E, m - 1), mips.p + ibl_level_offset(E, m), E >> m, face, i, j); });
    IblLevelArgs a;
    memset(&a, 0, sizeof a);
    a.mips = mips.p; a.E = E; a.M = M;
    for (int m = 0; m < M; ++m) a.off[m] = (uint32_t)ibl_level_offset(E, m);
    int kept_all = 0;
    for (int l = 1; l < L; ++l) {
        std::vector<IblSample> tab;
        ibl_build_samples(E, L, K, l, lod_bias, &tab);
        CHECK(!tab.empty() && tab[0].coef == 1.0f, "level %d: the first kept sample's coefficient is not 1", l);
        for (const IblSample& s : tab) CHECK(s.l0 >= 0 && s.l0 <= s.l1 && s.l1 <= M - 1 && s.frac >= 0.0f && s.frac < 1.0f && s.coef > 0.0f && s.coef <= 1.0f, "level %d: a sample outside its ranges", l);
        IblSample* exact = (IblSample*)malloc(tab.size() * sizeof(IblSample));      // exactly the kept samples
        memcpy(exact, tab.data(), tab.size() * sizeof(IblSample));
        a.tab = exact; a.n = (int)tab.size(); a.e = E >> l; a.out = spec.p + (ibl_level_offset(E, l) - ibl_level_offset(E, 1));
        for_each_thread(a.e, [&](int face, int i, int j) { ibl_spec_texel(a, face, i, j); });
        free(exact);
        kept_all += a.n;
    }
    for (size_t k = 0; k < mips.n; ++k) CHECK(is_constant ? mips.p[k] == constant : isfinite(mips.p[k]), "mip chain float %zu", k);
    for (size_t k = 0; k < spec.n; ++k) CHECK(is_constant ? spec.p[k] == constant : isfinite(spec.p[k]), "specular float %zu", k);
    // SH: the workgroups' trees and the ordered sum
    const int es = E < IBL_SH_EDGE ? E : IBL_SH_EDGE, groups = (6 * es * es + IBL_THREADS - 1) / IBL_THREADS;
    std::vector<float> omega;
    ibl_build_omega(es, &omega);
    Heap om(omega.size()), partial((size_t)groups * 27);
    memcpy(om.p, omega.data(), omega.size() * sizeof(float));
    double sphere = 0.0;
    for (float w : omega) sphere += 6.0 * (double)w;
    CHECK(fabs(sphere - 4.0 * 3.14159265358979323846) <= 4.0 * 3.14159265358979323846 * ldexp(1.0, -24), "the solid angles sum to %.9f", sphere);
    const float* level = mips.p + ibl_level_offset(E, ibl_log2(E / es));
    for (int g = 0; g < groups; ++g) {
        std::vector<float> s((size_t)27 * IBL_THREADS, 0.0f);
        for (int t = 0; t < IBL_THREADS; ++t) {
            float terms[27];
            const int texel = g * IBL_THREADS + t;
            if (texel < 6 * es * es) ibl_sh_terms(level, om.p, es, texel, terms); else for (float& v : terms) v = 0.0f;
            for (int k = 0; k < 27; ++k) s[(size_t)k * IBL_THREADS + t] = terms[k];
        }
        for (int h = IBL_THREADS / 2; h > 0; h >>= 1)
            for (int t = 0; t < h; ++t) for (int k = 0; k < 27; ++k) s[(size_t)k * IBL_THREADS + t] += s[(size_t)k * IBL_THREADS + t + h];
        for (int k = 0; k < 27; ++k) partial.p[(size_t)g * 27 + k] = s[(size_t)k * IBL_THREADS];
    }
    float sh[27];
    for (int k = 0; k < 27; ++k) {
        float acc = partial.p[k];
        for (int g = 1; g < groups; ++g) acc = acc + partial.p[(size_t)g * 27 + k];
        sh[k] = acc * ibl_sh_band_factor(k % 9);
    }
    if (is_constant) {
        const double want = (double)constant * 2.0 * sqrt(3.14159265358979323846) * 3.14159265358979323846;
        for (int c = 0; c < 3; ++c) CHECK(fabs((double)sh[c * 9] - want) <= 32.0 * ldexp(1.0, -24) * fabs(want), "band 0 of a constant: %.9g, want %.9g", (double)sh[c * 9], want);
    }
    // the file
    const size_t payload = ibl_payload_bytes(E, L, pixel_type);
    uint8_t* file = (uint8_t*)malloc(payload);
    IblPackArgs q;
    memset(&q, 0, sizeof q);
    q.mips = mips.p; q.spec = spec.p; q.out = file; q.E = E; q.L = L; q.half = pixel_type == IBL_PIXEL_HALF; q.texels_per_face = (uint32_t)ibl_texels_before(E, L);
    for (int l = 1; l < L; ++l) q.spec_off[l] = (uint32_t)(ibl_level_offset(E, l) - ibl_level_offset(E, 1));
    const uint32_t blocks = (6u * q.texels_per_face + IBL_THREADS - 1) / IBL_THREADS;
    for (uint32_t idx = 0; idx < blocks * IBL_THREADS; ++idx) if (idx < 6u * q.texels_per_face) ibl_pack_texel(q, idx);
    if (is_constant && pixel_type == IBL_PIXEL_HALF) {
        const uint16_t want = (uint16_t)exr_half_bits(exr_sample_bits(constant, 1.0f));
        for (size_t k = 0; k < payload / 2; ++k) { uint16_t v; memcpy(&v, file + 2 * k, 2); CHECK(v == ((k & 3) == 3 ? 0x3c00 : want), "half %zu of the payload", k); }
    }
    free(file);
    printf("bake N=%d apron=%d E=%d L=%d K=%d S=%d bias=%g %s: %d kept samples, %zu payload bytes\n", N, apron, E, L, K, S, (double)lod_bias, pixel_type == IBL_PIXEL_HALF ? "half" : "float", kept_all, payload);
}

int main() {
    bake(16, 1, 16, 5, 8, 1, 0.0f, IBL_PIXEL_HALF, 0.0f, false);
    bake(16, 4, 64, 4, 16, 3, 0.0f, IBL_PIXEL_FLOAT, 0.0f, false);
    bake(16, 1, 32, 6, 64, 2, 0.0f, IBL_PIXEL_HALF, 0.0f, false);
    bake(16, 1, 32, 6, 8, 1, -100.0f, IBL_PIXEL_HALF, 0.0f, false);      // every sample reads level 0
    bake(16, 1, 8, 4, 8, 4, 100.0f, IBL_PIXEL_FLOAT, 0.0f, false);       // every sample reads the last level
    for (float c : {0.0f, 0.3f, 70000.0f}) for (int S : {1, 3, 4}) bake(16, 1, 16, 5, 8, S, 0.0f, IBL_PIXEL_HALF, c, true);
    CHECK(exr_half_bits(exr_sample_bits(70000.0f, 1.0f)) == 0x7bffu, "half of 70000");
    // the settings
    CHECK(ibl_settings_fault(128, 6, 256, 2, 0.0f, 1) == nullptr && ibl_settings_fault(1024, 11, 1024, 4, -3.0f, 2) == nullptr && ibl_settings_fault(8, 4, 8, 1, 0.0f, 1) == nullptr, "good settings refused");
    CHECK(ibl_settings_fault(4, 2, 8, 1, 0.0f, 1) && ibl_settings_fault(2048, 2, 8, 1, 0.0f, 1) && ibl_settings_fault(24, 2, 8, 1, 0.0f, 1), "a bad edge accepted");
    CHECK(ibl_settings_fault(8, 1, 8, 1, 0.0f, 1) && ibl_settings_fault(8, 5, 8, 1, 0.0f, 1), "bad levels accepted");
    CHECK(ibl_settings_fault(8, 2, 4, 1, 0.0f, 1) && ibl_settings_fault(8, 2, 2048, 1, 0.0f, 1) && ibl_settings_fault(8, 2, 12, 1, 0.0f, 1), "bad samples accepted");
    CHECK(ibl_settings_fault(8, 2, 8, 0, 0.0f, 1) && ibl_settings_fault(8, 2, 8, 5, 0.0f, 1) && ibl_settings_fault(8, 2, 8, 1, NAN, 1) && ibl_settings_fault(8, 2, 8, 1, INFINITY, 1), "a bad supersample or bias accepted");
    CHECK(ibl_settings_fault(8, 2, 8, 1, 0.0f, 0) && ibl_settings_fault(8, 2, 8, 1, 0.0f, 3), "a bad pixel type accepted");
    CHECK(ibl_payload_bytes(1024, 11, IBL_PIXEL_FLOAT) == 134217696u && ibl_payload_bytes(1024, 11, IBL_PIXEL_FLOAT) <= IBL_MAX_PAYLOAD, "the largest payload");
    // the front
    uint8_t* front = (uint8_t*)malloc(IBL_DDS_HEADER);
    ibl_dds_header(256, 6, IBL_PIXEL_HALF, front);
    uint32_t w[37];
    memcpy(w, front, sizeof w);
    CHECK(memcmp(front, "DDS ", 4) == 0 && w[1] == 124 && w[3] == 256 && w[4] == 256 && w[5] == 2048 && w[7] == 6 && memcmp(front + 84, "DX10", 4) == 0 && w[32] == 10 && w[33] == 3 && w[34] == 4 && w[35] == 1, "the DDS front");
    free(front);
    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("ibl bodies: every thread replayed, no sanitizer report\n");
    return 0;
}

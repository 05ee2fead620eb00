// look_host_check.cpp — look_apply_kernel's own source (csrc/look_kernels.hip) compiled for the HOST, so that the address and undefined-behaviour
// sanitizers can watch every index it forms.  The kernel is one pointwise step: this program runs lk_thread for every thread of every
// workgroup of the launch (the idle threads of the last workgroup included) over a heap image of exactly n x 3 floats and heap tables of exactly
// their sizes: one index past either end of any of them is the sanitizer's to find.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off tools/look_host_check.cpp -o look_host_check
//   look_host_check            n in {1, 3, 4, 5, 255, 256, 257, 1023, 4100, 48 x 24}; 3D edges 2, 3, 17, 33, 65 and 1D sizes 2, 1024, 65536, alone and
//                              chained; both interpolations; strengths 0, 0.37, 1; a default and a non-default domain; on pixels of its own with the
//                              special values among them.  Every output must lie in [0, 1], and strength 0 must give back every pixel of [0, 1].
//   look_host_check IN OUT     one conversion.  IN: uint64 n; int32 size_1d, size_3d, interpolation; float strength, min_1d[3], max_1d[3], min_3d[3],
//                              max_3d[3]; then the 1D table, the 3D table (size^3 x 3, red fastest) and n x 3 pixels, all f32.  OUT: n x 3 f32.
//                              (tests/look_ref.py's apply() gives the same bytes.)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_LOOK_STANDALONE
#define DE_DEV static inline
struct alignas(16) float4 { float x, y, z, w; };
#include "../digital_earth_amd/csrc/look_kernels.hip"

// `bytes` on the heap, 16-byte aligned as hipMalloc's memory is (the float4 views need it), and not one byte more: the sanitizer sees the exact end.
static void* exact16(size_t bytes) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) { fprintf(stderr, "no memory\n"); exit(2); }
    return p;
}

struct Look {
    int n1 = 0, n3 = 0, tetrahedral = 1;
    float strength = 1.0f;
    float lo1[3] = {0, 0, 0}, hi1[3] = {1, 1, 1}, lo3[3] = {0, 0, 0}, hi3[3] = {1, 1, 1};
    std::vector<float> t1, t3;      // as the caller gives them: [n1][3], [n3^3][3]
};

// The launch over `px` in place, as lk_upload and lk_launch (de_display.h) set it up.  
static void run(const Look& L, float* px, uint64_t n) {
    const size_t cells = (size_t)L.n3 * L.n3 * L.n3;
    float4* wide = cells ? (float4*)exact16(cells * sizeof(float4)) : nullptr;
    for (size_t i = 0; i < cells; ++i) { wide[i].x = L.t3[3 * i]; wide[i].y = L.t3[3 * i + 1]; wide[i].z = L.t3[3 * i + 2]; wide[i].w = 0.0f; }
    std::vector<float> t1 = L.t1;
    LookArgs a;
    a.image = px; a.n = n; a.t1 = L.n1 ? t1.data() : nullptr; a.t3 = wide; a.n1 = L.n1; a.n3 = L.n3; a.tetrahedral = L.tetrahedral; a.strength = L.strength;
    for (int c = 0; c < 3; ++c) {
        a.a1[c].lo = L.lo1[c]; a.a1[c].k = L.n1 ? lk_scale(L.n1, L.lo1[c], L.hi1[c]) : 0.0f;
        a.a3[c].lo = L.lo3[c]; a.a3[c].k = L.n3 ? lk_scale(L.n3, L.lo3[c], L.hi3[c]) : 0.0f;
    }
    const uint64_t blocks = (lk_threads(n) + 255u) / 256u;
    for (uint64_t j = 0; j < blocks * 256u; ++j) lk_thread(a, j);
    free(wide);
}

static uint32_t g_seed = 12345u;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) * (1.0f / 16777216.0f); }

static std::vector<float> noise_table(size_t rows) {
    std::vector<float> t(rows * 3);
    for (float& v : t) v = rnd() * 1.5f - 0.25f;
    return t;
}

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc == 3) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        const uint64_t n = take<uint64_t>(f, 1)[0];
        const std::vector<int32_t> head = take<int32_t>(f, 3);
        const std::vector<float> fl = take<float>(f, 13);
        Look L;
        L.n1 = head[0]; L.n3 = head[1]; L.tetrahedral = head[2]; L.strength = fl[0];
        if (n == 0 || n > (1u << 28) || L.n1 < 0 || L.n1 == 1 || L.n1 > 65536 || L.n3 < 0 || L.n3 == 1 || L.n3 > 65 || (!L.n1 && !L.n3)) return 2;
        for (int c = 0; c < 3; ++c) { L.lo1[c] = fl[1 + c]; L.hi1[c] = fl[4 + c]; L.lo3[c] = fl[7 + c]; L.hi3[c] = fl[10 + c]; }
        L.t1 = take<float>(f, (size_t)L.n1 * 3);
        L.t3 = take<float>(f, (size_t)L.n3 * L.n3 * L.n3 * 3);
        const std::vector<float> in = take<float>(f, (size_t)n * 3);
        fclose(f);
        float* px = (float*)exact16((size_t)n * 12);
        memcpy(px, in.data(), (size_t)n * 12);
        run(L, px, n);
        f = fopen(argv[2], "wb");
        if (!f) return 2;
        fwrite(px, 12, (size_t)n, f);
        fclose(f);
        free(px);
        return 0;
    }
    if (argc != 1) return 2;
    static const uint64_t counts[] = {1, 3, 4, 5, 255, 256, 257, 1023, 4100, 48 * 24};
    static const int edges[][2] = {{0, 2}, {0, 3}, {0, 17}, {0, 33}, {0, 65}, {2, 0}, {1024, 0}, {65536, 0}, {2, 65}, {65536, 2}, {1024, 17}};      // {1D, 3D}
    static const float strengths[] = {0.0f, 0.37f, 1.0f};
    const float special[] = {-0.0f, NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e-45f, 1.0f, 0.0f, 0.99999994f, -1e-45f, 2.0f};
    int runs = 0;
    for (const auto& e : edges) {
        Look L;
        L.n1 = e[0]; L.n3 = e[1];
        L.t1 = noise_table((size_t)L.n1);
        L.t3 = noise_table((size_t)L.n3 * L.n3 * L.n3);
        for (int domain = 0; domain < 2; ++domain) {
            for (int c = 0; c < 3; ++c) {
                L.lo1[c] = domain ? -0.25f + 0.1f * c : 0.0f; L.hi1[c] = domain ? 1.5f - 0.2f * c : 1.0f;
                L.lo3[c] = domain ? 0.1f * c : 0.0f; L.hi3[c] = domain ? 0.9f + 0.3f * c : 1.0f;
            }
            for (int tetra = 0; tetra < 2; ++tetra)
                for (float s : strengths)
                    for (uint64_t n : counts) {
                        std::vector<float> in((size_t)n * 3);
                        for (float& v : in) v = rnd() * 1.4f - 0.2f;
                        for (size_t i = 0; i < sizeof(special) / sizeof(special[0]) && 2 * i + 1 < in.size(); ++i) in[2 * i + 1] = special[i];
                        float* buf = (float*)exact16((size_t)n * 12);      // exactly n x 3 floats
                        memcpy(buf, in.data(), (size_t)n * 12);
                        L.tetrahedral = tetra; L.strength = s;
                        run(L, buf, n);
                        for (size_t i = 0; i < in.size(); ++i) {
                            const float o = buf[i];
                            if (!(o >= 0.0f && o <= 1.0f)) { fprintf(stderr, "1D %d 3D %d n %llu: output %g outside [0, 1]\n", L.n1, L.n3, (unsigned long long)n, o); return 1; }
                            if (s == 0.0f && in[i] >= 0.0f && in[i] <= 1.0f && memcmp(&o, &in[i], 4) != 0 && !(in[i] == 0.0f && o == 0.0f)) {
                                fprintf(stderr, "1D %d 3D %d n %llu: strength 0 changed %g to %g\n", L.n1, L.n3, (unsigned long long)n, in[i], o);
                                return 1;
                            }
                        }
                        free(buf);
                        ++runs;
                    }
        }
    }
    printf("look_host_check: %d launches, every output in [0, 1], strength 0 the identity, no sanitizer report\n", runs);
    return 0;
}

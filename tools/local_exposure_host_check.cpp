// local_exposure_host_check.cpp — the four kernels' own source (csrc/local_exposure_kernels.hip) and the project's de_log / de_pow (csrc/de_math.h)
// compiled for the HOST, so that the address and undefined-behaviour sanitizers can watch every index they form
// (tools/local_exposure_host_check.py builds and drives this, with tools/host_shim on the include path in place of the HIP runtime header;
// DESIGN.md §15).  Every kernel is its phases around its barriers: this program runs each phase for the 256 threads of a workgroup, then the next,
// one workgroup at a time.  The LDS tiles are heap blocks of exactly the kernels' LDS sizes filled with NaN (a read of a word that was never staged
// would show in the output), and every level is a heap block of exactly its size.  The plan of the levels, the staging of a level and the row and
// column passes are the shared pyramid's (csrc/pyramid.h): this program exercises the passes that the bloom runs too.
//   local_exposure_host_check run IN OUT     IN: int32 W, H, levels, vec; f32 exposure_scale, highlights, shadows, sigma, max_ev, key; then the mean
//                                            [H][W][3] f32.  OUT: the dodged mean [H][W][3] f32.
//   local_exposure_host_check log IN OUT     IN: f32 values.  OUT: de_log of each — what the Python side injects into the restatement ...
//   local_exposure_host_check pow2 IN OUT    ... and de_pow(2, each).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits>
#include <vector>

#include "../digital_earth_amd/csrc/de_math.h"
struct FrameConsts { float exposure_scale; };      // the one field the stage reads
#define DE_LX_STANDALONE
#include "../digital_earth_amd/csrc/local_exposure_kernels.hip"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);      // exactly n elements on the heap: one index past either end is the sanitizer's to find
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
static std::vector<float> take_all(FILE* f) {
    std::vector<float> v;
    float x;
    while (fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
    return v;
}

template <int STRIDE>
struct Tiles {      // one workgroup's LDS
    std::vector<float> src, hb;
    Tiles() : src((size_t)2 * 34 * STRIDE, std::numeric_limits<float>::quiet_NaN()), hb((size_t)2 * 34 * PYR_H_STRIDE, std::numeric_limits<float>::quiet_NaN()) {}
    float (*s())[34][STRIDE] { return reinterpret_cast<float (*)[34][STRIDE]>(src.data()); }
    float (*h())[34][PYR_H_STRIDE] { return reinterpret_cast<float (*)[34][PYR_H_STRIDE]>(hb.data()); }
};

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<float> result;
    if (!strcmp(argv[1], "log") || !strcmp(argv[1], "pow2")) {
        result = take_all(f);
        const bool is_log = argv[1][0] == 'l';
        for (float& x : result) x = is_log ? de_log(x) : de_pow(2.0f, x);
    } else {
        const std::vector<int32_t> head = take<int32_t>(f, 4);
        const std::vector<float> set = take<float>(f, 6);
        const int W = head[0], H = head[1], levels = head[2];
        const bool vec = head[3] != 0;
        const std::vector<float> mean = take<float>(f, (size_t)W * H * 3);
        const PyramidPlan plan = pyr_plan(W, H, levels);      // the host side's own (csrc/pyramid.h)
        const int* w = plan.w;
        const int* h = plan.h;
        const int L = plan.L;
        std::vector<std::vector<float2>> D(L + 1);
        std::vector<std::vector<float>> B(L + 1);
        for (int l = 1; l <= L; ++l) { D[l].resize((size_t)w[l] * h[l]); if (l < L) B[l].resize((size_t)w[l] * h[l]); }
        const FrameConsts fc = {set[0]};
        DisplaySrc s;
        s.hdr = mean.data(); s.tile_spp = nullptr; s.samples = 1; s.W = W; s.H = H;
        for (int by = 0; by < (h[1] + 15) / 16; ++by)
            for (int bx = 0; bx < (w[1] + 15) / 16; ++bx) {
                Tiles<PYR_SRC_STRIDE> lds;
                for (int t = 0; t < 256; ++t) { if (vec) lx_stage0<true>(s, lds.s(), t, bx, by); else lx_stage0<false>(s, lds.s(), t, bx, by); }
                for (int t = 0; t < 256; ++t) pyr_row_pass<2, PYR_SRC_STRIDE>(lds.s(), lds.h(), t, bx, by, bx * 32 - 4, W, H, w[1]);
                for (int t = 0; t < 256; ++t) pyr_col_pass<2>(lds.h(), t, bx, by, H, w[1], h[1], D[1].data());
            }
        for (int l = 1; l < L; ++l)
            for (int by = 0; by < (h[l + 1] + 15) / 16; ++by)
                for (int bx = 0; bx < (w[l + 1] + 15) / 16; ++bx) {
                    Tiles<PYR_LVL_STRIDE> lds;
                    for (int t = 0; t < 256; ++t) pyr_stage_level<2>(D[l].data(), w[l], h[l], lds.s(), t, bx, by);
                    for (int t = 0; t < 256; ++t) pyr_row_pass<2, PYR_LVL_STRIDE>(lds.s(), lds.h(), t, bx, by, bx * 32 - 1, w[l], h[l], w[l + 1]);
                    for (int t = 0; t < 256; ++t) pyr_col_pass<2>(lds.h(), t, bx, by, h[l], w[l + 1], h[l + 1], D[l + 1].data());
                }
        const float inv_sigma = 1.0f / set[3];
        const float* top = nullptr;
        for (int l = L - 1; l >= 1; --l) {
            LxUpArgs u;
            u.fine = D[l].data(); u.coarse = D[l + 1].data(); u.coarse_b = top; u.out = B[l].data();
            u.Wc = w[l + 1]; u.Hc = h[l + 1]; u.Wf = w[l]; u.Hf = h[l]; u.inv_sigma = inv_sigma;
            const uint32_t n_wg = (uint32_t)(((size_t)u.Wf * u.Hf + 255) / 256);
            for (uint32_t item = 0; item < n_wg * 256u; ++item) lx_up_item(u, item);
            top = u.out;
        }
        result.assign((size_t)W * H * 3, std::numeric_limits<float>::quiet_NaN());
        LxApplyArgs a;
        a.s = s; a.d1 = D[1].data(); a.b1 = top; a.W1 = w[1]; a.H1 = h[1]; a.fc = &fc;
        a.highlights = set[1]; a.shadows = set[2]; a.inv_sigma = inv_sigma; a.max_ev = set[4]; a.key = set[5]; a.out = result.data();
        const uint32_t n_wg = (uint32_t)(((size_t)(W >> 2) * H + 255) / 256);
        for (uint32_t item = 0; item < n_wg * 256u; ++item) { if (vec) lx_apply_item<true>(a, item); else lx_apply_item<false>(a, item); }
    }
    fclose(f);
    f = fopen(argv[3], "wb");
    if (!f) return 2;
    fwrite(result.data(), sizeof(float), result.size(), f);
    fclose(f);
    return 0;
}

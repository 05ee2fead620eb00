// output_scale_kernels.hip — the opt-in output scaling behind the display transform and ahead of the 8-bit pack (include/digital_earth_output_scale.h,
// DESIGN.md §16): the displayed image, (W, H, 3) f32 with the pixels of a COLUMN contiguous (index (u H + v) 3 + c), is resampled to (ow, oh, 3) by a
// separable polyphase filter in two passes with an f32 intermediate, along v first, then along u.  The header carries the definition; the table
// builder below (host code, double precision) and the two kernels follow it, and so does tests/output_scale_ref.py, bit for bit.
//   os_build_table       one axis' table on the host: first[j] (unclamped) and w[tap][j] — [tap][j], not [j][tap], so that neighbouring lanes of the
//                        pass along v read neighbouring words — padded to one tap count, every row corrected to the exact-one property.
//   output_scale_v_kernel  the pass along v, inside the contiguous columns.  One 192-thread workgroup = one column x 64 output samples x 3 channels,
//                        thread t = output element (j0 + t / 3, t % 3).  Neighbouring outputs read source runs that overlap and are strided by r, so
//                        the source segment of the tile — clamp(first[j0]) ... clamp(first[j1] + taps - 1), at most 63 * 8 + 1 + 49 = 554 pixels
//                        because first[j + k] - first[j] <= k r + 1 and r <= 8 — is staged in LDS with coalesced loads (a wave reads 256 contiguous
//                        bytes per instruction) and filtered from there.  The segment is one row of 3 n words; lane t reads word
//                        3 (first + tap - lo) + c, a stride of 3 r words between pixels.  Derived for ds_read_b32 (32 banks, 32-lane groups, a
//                        group = 10 2/3 pixels): unpadded, r = 8 is a stride of 24 words with period 4 pixels — pixels k, k + 4 and k + 8 of a group
//                        share banks, 3-way; r = 4 (stride 12, period 8) is 2-way.  Skewing the row by one word per 32 (word i at i + i / 32, the
//                        padding pixels_kernels.hip gives each of its rows, here applied inside the one long row) breaks the period: at r = 8 the
//                        eleven pixels of a group start at banks 0 24 17 10 3 27 20 13 6 30 23, at worst two on a bank.  Other ratios are at worst
//                        2-way either way; nothing more is spent on a pass of a few microseconds.
//   output_scale_u_kernel  the pass along u, across columns.  One 256-thread workgroup = 256 consecutive floats of one output column: every tap is
//                        one fully coalesced load of the same 256 floats of a source column (a wave reads 256 contiguous bytes), `first` and the
//                        weights depend on the workgroup alone (wave-uniform: scalar loads), no LDS.
// Both kernels: acc = 0.0f; acc = acc + w[t] * src[t] in ascending tap order, the zero padding included (a multiply then an add: -ffp-contract=off);
// source indices are clamped to the axis when gathered; the last pass clamps its result to [0, 1] with the packs' clamp (pack.h).  An axis of equal size
// runs no pass.  One-dimensional grids (a dimension of 65 535 blocks would not hold a 4K column count times its tiles).  No atomics, no scratch; every
// index is range-checked, or clamped into a range derived above, before its load or store.
// Included into de_api.hip's translation unit after pixels_kernels.hip; display_kernel and pixels_pack_kernel are untouched.
#ifndef DE_OUTPUT_SCALE_STANDALONE      // a host build of this file alone brings its own DE_DEV (tools/output_scale_host_check.cpp)
#include "de_kernels.h"
#endif
#include <math.h>
#include <stdint.h>
#include <vector>
#include "pack.h"      // pack_clamp01 alone

#define OS_MAX_TAPS 49            // 2 ceil(3 * 8) + 1: Lanczos-3 shrinking by 8
#define OS_V_TILE 64              // output samples of a column per workgroup of the pass along v
#define OS_V_THREADS 192          // OS_V_TILE x 3 channels
#define OS_V_SEG_PIXELS 560       // >= (OS_V_TILE - 1) * 8 + 1 + OS_MAX_TAPS = 554
#define OS_V_LDS_WORDS 1736       // >= skew(3 * 560 - 1) + 1 = 1679 + 52 + 1 = 1732
#define OS_U_THREADS 256

struct ScaleTable {               // one axis, on the host
    int n_src = 0, n_dst = 0, filter = -1, taps = 0;
    std::vector<int32_t> first;   // [n_dst], unclamped
    std::vector<float> w;         // [taps][n_dst]
};

struct ScaleArgs {                // one pass
    const float* src;             // pass v: (lines, n_src, 3); pass u: (n_src, lines)
    float* dst;                   // pass v: (lines, n_dst, 3); pass u: (n_dst, lines)
    const int32_t* first;         // [n_dst]
    const float* w;               // [taps][n_dst]
    int n_src, n_dst, taps;
    int lines;                    // pass v: the columns; pass u: the floats of a column (rows x 3)
    int clamp;                    // this is the last pass: clamp to [0, 1]
};

inline double os_support(int filter) { return filter == 0 ? 0.5 : filter == 1 ? 1.0 : filter == 2 ? 2.0 : 3.0; }

inline double os_sinc(double z) {
    if (z == 0.0) return 1.0;
    const double p = M_PI * z;
    return sin(p) / p;
}

inline double os_kernel(int filter, double t) {
    const double at = fabs(t);
    if (filter == 0) return 1.0;
    if (filter == 1) return at < 1.0 ? 1.0 - at : 0.0;
    if (filter == 2) {
        if (at < 1.0) return (7.0 * at * at * at - 12.0 * at * at + 16.0 / 3.0) / 6.0;
        if (at < 2.0) return (-7.0 / 3.0 * at * at * at + 12.0 * at * at - 20.0 * at + 32.0 / 3.0) / 6.0;
        return 0.0;
    }
    return at < 3.0 ? os_sinc(t) * os_sinc(t / 3.0) : 0.0;
}

// The table of one axis as the header defines it.  false: the arguments are out of range, or a property the kernels rely on does not hold (the
// exact-one sum, `first` ascending, a tile's segment within OS_V_SEG_PIXELS) — none of which the definition admits for n_dst / n_src in [1/8, 8].
inline bool os_build_table(int n_src, int n_dst, int filter, ScaleTable* T) {
    if (n_src <= 0 || n_dst <= 0 || filter < 0 || filter > 3 || (long long)n_dst * 8 < n_src || (long long)n_src * 8 < n_dst) return false;
    const double r = (double)n_src / (double)n_dst, s = r > 1.0 ? r : 1.0, R = os_support(filter) * s;
    std::vector<int32_t> lo((size_t)n_dst), cnt((size_t)n_dst);
    int taps = 0;
    for (int j = 0; j < n_dst; ++j) {
        const double x = ((double)j + 0.5) * r - 0.5;
        int a = (int)floor(x - R) + 1, b = (int)ceil(x + R) - 1;
        if (b < a) a = b = (int)floor(x + 0.5);
        lo[(size_t)j] = a; cnt[(size_t)j] = b - a + 1;
        if (b - a + 1 > taps) taps = b - a + 1;
    }
    if (taps < 1 || taps > OS_MAX_TAPS) return false;
    T->n_src = n_src; T->n_dst = n_dst; T->filter = filter; T->taps = taps;
    T->first.assign(lo.begin(), lo.end());
    T->w.assign((size_t)taps * (size_t)n_dst, 0.0f);
    double k[OS_MAX_TAPS];
    for (int j = 0; j < n_dst; ++j) {
        const double x = ((double)j + 0.5) * r - 0.5;
        const int n = cnt[(size_t)j];
        double sum = 0.0;
        for (int t = 0; t < n; ++t) { k[t] = os_kernel(filter, ((double)(lo[(size_t)j] + t) - x) / s); sum = sum + k[t]; }
        if (!(sum > 0.0)) return false;
        float P = 0.0f;
        for (int t = 0; t < n - 1; ++t) {
            const float wt = (float)(k[t] / sum);
            T->w[(size_t)t * (size_t)n_dst + (size_t)j] = wt;
            P = P + wt;
        }
        const float last = 1.0f - P;                       // the correction: the row's last tap takes what the float32 sum of the others leaves
        T->w[(size_t)(n - 1) * (size_t)n_dst + (size_t)j] = last;
        const float one = P + last;
        if (one != 1.0f) return false;
        if (j > 0 && lo[(size_t)j] < lo[(size_t)j - 1]) return false;
    }
    for (int j0 = 0; j0 < n_dst; j0 += OS_V_TILE) {        // what output_scale_v_kernel's LDS segment relies on
        const int j1 = j0 + OS_V_TILE - 1 < n_dst ? j0 + OS_V_TILE - 1 : n_dst - 1;
        if ((long long)lo[(size_t)j1] + taps - 1 - lo[(size_t)j0] + 1 > OS_V_SEG_PIXELS) return false;
    }
    return true;
}

DE_DEV int os_skew(int i) { return i + (i >> 5); }
DE_DEV int os_clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// The source segment of tile `tile` of a column: pixels lo ... lo + n - 1, every (clamped) tap of the tile's outputs among them because `first` ascends.
DE_DEV void os_v_segment(const ScaleArgs& a, int tile, int* lo, int* n) {
    const int j0 = tile * OS_V_TILE;
    const int j1 = j0 + OS_V_TILE - 1 < a.n_dst ? j0 + OS_V_TILE - 1 : a.n_dst - 1;
    const int l = os_clampi(a.first[j0], a.n_src), h = os_clampi(a.first[j1] + a.taps - 1, a.n_src);
    const int m = h - l + 1;
    *lo = l;
    *n = m < 1 ? 1 : (m > OS_V_SEG_PIXELS ? OS_V_SEG_PIXELS : m);      // 1 ... 554 by os_build_table; bounded here whatever the table holds
}

// Pass along v, first half: thread t of the workgroup of (column, tile) stages words t, t + 192, ... of the segment.
DE_DEV void os_v_stage(const ScaleArgs& a, float* lds, int t, int column, int tile) {
    int lo, n;
    os_v_segment(a, tile, &lo, &n);
    const float* s = a.src + ((size_t)column * (size_t)a.n_src + (size_t)lo) * 3;      // lo + n <= n_src
    for (int i = t; i < n * 3; i += OS_V_THREADS) lds[os_skew(i)] = s[i];
}

// Second half: thread t filters output element (j0 + t / 3, t % 3) from the staged segment.
DE_DEV void os_v_filter(const ScaleArgs& a, const float* lds, int t, int column, int tile) {
    int lo, n;
    os_v_segment(a, tile, &lo, &n);
    const int j = tile * OS_V_TILE + t / 3, ch = t % 3;
    if (j >= a.n_dst) return;
    const int f = a.first[j];
    float acc = 0.0f;
    for (int k = 0; k < a.taps; ++k) {
        const int li = os_clampi(os_clampi(f + k, a.n_src) - lo, n);      // within the segment by construction; clamped into it all the same
        acc = acc + a.w[(size_t)k * (size_t)a.n_dst + (size_t)j] * lds[os_skew(li * 3 + ch)];
    }
    a.dst[((size_t)column * (size_t)a.n_dst + (size_t)j) * 3 + (size_t)ch] = a.clamp ? pack_clamp01(acc) : acc;
}

// Pass along u: thread t of the workgroup of (output column j, chunk) filters float e = 256 chunk + t of the column.
DE_DEV void os_u_filter(const ScaleArgs& a, int t, int j, int chunk) {
    const int e = chunk * OS_U_THREADS + t;
    if (j >= a.n_dst || e >= a.lines) return;
    const int f = a.first[j];
    float acc = 0.0f;
    for (int k = 0; k < a.taps; ++k) {
        const int i = os_clampi(f + k, a.n_src);
        acc = acc + a.w[(size_t)k * (size_t)a.n_dst + (size_t)j] * a.src[(size_t)i * (size_t)a.lines + (size_t)e];
    }
    a.dst[(size_t)j * (size_t)a.lines + (size_t)e] = a.clamp ? pack_clamp01(acc) : acc;
}

#ifndef DE_OUTPUT_SCALE_STANDALONE
#define OS_HOST_DEV __host__ __device__ inline      // the launchers size their grids with what the kernels divide by
#else
#define OS_HOST_DEV static inline
#endif
OS_HOST_DEV int os_v_tiles(int n_dst) { return (n_dst + OS_V_TILE - 1) / OS_V_TILE; }
OS_HOST_DEV int os_u_chunks(int lines) { return (lines + OS_U_THREADS - 1) / OS_U_THREADS; }

#ifndef DE_OUTPUT_SCALE_STANDALONE
__global__ void __launch_bounds__(OS_V_THREADS) output_scale_v_kernel(ScaleArgs a) {
    __shared__ float seg[OS_V_LDS_WORDS];
    const int tiles = os_v_tiles(a.n_dst);
    const int column = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    if (column >= a.lines) return;      // uniform per workgroup: ahead of the barrier
    os_v_stage(a, seg, (int)threadIdx.x, column, tile);
    __syncthreads();
    os_v_filter(a, seg, (int)threadIdx.x, column, tile);
}

__global__ void __launch_bounds__(OS_U_THREADS) output_scale_u_kernel(ScaleArgs a) {
    const int chunks = os_u_chunks(a.lines);
    os_u_filter(a, (int)threadIdx.x, (int)(blockIdx.x / (unsigned)chunks), (int)(blockIdx.x % (unsigned)chunks));
}
#endif

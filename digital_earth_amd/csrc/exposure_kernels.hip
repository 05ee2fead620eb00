// exposure_kernels.hip — the opt-in auto-exposure of the display path (include/digital_earth_exposure.h): histogram metering on the GPU
// ahead of the unchanged display transform.
//   meter_hist_kernel   a 256-bin histogram of the log2 luminance of what the display is about to read (8 bins per octave over [2^-24, 2^8), from the
//                       bit pattern: no transcendental); every workgroup STORES its 256 + 2 partial counts to its own row: no global atomics, nothing to clear
//   meter_solve_kernel  one workgroup: sums the rows, the trimmed mean between two percentiles and the EV update in f64, then writes a SECOND FrameConsts
//                       (a copy of the frame's with exposure_scale = 2^ev) that the display reads instead, and the result block of de_get_metering
// Integer counts: the histogram does not depend on the order of anything.  Included into de_api.hip's translation unit; display_kernel is untouched.
#include "de_kernels.h"
#include "display_source.h"

#define AE_BINS 256
#define AE_ROW 258          // a partial row: 256 bins, then the pixels below 2^-24 (not metered), then those at or above 2^8 (also in bin 255)
#define AE_MAX_WG 512       // two workgroups per CU: the rows the solve kernel has to sum stay at 528 KB

struct MeterArgs {
    DisplaySrc s;               // what the display launch is about to read
    int x0, y0, x1, y1;         // the metering region, half-open
    int gx0, gw;                // the region's columns in groups of 4 pixels: first group, groups per row
    uint32_t n_items;           // gw * (y1 - y0)
    uint32_t* partial;          // [gridDim.x][AE_ROW]
};

// Bin of a luminance: -1 for "below" (zero, negative, NaN, under 2^-24), else min((bits >> 20) - 824, 255): the exponent and the top three mantissa bits.
DE_DEV int ae_bin(float Y) {
    if (!(Y >= 0x1p-24f)) return -1;
    const uint32_t b = (de_f2u(Y) >> 20) - 824u;
    return (int)(b < 255u ? b : 255u);
}

// One count per live lane (code >= 0) into the wave's own LDS histogram.  Neighbouring pixels mostly share a bin, and a constant image puts all 64 lanes
// of every wave into one: LDS atomics on one address run one lane after the other, so the lanes that agree with the first live one are counted by ONE
// add of their number, and only the others add for themselves.  Called in wave-uniform control flow.
DE_DEV void ae_count(uint32_t* h, int code, uint32_t lane) {
    const bool live = code >= 0;
    const unsigned long long m = __ballot(live);
    if (m == 0ull) return;
    const uint32_t leader = (uint32_t)__builtin_ctzll(m);
    const int first = __builtin_amdgcn_readlane(code, (int)leader);
    const unsigned long long same = __ballot(live && code == first);
    if (lane == leader) atomicAdd(&h[first], (uint32_t)__builtin_popcountll(same));
    if (live && code != first) atomicAdd(&h[code], 1u);
}

// VEC: the buffer is 16-byte aligned (the context's own always are; a bound buffer or a display source may not be): a group of 4 pixels = 3 float4 loads.
template <bool VEC>
__global__ void __launch_bounds__(256) meter_hist_kernel(MeterArgs a) {
    __shared__ uint32_t hist[4][AE_ROW];      // one histogram per wave
    for (uint32_t i = threadIdx.x; i < 4u * AE_ROW; i += 256u) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* h = hist[threadIdx.x >> 6];
    const uint32_t stride = gridDim.x * 256u;
    // wave-uniform trip count: a lane past the end carries four dead pixels
    for (uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < a.n_items; base += stride) {
        const uint32_t item = base + lane;
        int code[4] = {-2, -2, -2, -2};       // -2: not in the region, -1: below, 0 .. 255: bin
        bool clipped[4] = {false, false, false, false};
        if (item < a.n_items) {
            const uint32_t row = item / (uint32_t)a.gw;
            const int j = a.y0 + (int)row, i0 = (a.gx0 + (int)(item - row * (uint32_t)a.gw)) * 4;      // i0 + 3 < W: W is a multiple of 16
            float px[12];
            src_load4<VEC>(a.s.hdr + ((size_t)j * a.s.W + i0) * 3, px);
            const float samples = src_samples(a.s, i0, j);      // display_pixel's own sample count and division
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + k;
                if (i < a.x0 || i >= a.x1) continue;
                const float r = px[3 * k] / samples, g = px[3 * k + 1] / samples, b = px[3 * k + 2] / samples;
                const float Y = src_luminance(r, g, b);
                code[k] = ae_bin(Y);
                clipped[k] = Y >= 0x1p8f;
            }
        }
        for (int k = 0; k < 4; ++k) {
            ae_count(h, code[k] == -1 ? AE_BINS : (code[k] == -2 ? -1 : code[k]), lane);      // "below" is column 256
            const unsigned long long mc = __ballot(clipped[k]);                               // one address: its first lane adds the wave's count
            if (mc != 0ull && lane == (uint32_t)__builtin_ctzll(mc)) atomicAdd(&h[AE_BINS + 1], (uint32_t)__builtin_popcountll(mc));
        }
    }
    __syncthreads();
    for (uint32_t col = threadIdx.x; col < AE_ROW; col += 256u)
        a.partial[(size_t)blockIdx.x * AE_ROW + col] = hist[0][col] + hist[1][col] + hist[2][col] + hist[3][col];
}

struct MeterState {
    double prev;           // the last EV, as the f32 that was used
    uint32_t has_prev;     // cleared by de_set_auto_exposure; survives de_reset
    uint32_t pad;
};
struct MeterResult {
    float ev, target, mean;
    uint32_t valid;
    unsigned long long n, below, clipped;
    uint32_t h[AE_BINS];
};
struct MeterSolveArgs {
    const uint32_t* partial;
    int n_rows;
    float low, high, adapt, compensation, ev_min, ev_max;
    float manual;              // de_params.exposure: what an all-black frame shows while there is no previous EV
    double log2_key;           // log2((double)key), from the host
    const double* centre;      // [AE_BINS] log2 of the bins' centres, from the host: the device computes no logarithm
    MeterState* state;
    const FrameConsts* fc;     // the frame's constants: read only (render launches in flight read them)
    FrameConsts* fc_ae;        // the copy the display reads
    MeterResult* res;
};

// One workgroup.  Everything after the integer sums is f64 with + - * /, floor and compare only (no contraction: -ffp-contract=off).
// The kernel is latency, not bandwidth: a thread sums up to 128 rows of its column, so the loads go out sixteen rows at a time before the first is
// waited for (a dependent L2 round trip per row would cost more than the whole display kernel), and the per-bin work — prefix count, retained count,
// r_k * centre_k — is done by 256 threads; one thread only adds the 256 terms, k ascending.
__global__ void __launch_bounds__(1024) meter_solve_kernel(MeterSolveArgs a) {
    __shared__ uint32_t part[4][AE_ROW];
    __shared__ uint32_t tot[AE_ROW];
    __shared__ double term[AE_BINS];
    __shared__ long long keep[AE_BINS];
    const uint32_t t = threadIdx.x, col = t & 255u, rg = t >> 8;
    {
        // the column of the bins, and with it one of the two counters behind them (every thread loads one; those of col < 2 are kept)
        const uint32_t* p0 = a.partial + col;
        const uint32_t* p1 = a.partial + AE_BINS + (col & 1u);
        uint32_t s = 0u, s2 = 0u;
        int r = (int)rg;
        for (; r + 60 < a.n_rows; r += 64) {
            uint32_t v[16], w[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) { v[u] = p0[(size_t)(r + 4 * u) * AE_ROW]; w[u] = p1[(size_t)(r + 4 * u) * AE_ROW]; }
#pragma unroll
            for (int u = 0; u < 16; ++u) { s += v[u]; s2 += w[u]; }
        }
        for (; r < a.n_rows; r += 4) { s += p0[(size_t)r * AE_ROW]; s2 += p1[(size_t)r * AE_ROW]; }
        part[rg][col] = s;
        if (col < 2u) part[rg][AE_BINS + col] = s2;
    }
    __syncthreads();
    if (t < AE_ROW) tot[t] = part[0][t] + part[1][t] + part[2][t] + part[3][t];
    __syncthreads();
    if (t < AE_BINS) {
        a.res->h[t] = tot[t];
        long long C = 0, N = 0;      // the exclusive prefix count of bin t, and the metered pixels
        for (int k = 0; k < AE_BINS; ++k) { const long long v = (long long)tot[k]; N += v; if (k < (int)t) C += v; }
        long long lo = (long long)__builtin_floor((double)a.low * (double)N), hi = (long long)__builtin_floor((double)a.high * (double)N);
        if (hi == lo) hi = lo + 1;
        const long long top = C + (long long)tot[t];
        const long long r = (top < hi ? top : hi) - (C > lo ? C : lo);      // the retained count of bin t
        keep[t] = r > 0 ? r : 0;
        term[t] = r > 0 ? (double)r * a.centre[t] : 0.0;
    }
    __syncthreads();
    if (t != 0u) return;
    unsigned long long N = 0ull;
    for (int k = 0; k < AE_BINS; ++k) N += tot[k];
    const bool has_prev = a.state->has_prev != 0u;
    const double prev = a.state->prev;
    double ev, target = 0.0, mean = 0.0;
    if (N > 0ull) {
        long long kept = 0;
        double acc = 0.0;
        for (int k = 0; k < AE_BINS; ++k) { acc += term[k]; kept += keep[k]; }      // k ascending; a bin that retains nothing adds an exact zero
        mean = acc / (double)kept;
        target = (a.log2_key - mean) + (double)a.compensation;
        if (target < (double)a.ev_min) target = (double)a.ev_min;
        if (target > (double)a.ev_max) target = (double)a.ev_max;
        ev = has_prev ? prev + (double)a.adapt * (target - prev) : target;
    } else {
        ev = has_prev ? prev : (double)a.manual;      // an all-black frame keeps the exposure
    }
    const float ev_f32 = (float)ev;
    if (N > 0ull) { a.state->prev = (double)ev_f32; a.state->has_prev = 1u; }
    FrameConsts f = *a.fc;
    f.exposure_scale = de_pow(2.0f, ev_f32);      // setup_kernel's own expression
    *a.fc_ae = f;
    a.res->ev = ev_f32;
    a.res->target = N > 0ull ? (float)target : ev_f32;
    a.res->mean = (float)mean;
    a.res->valid = N > 0ull ? 1u : 0u;
    a.res->n = N; a.res->below = tot[AE_BINS]; a.res->clipped = tot[AE_BINS + 1];
}

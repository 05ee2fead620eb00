// rgbe_kernels.hip — the opt-in Radiance HDR output in front of the display transform (include/digital_earth_rgbe.h): the frame's mean,
// or the mean a stage of the display chain made of it, becomes one complete .hdr file of RGBE pixels behind the front the host composed.  Four kernels,
// one after the other on the context stream, no atomics on global memory and no host synchronisation between them:
//   rgbe_convert_kernel  one thread per group of four pixels of a file row (display_source.h: src_load4, src_samples): the division and the scale as
//                        exr_layout_kernel has them, the conversion (rgbe_tables.h: rgbe_pixel), and the four bytes of each pixel into the row's
//                        four planes R, G, B, E of the planar buffer — one dword per plane, consecutive threads store consecutive bytes.  FLAT rows
//                        (RLE off, W < 8, W > 32767) go interleaved into their final place in the file instead.  It clears the status word.
//   rgbe_code_kernel     one 256-thread workgroup per (row, plane): the plane in LDS, each thread a contiguous span of at most 128 bytes, the three
//                        rounds of rgbe_tables.h between workgroup scans — where stretches begin and end across span boundaries, where literal
//                        regions do, what each position emits and its exclusive sum.  The packets go into the piece's slot; plane R's piece begins
//                        with the row's 02 02 hi(W) lo(W).
//   rgbe_scan_kernel     one workgroup: the coded tail's scan (coded_stream.h) with nothing behind a piece and no trailer; the front.
//   rgbe_compact_kernel  one workgroup per piece: the shared compaction from its slot.
// THE LDS IMAGE of rgbe_code_kernel: the plane, W bytes rounded up to 16 (dynamic, at most 32 768), and four arrays of 256 words for the scans
// (4 096 bytes): 36 864 bytes at the largest W, four workgroups per CU of 160 KiB.  THE WORST CASE of a slot is W + ceil(W / 128) (+ 4 in plane R's):
// the header's proof.  Every store into a slot and the file is checked; one that would pass is not made, raises the status word and the conversion
// ends with DE_ERR_INTERNAL.  (A flat row's place is a function of the launch's arguments alone: where it would pass the capacity the store is not
// made and the scan, which adds up the same numbers, raises the word — the convert kernel clears that word and must not also raise it.)
// Included into de_api.hip's translation unit behind exr_kernels.hip; it touches no other kernel.
#include "de_kernels.h"
#include "display_source.h"
#include "rgbe_tables.h"
#include "coded_stream.h"

struct RgbeArgs : CodedTail {   // the pieces are the rows' planes, 4 H of them (flat: none, and `front` holds the pixels too)
    DisplaySrc src;             // what is converted: [H][W][3] sums and their divisor
    int flip;                   // file row y is source row H - 1 - y (the context's frames: v = 0 at the bottom), else row y (de_debug_rgbe)
    float scale;
    int rounding, rle;
    uint8_t* planes;            // [H][4][plane_stride]: the bytes R, G, B, E of a row, planar
    uint32_t W, H, plane_stride;
    uint32_t header;            // the bytes of front_bytes
    uint8_t front_bytes[RGBE_FRONT_MAX];
};

// workgroups of 256 threads along a file row, four pixels per thread; the host sizes the flat grid by the same quotient (de_display.h: rg_launch)
DE_DEV uint32_t rgbe_row_workgroups(const RgbeArgs& a) { return ((a.W + 3u) / 4u + 255u) / 256u; }

// ---- the conversion
template <bool VEC>
__global__ void __launch_bounds__(256) rgbe_convert_kernel(RgbeArgs a) {
    const uint32_t wgs = rgbe_row_workgroups(a), y = blockIdx.x / wgs;      // a flat grid: rows may outnumber what a grid's second dimension takes
    const uint32_t g = (blockIdx.x - y * wgs) * 256u + threadIdx.x, x0 = 4u * g;
    if (y == 0u && g == 0u) *a.status = 0u;
    if (y >= a.H || x0 >= a.W) return;
    const uint32_t j = a.flip ? a.H - 1u - y : y;
    const float* p = a.src.hdr + ((size_t)j * (size_t)a.W + (size_t)x0) * 3u;
    const uint32_t n = a.W - x0 < 4u ? a.W - x0 : 4u;
    float px[12];
    if (VEC) src_load4<true>(p, px);      // (W is a multiple of 4 and the buffer 16-byte aligned)
    else for (uint32_t k = 0u; k < 3u * n; ++k) px[k] = p[k];
    const float samples = src_samples(a.src, (int)x0, (int)j);
    uint32_t pix[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0u; k < n; ++k)
        pix[k] = rgbe_pixel((px[3u * k] / samples) * a.scale, (px[3u * k + 1u] / samples) * a.scale, (px[3u * k + 2u] / samples) * a.scale, a.rounding);
    if (!a.rle) {      // interleaved, where the file has them
        const unsigned long long at = (unsigned long long)a.header + 4ull * ((unsigned long long)y * a.W + x0);
        if (at + 4ull * n > (unsigned long long)a.capacity) return;      // (the scan refuses such a total)
        uint8_t* dst = a.out + CS_WORD_BYTES + at;
        for (uint32_t k = 0u; k < n; ++k)
            for (uint32_t c = 0u; c < 4u; ++c) dst[4u * k + c] = (uint8_t)(pix[k] >> (8u * c));
        return;
    }
    for (uint32_t c = 0u; c < 4u; ++c) {
        uint8_t* plane = a.planes + ((size_t)y * 4u + c) * (size_t)a.plane_stride;
        const uint32_t sh = 8u * c;
        if (n == 4u) {      // 4-byte aligned: plane_stride is a multiple of 16, x0 of 4
            *reinterpret_cast<uint32_t*>(plane + x0) = ((pix[0] >> sh) & 0xffu) | (((pix[1] >> sh) & 0xffu) << 8) | (((pix[2] >> sh) & 0xffu) << 16) | (((pix[3] >> sh) & 0xffu) << 24);
        } else {
            for (uint32_t k = 0u; k < n; ++k) plane[x0 + k] = (uint8_t)(pix[k] >> sh);
        }
    }
}

// ---- the coder's scans over one word per thread, both exclusive: `up` the maximum over the threads in front of t (0 in front of the first), `down`
// the minimum over the threads behind it (`top` behind the last).  Hillis and Steele's steps between two buffers each.
DE_DEV void rgbe_scan_pair(uint32_t (*sa)[RGBE_THREADS], uint32_t (*sb)[RGBE_THREADS], uint32_t t, uint32_t up, uint32_t down, uint32_t top, uint32_t* before, uint32_t* behind) {
    const uint32_t r = RGBE_THREADS - 1u - t;      // the minimum runs over the mirrored index
    int cur = 0;
    sa[0][t] = up; sb[0][r] = down;
    __syncthreads();
    for (uint32_t d = 1u; d < RGBE_THREADS; d <<= 1) {
        uint32_t x = sa[cur][t], y = sb[cur][r];
        if (t >= d) { const uint32_t o = sa[cur][t - d]; x = x > o ? x : o; }
        if (r >= d) { const uint32_t o = sb[cur][r - d]; y = y < o ? y : o; }
        sa[cur ^ 1][t] = x; sb[cur ^ 1][r] = y;
        __syncthreads();
        cur ^= 1;
    }
    *before = t ? sa[cur][t - 1u] : 0u;
    *behind = r ? sb[cur][r - 1u] : top;
    __syncthreads();      // the buffers are free again
}
DE_DEV uint32_t rgbe_scan_sum(uint32_t (*sa)[RGBE_THREADS], uint32_t t, uint32_t v) {      // the exclusive sum
    int cur = 0;
    sa[0][t] = v;
    __syncthreads();
    for (uint32_t d = 1u; d < RGBE_THREADS; d <<= 1) {
        uint32_t x = sa[cur][t];
        if (t >= d) x += sa[cur][t - d];
        sa[cur ^ 1][t] = x;
        __syncthreads();
        cur ^= 1;
    }
    const uint32_t at = t ? sa[cur][t - 1u] : 0u;
    __syncthreads();
    return at;
}

// ---- the coder of one (row, plane)
extern __shared__ __align__(16) uint8_t rgbe_lds_plane[];
__global__ void __launch_bounds__(RGBE_THREADS) rgbe_code_kernel(RgbeArgs a) {
    __shared__ uint32_t sa[2][RGBE_THREADS], sb[2][RGBE_THREADS];
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    if (k >= a.count || a.W > RGBE_MAX_RLE_W || a.plane_stride < a.W) return;      // (uniform over the workgroup)
    const uint32_t c = k & 3u, W = a.W;
    uint8_t* plane = rgbe_lds_plane;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.planes + (size_t)k * (size_t)a.plane_stride);      // 16-byte aligned
        uint32_t* dst = reinterpret_cast<uint32_t*>(plane);
        for (uint32_t w = t; w < a.plane_stride / 4u; w += RGBE_THREADS) dst[w] = src[w];      // what lies behind W in the stride is never read below
    }
    __syncthreads();
    const RgbeSpan s = rgbe_span(W, t, RGBE_THREADS);
    uint32_t last, first, before, next, region, run_behind;
    rgbe_round1(plane, W, s, &last, &first);
    rgbe_scan_pair(sa, sb, t, last, first, W, &before, &next);
    rgbe_round2(plane, W, s, before, next, &last, &first);
    rgbe_scan_pair(sa, sb, t, last, first, W, &region, &run_behind);
    bool ok = true;
    const uint32_t n = rgbe_round3(plane, W, s, before, next, region, run_behind, nullptr, 0u, 0u, &ok);
    const uint32_t head = c == 0u ? 4u : 0u, at = head + rgbe_scan_sum(sa, t, n);
    uint8_t* slot = a.slots + (size_t)k * (size_t)a.slot_bytes;      // 16-byte aligned; slot_bytes is a multiple of 16
    rgbe_round3(plane, W, s, before, next, region, run_behind, slot, at, a.slot_bytes, &ok);
    if (t == 0u && head) {
        if (a.slot_bytes >= 4u) { slot[0] = 2u; slot[1] = 2u; slot[2] = (uint8_t)(W >> 8); slot[3] = (uint8_t)W; } else ok = false;
    }
    if (!ok) *a.status = CS_STATUS_OVERFLOW;
    if (t == RGBE_THREADS - 1u) {
        const uint32_t total = at + n;
        a.len[k] = total <= a.slot_bytes ? total : 0u;
        if (total > a.slot_bytes) *a.status = CS_STATUS_OVERFLOW;
    }
}

// ---- the scan: thread t owns pieces [t run, (t + 1) run); the front
__global__ void __launch_bounds__(CS_SCAN_THREADS) rgbe_scan_kernel(RgbeArgs a) {
    __shared__ uint32_t sums[CS_SCAN_THREADS];
    const uint32_t t = threadIdx.x;
    cs_scan_sum(a, sums, (int)t);
    if (t < a.header && t < RGBE_FRONT_MAX && t < a.capacity) a.out[CS_WORD_BYTES + t] = a.front_bytes[t];      // header <= RGBE_FRONT_MAX < CS_SCAN_THREADS
    __syncthreads();
    cs_scan_total(a, sums, (int)t);
    __syncthreads();
    cs_scan_offsets(a, sums, (int)t);
}

// ---- the compaction: the workgroup of piece i
__global__ void __launch_bounds__(256) rgbe_compact_kernel(RgbeArgs a) {
    (void)cs_compact(a, blockIdx.x, (int)threadIdx.x, 256);
}

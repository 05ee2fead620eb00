// exr_kernels.hip — the opt-in OpenEXR output in front of the display transform (include/digital_earth_exr.h): the frame's mean, or
// the mean a stage of the display chain made of it, becomes one complete scan-line file behind the front the host composed.  Six kernels (seven with
// AOV channels: include/digital_earth_exr_aovs.h), one after the other on the context stream, no atomics on global memory and no host
// synchronisation between them:
//   exr_layout_kernel    one thread per group of four pixels of a file row (display_source.h: src_load4, src_samples): the division, the scale, the
//                        conversion (exr_tables.h: exr_sample_bits, exr_half_bits), and the samples into the row's three planes B, G, R of the FRAMED
//                        raw buffer — per block its 8-byte header {y0, P} and its raw bytes r, which is what a raw block is in the file.  Consecutive
//                        threads store consecutive samples of one plane.  The planes' offsets within a line are the host's (exr_tables.h).
//   exr_aov_layout_kernel  only with AOV channels, on the same flat grid: a thread loads its four pixels' guides (two float4 and a float each, 16-byte
//                        loads), S1, S2 and the divisor — only what the mask selects; an unselected buffer may be null — and stores four
//                        consecutive samples into each selected plane of the same line (exr_tables.h: exr_aov_thread, every store checked
//                        against line_bytes).
//   exr_predict_kernel   ZIP / ZIPS: four bytes of p per thread from r (exr_predicted: the reorder and the predictor), one dword store.
//   exr_deflate_kernel   ZIP / ZIPS: one 512-thread workgroup per chunk of a block's p; the chunk's deflate data is the shared coder's
//                        (png_deflate.h: png_code_chunk) in the same LDS image, which keeps two workgroups per CU.  What is this file's alone: a
//                        block's first piece begins with the block header (dataSize left open) and 78 01, its last ends with four bytes of room
//                        for the Adler-32.
//   exr_block_kernel     one thread per block: the sum of its pieces, the raw fallback (Z >= P: the pieces become their shares of the framed raw
//                        buffer, the first with the header), else dataSize and the pieces' Adler partials joined (png_adler_join) into the room.
//   exr_scan_kernel      one workgroup: the coded tail's scan (coded_stream.h) with nothing behind a piece and no trailer; the front.
//   exr_compact_kernel   one workgroup per piece: the shared compaction from its slot or from the raw buffer; a block's first also writes the
//                        block's entry of the offset table.
// THE WORST CASE of a slot (exr_tables.h: EXR_CHUNK_OVERHEAD) is the PNG slot's, n + 24; of the file, front + 8 nb + H W 3 bps, by the raw fallback.
// Every store into the LDS image, a slot and the file is checked; one that would pass raises the status word and the conversion ends with
// DE_ERR_INTERNAL.
// Included into de_api.hip's translation unit behind png_kernels.hip; it touches no other kernel.
#include "de_kernels.h"
#include "display_source.h"
#include "png_tables.h"
#include "png_deflate.h"
#include "exr_tables.h"
#include "coded_stream.h"

struct ExrArgs : CodedTail {    // the pieces are the blocks' chunks (NONE: the blocks): count of them; front: the bytes of front_bytes and the table
    DisplaySrc src;             // what is converted: [H][W][3] sums and their divisor
    int flip;                   // file row y is source row H - 1 - y (the context's frames: v = 0 at the bottom), else row y (de_debug_exr)
    float scale;
    const PngTables* tab;
    uint8_t* raw;               // [blocks][r_stride]: {int32 y0, int32 P}, r
    uint8_t* pred;              // [blocks][p_stride]: p
    uint32_t* adler;            // [count][2]: A and B of the chunk's own bytes, from (0, 0)
    uint32_t* alt_w;            // alt_at, to be written
    int pixel_type, compression;
    uint32_t W, H, L, line_bytes, block_bytes, blocks, chunk, cpb, r_stride, p_stride;
    uint32_t front_fixed;       // the header's bytes in front_bytes: 313 with B, G, R alone
    uint32_t rgb_offset[3];     // of the planes of R, G, B within a line (B, G, R alone: 2 W bps, W bps, 0), each of W bps bytes
    uint32_t rgb_bps;
    const float* counts;        // the divisor per pixel, [H][W] (de_debug_exr_aovs), else null: src_samples
    ExrAov aov;                 // the AOV planes and what they read; aov.planes == 0: none, exr_aov_layout_kernel does not run
    uint8_t front_bytes[EXR_FRONT_MAX];
};

DE_DEV uint32_t exr_block_P(const ExrArgs& a, uint32_t b) {      // P of block b
    const uint32_t y0 = b * a.L, lines = a.H - y0 < a.L ? a.H - y0 : a.L;
    return lines * a.line_bytes;
}

// workgroups of 256 threads along a file row (four pixels per thread) and along a full block's p (four bytes per thread); the host sizes the flat grids by the same quotients (de_display.h: ex_launch)
DE_DEV uint32_t exr_row_workgroups(const ExrArgs& a) { return ((a.W + 3u) / 4u + 255u) / 256u; }
DE_DEV uint32_t exr_block_workgroups(const ExrArgs& a) { return ((a.block_bytes + 3u) / 4u + 255u) / 256u; }

// ---- the layout
template <bool VEC>
__global__ void __launch_bounds__(256) exr_layout_kernel(ExrArgs a) {
    const uint32_t wgs = exr_row_workgroups(a), y = blockIdx.x / wgs;      // a flat grid: rows may outnumber what a grid's second dimension takes
    const uint32_t g = (blockIdx.x - y * wgs) * 256u + threadIdx.x, x0 = 4u * g;
    if (y == 0u && g == 0u) *a.status = 0u;
    if (y >= a.H || x0 >= a.W) return;
    const uint32_t j = a.flip ? a.H - 1u - y : y;
    const uint32_t b = y / a.L, line = y - b * a.L;
    uint8_t* block = a.raw + (size_t)b * (size_t)a.r_stride;
    if (line == 0u && g == 0u) {      // the block's header as a raw block carries it
        uint32_t* head = reinterpret_cast<uint32_t*>(block);      // 16-byte aligned: r_stride is a multiple of 16
        head[0] = y; head[1] = exr_block_P(a, b);
    }
    const float* p = a.src.hdr + ((size_t)j * (size_t)a.W + (size_t)x0) * 3u;
    const uint32_t n = a.W - x0 < 4u ? a.W - x0 : 4u;
    float px[12];
    if (VEC) src_load4<true>(p, px);      // (W is a multiple of 4 and the buffer 16-byte aligned)
    else for (uint32_t k = 0u; k < 3u * n; ++k) px[k] = p[k];
    float samples[4];
    samples[0] = src_samples(a.src, (int)x0, (int)j);
    for (uint32_t k = 1u; k < 4u; ++k) samples[k] = samples[0];
    if (a.counts) for (uint32_t k = 0u; k < n; ++k) samples[k] = a.counts[(size_t)j * (size_t)a.W + x0 + k];
    uint8_t* row = block + EXR_BLOCK_HEADER + (size_t)line * (size_t)a.line_bytes;
    for (uint32_t ch = 0u; ch < 3u; ++ch) {      // the planes of R, G, B where the host's sort put them
        const uint32_t off = a.rgb_offset[ch];
        if ((size_t)off + (size_t)a.W * (size_t)a.rgb_bps > (size_t)a.line_bytes) continue;      // (the host's offsets lie inside the line)
        if (a.pixel_type == EXR_PIXEL_HALF) {
            uint16_t* dst = reinterpret_cast<uint16_t*>(row + off) + x0;
            for (uint32_t k = 0u; k < n; ++k) dst[k] = (uint16_t)exr_half_bits(exr_sample_bits(px[3u * k + ch] / samples[k], a.scale));
        } else {
            uint32_t* dst = reinterpret_cast<uint32_t*>(row + off) + x0;
            for (uint32_t k = 0u; k < n; ++k) dst[k] = exr_sample_bits(px[3u * k + ch] / samples[k], a.scale);
        }
    }
}

// ---- the AOV planes of the same line: the layout's grid, thread for thread; it writes no plane the layout writes and no block header
template <bool VEC>
__global__ void __launch_bounds__(256) exr_aov_layout_kernel(ExrArgs a) {
    const uint32_t wgs = exr_row_workgroups(a), y = blockIdx.x / wgs;
    const uint32_t g = (blockIdx.x - y * wgs) * 256u + threadIdx.x, x0 = 4u * g;
    if (y >= a.H || x0 >= a.W) return;
    const uint32_t j = a.flip ? a.H - 1u - y : y;
    const uint32_t b = y / a.L, line = y - b * a.L;
    if (b >= a.blocks || (size_t)EXR_BLOCK_HEADER + (size_t)(line + 1u) * (size_t)a.line_bytes > (size_t)a.r_stride) return;      // the line lies in its block
    uint8_t* row = a.raw + (size_t)b * (size_t)a.r_stride + EXR_BLOCK_HEADER + (size_t)line * (size_t)a.line_bytes;
    if (!exr_aov_thread<VEC>(a.aov, row, a.line_bytes, a.W, x0, j)) *a.status = CS_STATUS_OVERFLOW;
}

// ---- the reorder and the predictor: thread g of a block owns p[4 g .. 4 g + 4); a flat grid, as the layout's
__global__ void __launch_bounds__(256) exr_predict_kernel(ExrArgs a) {
    const uint32_t wgs = exr_block_workgroups(a), b = blockIdx.x / wgs, i0 = 4u * ((blockIdx.x - b * wgs) * 256u + threadIdx.x);
    if (b >= a.blocks) return;
    const uint32_t P = exr_block_P(a, b);
    if (i0 >= P) return;
    const uint8_t* r = a.raw + (size_t)b * (size_t)a.r_stride + EXR_BLOCK_HEADER;
    uint8_t* p = a.pred + (size_t)b * (size_t)a.p_stride;
    if (i0 + 4u <= P) {
        uint32_t w = 0u;
        for (uint32_t k = 0u; k < 4u; ++k) w |= exr_predicted(r, P, i0 + k) << (8u * k);
        *reinterpret_cast<uint32_t*>(p + i0) = w;      // 4-byte aligned: p_stride is a multiple of 16
    } else {
        for (uint32_t i = i0; i < P; ++i) p[i] = (uint8_t)exr_predicted(r, P, i);
    }
}

// ---- the coder of one chunk: png_deflate.h; here, what a block puts around its first and last
__global__ void __launch_bounds__(PNG_THREADS) exr_deflate_kernel(ExrArgs a) {
    __shared__ PngLds s;
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    if (k >= a.count) return;
    const uint32_t b = k / a.cpb, j = k - b * a.cpb;
    const uint32_t P = exr_block_P(a, b), off = j * a.chunk;
    if (off >= P) {      // the last block is shorter and needs fewer pieces: an empty one
        if (t == 0u) { a.len[k] = 0u; a.alt_w[k] = CS_NO_ALT; a.adler[2u * k] = 0u; a.adler[2u * k + 1u] = 0u; }
        return;
    }
    const uint32_t n = P - off < a.chunk ? P - off : a.chunk;
    const bool first = j == 0u, final_chunk = off + n == P;
    const uint8_t* c = a.pred + (size_t)b * (size_t)a.p_stride + off;
    const uint32_t d0 = first ? EXR_BLOCK_HEADER + 2u : 0u;      // the deflate data's first byte in the image
    const uint32_t end = png_code_chunk(s, *a.tab, c, n, t, d0, final_chunk);
    if (t == 0u && first) {
        png_put(s, 0u, b * a.L, 32u);      // y0; dataSize is the block step's
        png_put(s, 64u, 0x0178u, 16u);
    }
    __syncthreads();
    const uint32_t bytes = end + (final_chunk ? 4u : 0u);      // room for the Adler-32, which is the block step's too
    const bool fits = !s.overflow && bytes <= a.slot_bytes && bytes <= PNG_BUF_WORDS * 4u;
    if (fits) {
        uint32_t* slot = reinterpret_cast<uint32_t*>(a.slots + (size_t)k * (size_t)a.slot_bytes);      // 16-byte aligned; slot_bytes is a multiple of 16
        for (uint32_t w = t; w < (bytes + 3u) / 4u; w += PNG_THREADS) slot[w] = s.buf[w];
    }
    if (t == 0u) {
        a.len[k] = fits ? bytes : 0u;
        a.alt_w[k] = CS_NO_ALT;
        a.adler[2u * k] = (uint32_t)(s.adler[0] % PNG_ADLER);
        a.adler[2u * k + 1u] = (uint32_t)(s.adler[1] % PNG_ADLER);
        if (!fits) *a.status = CS_STATUS_OVERFLOW;
    }
}

// ---- the block step: thread b
__global__ void __launch_bounds__(256) exr_block_kernel(ExrArgs a) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= a.blocks) return;
    const uint32_t P = exr_block_P(a, b), k0 = b * a.cpb;
    const uint32_t raw_at = b * a.r_stride;      // of the block's header in the framed raw buffer
    if (a.compression == EXR_COMPRESSION_NONE) {      // one piece: the framed block as it lies
        a.len[k0] = EXR_BLOCK_HEADER + P; a.alt_w[k0] = raw_at;
        return;
    }
    const uint32_t chunks = (P + a.chunk - 1u) / a.chunk;
    unsigned long long A = 1ull, B = 0ull;
    uint32_t sum = 0u;
    bool failed = false;
    for (uint32_t j = 0u; j < chunks; ++j) {
        const uint32_t n = P - j * a.chunk < a.chunk ? P - j * a.chunk : a.chunk;
        const uint32_t l = a.len[k0 + j];
        if (!l) failed = true;      // its coder has raised the status word
        sum += l;
        png_adler_join(&A, &B, n, a.adler[2u * (k0 + j)], a.adler[2u * (k0 + j) + 1u]);
    }
    if (failed) return;
    const uint32_t Z = sum - EXR_BLOCK_HEADER;      // 78 01, the chunks, the Adler-32
    if (Z >= P) {      // the raw fallback: piece j is its share of r, the first behind the header
        for (uint32_t j = 0u; j < chunks; ++j) {
            const uint32_t n = P - j * a.chunk < a.chunk ? P - j * a.chunk : a.chunk;
            a.len[k0 + j] = n + (j ? 0u : EXR_BLOCK_HEADER);
            a.alt_w[k0 + j] = raw_at + (j ? EXR_BLOCK_HEADER + j * a.chunk : 0u);
        }
        return;
    }
    uint8_t* head = a.slots + (size_t)k0 * (size_t)a.slot_bytes + 4u;
    const uint32_t last = k0 + chunks - 1u, l = a.len[last];
    if (l < 4u || l > a.slot_bytes) { *a.status = CS_STATUS_OVERFLOW; return; }
    uint8_t* tail = a.slots + (size_t)last * (size_t)a.slot_bytes + (l - 4u);
    const uint32_t adler = (uint32_t)((B << 16) | A);
    for (int i = 0; i < 4; ++i) { head[i] = (uint8_t)(Z >> (8 * i)); tail[i] = (uint8_t)(adler >> (24 - 8 * i)); }
}

// ---- the scan: thread t owns pieces [t run, (t + 1) run)
__global__ void __launch_bounds__(CS_SCAN_THREADS) exr_scan_kernel(ExrArgs a) {
    __shared__ uint32_t sums[CS_SCAN_THREADS];
    const uint32_t t = threadIdx.x;
    cs_scan_sum(a, sums, (int)t);
    if (t < a.front_fixed && t < EXR_FRONT_MAX && t < a.capacity) a.out[CS_WORD_BYTES + t] = a.front_bytes[t];      // front_fixed <= 626 < CS_SCAN_THREADS
    __syncthreads();
    cs_scan_total(a, sums, (int)t);
    __syncthreads();
    cs_scan_offsets(a, sums, (int)t);
}

// ---- the compaction: the workgroup of piece i; a block's first piece brings the block's entry of the offset table
__global__ void __launch_bounds__(256) exr_compact_kernel(ExrArgs a) {
    const uint32_t i = blockIdx.x;
    const bool moved = cs_compact(a, i, (int)threadIdx.x, 256);
    if (!moved || threadIdx.x != 0u) return;
    const uint32_t b = i / a.cpb;
    if (i != b * a.cpb) return;
    const uint32_t at = a.front_fixed + 8u * b;
    if (at + 8u > a.front || a.front > a.capacity) return;
    uint8_t* entry = a.out + CS_WORD_BYTES + at;
    const uint32_t offset = a.offset[i];
    for (int k = 0; k < 8; ++k) entry[k] = k < 4 ? (uint8_t)(offset >> (8 * k)) : (uint8_t)0;
}

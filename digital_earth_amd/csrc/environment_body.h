// environment_body.h — the two phases of environment_capture_kernel (environment_kernels.hip, include/digital_earth_environment.h), free
// of anything of the device, so that a host build (tools/environment_host_check.cpp) runs them thread by thread under the sanitizers.  The includer
// brings DE_DEV and display_source.h (DisplaySrc, src_samples).
// One workgroup of ENV_THREADS threads moves one ENV_TILE x ENV_TILE tile of pixels from the sums, [N][N][3] with the pixels of a ROW j contiguous, into
// a face slot, index (i N + j) 3 + c with the pixels of a COLUMN i contiguous, through a tile of its own:
//   load    element e = t, t + 256, ... of the tile's 32 rows of 96 floats: row e / 96, float e % 96 of the row.  The 32 lanes of half a wave read 32
//           consecutive floats of one row of the sums (96 is a multiple of 32: half a wave never spans two rows), divide each by its pixel's count
//           (one IEEE float32 division: display_source.h's src_samples, the frame's count or the 8 x 8 tile's own) and write 32 consecutive words of
//           the tile: no bank shared.
//   store   the same e read the other way round: column e / 96 of the tile, float e % 96 = 3 jl + c of that column.  Half a wave stores 32 consecutive
//           floats of one column of the slot.  Its tile words are jl ENV_STRIDE + 3 il + c with il fixed: ENV_STRIDE = 99 = 3 (mod 32), so the word's
//           bank is (3 jl + c + 3 il) mod 32 = (e + 3 il) mod 32 — 32 lanes, 32 banks (96 would put every jl on one bank, 97 three lanes on one).
// Every load and every store is range-checked against N; nothing is staged that is not read back once, transposed — that reuse is what the tile is for.
#pragma once
#include <stdint.h>

#define ENV_TILE 32
#define ENV_ROW (ENV_TILE * 3)                 // the floats of a tile row
#define ENV_STRIDE (ENV_ROW + 3)               // of a tile row in the staging tile
#define ENV_TILE_FLOATS (ENV_TILE * ENV_STRIDE)
#define ENV_THREADS 256

// Thread t's share of the load: rows j0 ... j0 + 31 of the source, columns i0 ... i0 + 31, each channel divided by its pixel's count.
DE_DEV void env_tile_load(const DisplaySrc& s, int i0, int j0, int t, float* tile) {
    for (int e = t; e < ENV_TILE * ENV_ROW; e += ENV_THREADS) {
        const int row = e / ENV_ROW, col = e - row * ENV_ROW;
        const int j = j0 + row, i = i0 + col / 3;
        if (j >= s.H || i >= s.W) continue;
        tile[row * ENV_STRIDE + col] = s.hdr[((size_t)j * (size_t)s.W + (size_t)i0) * 3 + (size_t)col] / src_samples(s, i, j);
    }
}

// Thread t's share of the store: columns i0 ... i0 + 31 of the slot (N x N x 3, index (i N + j) 3 + c), rows j0 ... j0 + 31.
DE_DEV void env_tile_store(float* slot, int N, int i0, int j0, int t, const float* tile) {
    for (int e = t; e < ENV_TILE * ENV_ROW; e += ENV_THREADS) {
        const int il = e / ENV_ROW, rem = e - il * ENV_ROW, jl = rem / 3, ch = rem - jl * 3;
        const int i = i0 + il, j = j0 + jl;
        if (i >= N || j >= N) continue;
        slot[((size_t)i * (size_t)N + (size_t)j) * 3 + (size_t)ch] = tile[jl * ENV_STRIDE + il * 3 + ch];
    }
}

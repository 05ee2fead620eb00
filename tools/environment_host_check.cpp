// environment_host_check.cpp — the two phases of the scene-linear panorama's capture kernel (csrc/environment_body.h: env_tile_load, env_tile_store)
// compiled for the HOST, so that the address and undefined-behaviour sanitizers can watch every index they form (tools/environment_host_check.py
// builds and drives this).  The launch is replayed workgroup by workgroup, thread by thread, on heap blocks of exactly their sizes:
// the sums (N N 3 floats), the tile counts ((N / 8)^2 int32, when given), one staging tile per workgroup (ENV_TILE_FLOATS floats, filled with NaN
// first: a word the load did not write and the store reads would show) and the slot (N N 3 floats).
//   environment_host_check IN OUT
// IN: int32 N, samples, per_tile; f32 sums [N][N][3]; per_tile: int32 counts [N / 8][N / 8].  OUT: the slot, (N, N, 3) f32, index (i N + j) 3 + c.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define DE_DEV static inline
struct float4 { float x, y, z, w; };      // display_source.h's vector load; not run here
#include "../digital_earth_amd/csrc/display_source.h"
#include "../digital_earth_amd/csrc/environment_body.h"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);      // exactly n elements on the heap: one index past either end is the sanitizer's to find
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> head = take<int32_t>(f, 3);
    const int N = head[0];
    if (N < 8 || (N % 8) != 0 || head[1] < 1) return 2;
    const std::vector<float> sums = take<float>(f, (size_t)N * N * 3);
    const std::vector<int32_t> counts = take<int32_t>(f, head[2] ? (size_t)(N / 8) * (N / 8) : 0);
    fclose(f);
    DisplaySrc s;
    s.hdr = sums.data(); s.tile_spp = head[2] ? counts.data() : nullptr; s.samples = head[1]; s.W = N; s.H = N;
    std::vector<float> slot((size_t)N * N * 3, NAN);
    const int tiles = (N + ENV_TILE - 1) / ENV_TILE;
    for (int block = 0; block < tiles * tiles; ++block) {      // the kernel's decode of blockIdx.x
        const int i0 = (block % tiles) * ENV_TILE, j0 = (block / tiles) * ENV_TILE;
        std::vector<float> tile(ENV_TILE_FLOATS, NAN);
        for (int t = 0; t < ENV_THREADS; ++t) env_tile_load(s, i0, j0, t, tile.data());
        for (int t = 0; t < ENV_THREADS; ++t) env_tile_store(slot.data(), N, i0, j0, t, tile.data());      // behind the barrier
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(slot.data(), sizeof(float), slot.size(), f);
    fclose(f);
    return 0;
}

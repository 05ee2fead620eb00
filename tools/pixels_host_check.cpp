// pixels_host_check.cpp — pixels_pack_kernel's own source (csrc/pixels_kernels.hip) compiled for the HOST, so that the address and undefined-behaviour
// sanitizers can watch every index it forms (tools/pixels_host_check.py builds and drives this).  The kernel is its two halves around one
// barrier: this program runs the first half for the 256 threads of a workgroup, then the second, one workgroup at a time, on a heap tile of exactly the
// kernel's LDS size filled with a pattern no staged pixel can hold (a read of a word that was never staged would show in the bytes).
//   pixels_host_check IN OUT
// IN: int32 W, H, channels, mode; uint32 seed, phase; then the image (W, H, 3) f32 as the display writes it.  OUT: [H][W][channels] bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_PIXELS_STANDALONE
#define DE_DEV static inline
#include "../digital_earth_amd/csrc/pixels_kernels.hip"

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
    const std::vector<int32_t> head = take<int32_t>(f, 4);
    const std::vector<uint32_t> hash = take<uint32_t>(f, 2);
    const int W = head[0], H = head[1];
    const std::vector<float> image = take<float>(f, (size_t)W * H * 3);
    fclose(f);
    std::vector<uint32_t> out32((size_t)W * H * head[2] / 4);      // dword-aligned, exactly W * H * channels bytes
    PixelsArgs a;
    a.image = image.data(); a.out = reinterpret_cast<uint8_t*>(out32.data()); a.W = W; a.H = H; a.channels = head[2]; a.mode = head[3]; a.seed = hash[0]; a.phase = hash[1];
    for (int by = 0; by < (H + PX_TILE - 1) / PX_TILE; ++by)
        for (int bx = 0; bx < (W + PX_TILE - 1) / PX_TILE; ++bx) {
            std::vector<uint32_t> lds((size_t)PX_TILE * PX_LDS_STRIDE, 0xA5000000u);      // staged words have a zero top byte
            uint32_t (*tile)[PX_LDS_STRIDE] = reinterpret_cast<uint32_t (*)[PX_LDS_STRIDE]>(lds.data());
            for (int t = 0; t < 256; ++t) pixels_stage_tile(a, tile, t, bx, by);
            for (int t = 0; t < 256; ++t) pixels_store_tile(a, tile, t, bx, by);
        }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out32.data(), 1, (size_t)W * H * head[2], f);
    fclose(f);
    return 0;
}

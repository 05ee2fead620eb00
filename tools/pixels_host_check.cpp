// pixels_host_check.cpp — the pixel packs' own source (csrc/pixels_kernels.hip: pixels_pack_kernel; csrc/hdr_pack.h: hdr_pack_kernel; both over
// csrc/pack.h) compiled for the HOST, so that the address and undefined-behaviour sanitizers can watch every index they form
// (tools/pixels_host_check.py builds and drives this).  Each kernel is its two halves around one barrier: this program runs the
// first half for the 256 threads of a workgroup, then the second, one workgroup at a time, on a heap tile of exactly the kernel's LDS size filled with a
// pattern no staged word can hold (a read of a word that was never staged would show in the bytes), into a heap buffer of exactly the output's size.
//   pixels_host_check IN OUT
// IN: int32 W, H, format, mode; uint32 seed, phase; then the image (W, H, 3) f32 as the display writes it.  format: 3 = RGB8, 4 = RGBA8 (the 8-bit pack's
// channels), 10 = RGB10A2, 16 = RGB16 (the HDR pack).  OUT: [H][W][channels] bytes, [H][W] uint32 or [H][W][3] uint16.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_PIXELS_STANDALONE
#define DE_DEV static inline
#include "../digital_earth_amd/csrc/pixels_kernels.hip"
#include "../digital_earth_amd/csrc/hdr_pack.h"

// 0xA5000000: an 8-bit staged word has a zero top byte, an RGB10A2 word both top bits set, an RGB16 plane word at most 0xffff.
static const uint32_t LDS_FILL = 0xA5000000u;

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
    const int format = head[2];
    const bool hdr = format == 10 || format == 16;
    if (!hdr && format != 3 && format != 4) return 2;
    const size_t out_bytes = (size_t)W * H * (hdr ? (format == 16 ? 6 : 4) : format);      // a multiple of 4: W is a multiple of 16
    std::vector<uint32_t> out32(out_bytes / 4);                   // dword-aligned, exactly the output
    PixelsArgs a;
    a.image = image.data(); a.out = reinterpret_cast<uint8_t*>(out32.data()); a.W = W; a.H = H; a.channels = format; a.mode = head[3]; a.seed = hash[0]; a.phase = hash[1];
    HdrPackArgs h;
    h.image = image.data(); h.out = out32.data(); h.W = W; h.H = H; h.format = format == 16 ? 1 : 0; h.mode = head[3]; h.seed = hash[0]; h.phase = hash[1];
    for (int by = 0; by < (H + PACK_TILE - 1) / PACK_TILE; ++by)
        for (int bx = 0; bx < (W + PACK_TILE - 1) / PACK_TILE; ++bx) {
            std::vector<uint32_t> lds((size_t)(hdr ? HPX_PLANES : 1) * PACK_TILE * PACK_LDS_STRIDE, LDS_FILL);
            if (hdr) {
                uint32_t (*tile)[PACK_TILE][PACK_LDS_STRIDE] = reinterpret_cast<uint32_t (*)[PACK_TILE][PACK_LDS_STRIDE]>(lds.data());
                for (int t = 0; t < 256; ++t) hdr_stage_tile(h, tile, t, bx, by);
                for (int t = 0; t < 256; ++t) hdr_store_tile(h, tile, t, bx, by);
            } else {
                uint32_t (*tile)[PACK_LDS_STRIDE] = reinterpret_cast<uint32_t (*)[PACK_LDS_STRIDE]>(lds.data());
                for (int t = 0; t < 256; ++t) pixels_stage_tile(a, tile, t, bx, by);
                for (int t = 0; t < 256; ++t) pixels_store_tile(a, tile, t, bx, by);
            }
        }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out32.data(), 1, out_bytes, f);
    fclose(f);
    return 0;
}

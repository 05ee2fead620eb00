// video_host_check.cpp — videoframe_pack_kernel's own source (csrc/videoframe_kernels.hip) compiled for the HOST, so that the address and undefined-behaviour
// sanitizers can watch every index it forms.  The kernel is three steps around two barriers: this program runs each step for the 256
// threads of a workgroup in turn, one workgroup at a time, on a heap tile of exactly the kernel's LDS size, and writes into a heap frame of exactly
// the frame's size: one index past either end of either is the sanitizer's to find.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off tools/video_host_check.cpp -o video_host_check
//   video_host_check            every format x siting x mode over the test sizes (16x8, 18x10, 20x6, 34x34, 80x56, 208x120) on an image of its own; each
//                               frame is packed twice over different fill patterns and the two must agree: every byte of the frame is written
//   video_host_check IN OUT     one conversion.  IN: int32 W, H, format, matrix, range, siting, mode; uint32 seed, phase; then the image (W, H, 3) f32
//                               as the display writes it.  OUT: the frame.  (tests/video_ref.py's pack() gives the same bytes.)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_VIDEO_STANDALONE
#define DE_DEV static inline
#include "../digital_earth_amd/csrc/videoframe_kernels.hip"

static size_t frame_bytes(int W, int H, int format) { return (size_t)W * H / 2 * 3 * (format >= 2 ? 2 : 1); }

static std::vector<uint32_t> run(const std::vector<float>& image, int W, int H, int format, int matrix, int range, int siting, int mode, uint32_t seed, uint32_t phase, uint32_t fill) {
    const size_t bytes = frame_bytes(W, H, format);      // a multiple of 4 whenever a 32-bit store is taken; otherwise at least even
    std::vector<uint32_t> out32((bytes + 3) / 4, fill);
    std::vector<uint8_t> exact(bytes, (uint8_t)fill);     // exactly the frame: no slack behind it
    VideoArgs a;
    a.image = image.data(); a.W = W; a.H = H; a.format = format; a.siting = siting; a.mode = mode; a.seed = seed; a.phase = phase;
    a.k = vd_make_consts(format, matrix, range);
    // the 32-bit stores need a 4-byte aligned base, as hipMalloc gives: operator new's is 16-byte aligned
    a.out = exact.data();
    for (int by = 0; by < (H + PACK_TILE - 1) / PACK_TILE; ++by)
        for (int bx = 0; bx < (W + PACK_TILE - 1) / PACK_TILE; ++bx) {
            std::vector<VideoTile> lds(1);
            memset(&lds[0], 0xA5, sizeof(VideoTile));      // a staged word never read before it is written would show in the bytes
            for (int t = 0; t < 256; ++t) vd_stage_tile(a, lds[0], t, bx, by);
            for (int t = 0; t < 256; ++t) vd_chroma_tile(a, lds[0], t, bx, by);
            for (int t = 0; t < 256; ++t) vd_store_tile(a, lds[0], t, bx, by);
        }
    memcpy(out32.data(), exact.data(), bytes);
    return out32;
}

static std::vector<float> test_image(int W, int H) {
    std::vector<float> img((size_t)W * H * 3);
    uint32_t s = 12345u + (uint32_t)W * 131u + (uint32_t)H;
    for (size_t i = 0; i < img.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        img[i] = (float)(s >> 8) * (1.2f / 16777216.0f) - 0.1f;
    }
    const float special[] = {-0.0f, NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e-45f, 1.0f, 0.0f};
    for (size_t i = 0; i < sizeof(special) / sizeof(special[0]) && 2 * i + 1 < img.size(); ++i) img[2 * i + 1] = special[i];
    return img;
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
        const std::vector<int32_t> head = take<int32_t>(f, 7);
        const std::vector<uint32_t> hash = take<uint32_t>(f, 2);
        const int W = head[0], H = head[1];
        if (W <= 0 || H <= 0 || (W & 1) || (H & 1)) return 2;
        const std::vector<float> image = take<float>(f, (size_t)W * H * 3);
        fclose(f);
        const std::vector<uint32_t> out = run(image, W, H, head[2], head[3], head[4], head[5], head[6], hash[0], hash[1], 0u);
        f = fopen(argv[2], "wb");
        if (!f) return 2;
        fwrite(out.data(), 1, frame_bytes(W, H, head[2]), f);
        fclose(f);
        return 0;
    }
    if (argc != 1) return 2;
    static const int sizes[][2] = {{16, 8}, {18, 10}, {20, 6}, {34, 34}, {80, 56}, {208, 120}, {2, 2}, {66, 2}};
    int runs = 0;
    for (const auto& sz : sizes) {
        const std::vector<float> image = test_image(sz[0], sz[1]);
        for (int format = 0; format < 4; ++format)
            for (int siting = 0; siting < 3; ++siting)
                for (int mode = 0; mode < 3; ++mode) {
                    const int matrix = (format + siting) % 3, range = (siting + mode) & 1;
                    const std::vector<uint32_t> a = run(image, sz[0], sz[1], format, matrix, range, siting, mode, 7u, (uint32_t)mode, 0x00000000u);
                    const std::vector<uint32_t> b = run(image, sz[0], sz[1], format, matrix, range, siting, mode, 7u, (uint32_t)mode, 0xffffffffu);
                    if (memcmp(a.data(), b.data(), frame_bytes(sz[0], sz[1], format)) != 0) {
                        fprintf(stderr, "%d x %d format %d siting %d mode %d: a byte of the frame was not written\n", sz[0], sz[1], format, siting, mode);
                        return 1;
                    }
                    ++runs;
                }
    }
    printf("video_host_check: %d conversions, every frame byte written, no sanitizer report\n", runs);
    return 0;
}

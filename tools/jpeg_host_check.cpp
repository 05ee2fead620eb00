// jpeg_host_check.cpp — the JPEG kernels' own source (csrc/jpeg_kernels.hip, behind csrc/videoframe_kernels.hip) compiled for the HOST, so that the address
// and undefined-behaviour sanitizers can watch every index they form.  Each kernel is a sequence of leaves around barriers: this program
// runs each leaf for every thread of a workgroup in turn, one workgroup at a time, on heap buffers of exactly the sizes the library allocates, so one
// index past an end is the sanitizer's to find.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off tools/jpeg_host_check.cpp -o jpeg_host_check
//   jpeg_host_check            a sweep of its own over sizes, qualities and restart intervals on noise and on flat images; every stream must end in EOI
//   jpeg_host_check IN OUT     one conversion.  IN: int32 W, H, quality, restart; then the image (W, H, 3) f32 as the display writes it.  OUT: the stream.
//                              (tests/jpeg_ref.py's encode() gives the same bytes.)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_VIDEO_STANDALONE
#define DE_JPEG_STANDALONE
#define DE_DEV static inline
#include "../digital_earth_amd/csrc/videoframe_kernels.hip"
#include "../digital_earth_amd/csrc/jpeg_kernels.hip"

static std::vector<uint8_t> run(const std::vector<float>& image, int W, int H, int quality, int restart, uint32_t* status) {
    const JpegGeometry g = jp_geometry(W, H, restart);
    // the planes, exactly as de_display.h's jp_launch asks for them
    std::vector<uint8_t> planes((size_t)W * H / 2 * 3, 0xA5);
    VideoArgs v;
    v.image = image.data(); v.out = planes.data(); v.W = W; v.H = H; v.format = 1; v.siting = 1; v.mode = 1; v.seed = 0; v.phase = 0;
    v.k = vd_make_consts(1, 1, 1);
    for (int by = 0; by < (H + PACK_TILE - 1) / PACK_TILE; ++by)
        for (int bx = 0; bx < (W + PACK_TILE - 1) / PACK_TILE; ++bx) {
            std::vector<VideoTile> lds(1);
            for (int t = 0; t < 256; ++t) vd_stage_tile(v, lds[0], t, bx, by);
            for (int t = 0; t < 256; ++t) vd_chroma_tile(v, lds[0], t, bx, by);
            for (int t = 0; t < 256; ++t) vd_store_tile(v, lds[0], t, bx, by);
        }
    JpegTables tab;
    jp_make_tables(quality, &tab);
    std::vector<int16_t> coef(g.blocks * 64, 0x5A5A);
    std::vector<unsigned long long> mask(g.blocks, ~0ull);
    std::vector<uint32_t> slots(g.intervals * g.slot_bytes / 4, 0xA5A5A5A5u);
    std::vector<uint32_t> words(2 * g.intervals + 4, 0xA5A5A5A5u);
    std::vector<uint32_t> out((CS_WORD_BYTES + g.capacity + 15) / 16 * 4, 0xA5A5A5A5u);
    JpegArgs a;
    a.planes = planes.data(); a.tab = &tab; a.coef = coef.data(); a.mask = mask.data(); a.slots = (uint8_t*)slots.data();
    a.len = words.data(); a.offset = words.data() + g.intervals; a.status = words.data() + 2 * g.intervals; a.out = (uint8_t*)out.data();
    a.W = W; a.H = H; a.mcus_x = g.mcus_x; a.restart = g.restart;
    a.blocks = (uint32_t)g.blocks; a.mcus = (uint32_t)g.mcus; a.count = (uint32_t)g.intervals; a.slot_bytes = (uint32_t)g.slot_bytes;
    a.front = JP_FRAMING_BYTES; a.extra = 2u; a.trailer = 0u; a.capacity = (uint32_t)g.capacity;
    if (jp_write_framing(tab, W, H, restart, a.out + CS_WORD_BYTES) != JP_FRAMING_BYTES) { fprintf(stderr, "the framing is not JP_FRAMING_BYTES long\n"); exit(1); }
    for (uint32_t wg = 0; wg < (a.blocks + JP_WG_BLOCKS - 1) / JP_WG_BLOCKS; ++wg) {
        std::vector<JpegTile> lds(1);
        memset(&lds[0], 0xA5, sizeof(JpegTile));
        for (int t = 0; t < 256; ++t) jp_stage(a, lds[0], t, wg);
        for (int t = 0; t < 256; ++t) jp_rows(a, lds[0], t, wg);
        for (int t = 0; t < 256; ++t) jp_columns(a, lds[0], t, wg);
        for (int t = 0; t < 256; ++t) jp_store(a, lds[0], t, wg);
        for (int t = 0; t < 256; ++t) jp_mask(a, lds[0], t, wg);
    }
    for (uint32_t i = 0; i < (a.count + 63) / 64 * 64; ++i) jp_encode_interval(a, i);
    std::vector<uint32_t> sums(CS_SCAN_THREADS, 0xA5A5A5A5u);
    for (int t = 0; t < CS_SCAN_THREADS; ++t) cs_scan_sum(a, sums.data(), t);
    for (int t = 0; t < CS_SCAN_THREADS; ++t) cs_scan_total(a, sums.data(), t);
    for (int t = 0; t < CS_SCAN_THREADS; ++t) cs_scan_offsets(a, sums.data(), t);
    for (uint32_t i = 0; i < a.count; ++i)
        for (int t = 0; t < 256; ++t)
            if (cs_compact(a, i, t, 256) && t == 0) jp_marker(a, i);
    uint64_t len;
    memcpy(&len, out.data(), 8);
    *status = out[2];
    if (len > g.capacity) { fprintf(stderr, "the length passes the capacity\n"); exit(1); }
    const uint8_t* s = (const uint8_t*)out.data() + CS_WORD_BYTES;
    return std::vector<uint8_t>(s, s + len);
}

int main(int argc, char** argv) {
    uint32_t status = 0;
    if (argc == 3) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        int32_t head[4];
        if (fread(head, 4, 4, f) != 4 || head[0] <= 0 || head[1] <= 0 || (head[0] & 1) || (head[1] & 1)) return 2;
        std::vector<float> image((size_t)head[0] * head[1] * 3);
        if (fread(image.data(), 4, image.size(), f) != image.size()) return 2;
        fclose(f);
        const std::vector<uint8_t> s = run(image, head[0], head[1], head[2], head[3], &status);
        if (status) { fprintf(stderr, "status %u\n", status); return 1; }
        f = fopen(argv[2], "wb");
        if (!f) return 2;
        fwrite(s.data(), 1, s.size(), f);
        fclose(f);
        return 0;
    }
    if (argc != 1) return 2;
    static const int sizes[][2] = {{2, 2}, {16, 16}, {34, 18}, {48, 40}, {160, 16}, {64, 32}, {208, 120}};
    static const int qualities[] = {1, 50, 90, 100}, restarts[] = {1, 3, 8, 65535};
    // More than CS_SCAN_THREADS intervals, where a thread of the scan owns two of them (528 x 528: 1089 intervals, the last owner has one, 479 threads none)
    // or three (544 x 1040: 2210 intervals, the last owner has two).  Restart 1 and one quality only: the sweep stays about as long as it was.
    static const int large[][2] = {{528, 528}, {544, 1040}};
    struct Case { int W, H, quality, restart; };
    std::vector<Case> cases;
    for (const auto& sz : sizes)
        for (int quality : qualities)
            for (int restart : restarts) cases.push_back({sz[0], sz[1], quality, restart});
    for (const auto& sz : large) {
        const JpegGeometry g = jp_geometry(sz[0], sz[1], 1);
        const size_t chunk = (g.intervals + CS_SCAN_THREADS - 1) / CS_SCAN_THREADS;
        if (chunk < 2 || g.intervals % chunk == 0) { fprintf(stderr, "%d x %d: no ragged chunk of two intervals or more per thread\n", sz[0], sz[1]); return 1; }
        cases.push_back({sz[0], sz[1], 90, 1});
    }
    int runs = 0;
    for (const Case& c : cases)
        for (int kind = 0; kind < 3; ++kind) {
            std::vector<float> image((size_t)c.W * c.H * 3);
            uint32_t r = 99u + (uint32_t)runs;
            for (float& x : image) { r = r * 1664525u + 1013904223u; x = kind == 0 ? (float)(r >> 8) * (1.2f / 16777216.0f) - 0.1f : kind == 1 ? 0.0f : ((r >> 30) & 1 ? 1.0f : 0.0f); }
            if (kind == 0) { image[1] = NAN; image[3] = -0.0f; image[5] = INFINITY; }
            const std::vector<uint8_t> s = run(image, c.W, c.H, c.quality, c.restart, &status);
            if (status || s.size() < JP_FRAMING_BYTES + 3 || s[s.size() - 2] != 0xff || s[s.size() - 1] != 0xd9) {
                fprintf(stderr, "%d x %d quality %d restart %d kind %d: status %u, %zu bytes, no EOI at the end\n", c.W, c.H, c.quality, c.restart, kind, status, s.size());
                return 1;
            }
            ++runs;
        }
    printf("jpeg_host_check: %d conversions, every stream ends in EOI within its capacity, no sanitizer report\n", runs);
    return 0;
}

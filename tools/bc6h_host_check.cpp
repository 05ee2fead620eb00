// bc6h_host_check.cpp — the BC6H encoder's body (csrc/bc6h_body.h, csrc/bc6h_tables.h; include/digital_earth_ibl_bc6h.h) replayed on the
// CPU, thread by thread in both kernels' launch shapes, on heap blocks of EXACTLY the sizes the library allocates, so that the address sanitizer sees
// any texel load or block store outside its buffer and the undefined-behaviour sanitizer any bad shift, cast or index.  A stand-alone program, no GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/bc6h_host_check.cpp -o bc6h_host_check && ./bc6h_host_check
// It also prints the tables (every mode's layout bit by bit, the partitions, the anchors) for tests/test_ibl_bc6h_abi.py to hold against
// digital_earth_amd/bc6h.py's, and checks what needs no device: black and 0x7BFF survive the quantiser at every precision, the file's front.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define DE_DEV static inline
#include "../digital_earth_amd/csrc/bc6h_body.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the launch over `images` images of `faces` faces: exact-size heap blocks in, exact-size heap blocks out, both launch shapes; the two qualities'
// blocks are left in q0 and q1
static void launch(const std::vector<int>& w, const std::vector<int>& h, int faces, uint32_t seed, std::vector<uint8_t>* q0, std::vector<uint8_t>* q1) {
    Bc6hArgs a;
    memset(&a, 0, sizeof a);
    std::vector<float*> heaps;
    a.images = (uint32_t)w.size();
    for (size_t m = 0; m < w.size(); ++m) {
        const size_t floats = (size_t)faces * (size_t)w[m] * (size_t)h[m] * 3;
        float* p = (float*)malloc(floats * sizeof(float));
        for (size_t k = 0; k < floats; ++k) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t pick = seed >> 28;
            p[k] = pick == 0 ? NAN : pick == 1 ? INFINITY : pick == 2 ? -INFINITY : pick == 3 ? -1.5f : pick == 4 ? 7e4f : pick == 5 ? 0.0f : (float)(seed >> 8 & 0xFFFF) * (pick < 10 ? 1e-4f : 1e-2f);
        }
        heaps.push_back(p);
        a.src[m] = p; a.w[m] = (uint32_t)w[m]; a.h[m] = (uint32_t)h[m];
        a.first[m + 1] = a.first[m] + (uint32_t)((w[m] + 3) / 4) * (uint32_t)((h[m] + 3) / 4);
    }
    a.per_face = a.first[a.images];
    a.total = a.per_face * (uint32_t)faces;
    for (int quality = 0; quality < 2; ++quality) {
        uint8_t* out = (uint8_t*)malloc((size_t)a.total * 16);
        memset(out, 0xA5, (size_t)a.total * 16);
        a.out = out;
        const uint32_t per_group = quality ? BC6H_Q1_GROUP_BLOCKS : BC6H_Q0_GROUP_BLOCKS, groups = (a.total + per_group - 1) / per_group;
        for (uint32_t g = 0; g < groups; ++g) {
            if (quality == 0) {
                for (uint32_t t = 0; t < BC6H_THREADS; ++t) {
                    const uint32_t b = g * BC6H_Q0_GROUP_BLOCKS + t;
                    if (b >= a.total) continue;
                    uint32_t rg[16], bb[16], words[4];
                    bc6h_load_block(a, b, rg, bb);
                    bc6h_encode_q0(rg, bb, words);
                    memcpy(out + (size_t)b * 16, words, 16);
                }
            } else {
                for (uint32_t half = 0; half < BC6H_Q1_GROUP_BLOCKS; ++half) {
                    const uint32_t b = g * BC6H_Q1_GROUP_BLOCKS + half, at = b < a.total ? b : a.total - 1u;
                    uint64_t best_err = ~0ull; uint32_t best_order = ~0u, best_words[4] = {0, 0, 0, 0};
                    for (uint32_t lane = 0; lane < BC6H_Q1_LANES; ++lane) {
                        uint32_t rg[16], bb[16], words[4], order; uint64_t err;
                        bc6h_load_block(a, at, rg, bb);
                        bc6h_lane_q1(rg, bb, lane, &err, &order, words);
                        if (err < best_err || (err == best_err && order < best_order)) { best_err = err; best_order = order; memcpy(best_words, words, 16); }
                    }
                    if (b < a.total) memcpy(out + (size_t)b * 16, best_words, 16);
                }
            }
        }
        std::vector<uint8_t>* keep = quality ? q1 : q0;
        keep->assign(out, out + (size_t)a.total * 16);
        free(out);
    }
    for (float* p : heaps) free(p);
    printf("launch of %u images x %d faces: %u blocks\n", a.images, faces, a.total);
}

static const char* const FIELD[13] = {"RW", "GW", "BW", "RX", "GX", "BX", "RY", "GY", "BY", "RZ", "GZ", "BZ", "D"};

int main() {
    // the tables, for the test to compare
    for (int m = 1; m <= 14; ++m) {
        const Bc6hMode& d = BC6H_MODE[m - 1];
        printf("mode %d value %d count %d precision %d delta %d %d %d regions %d layout", m, d.value, d.count, d.precision, d.delta[0], d.delta[1], d.delta[2], d.regions);
        int bits = d.count;
        for (int k = 0; k < BC6H_LAYOUT_RUNS && BC6H_LAYOUT[m - 1][k]; ++k) {
            const uint32_t run = BC6H_LAYOUT[m - 1][k], field = run & 15u, low = (run >> 4) & 15u, count = (run >> 8) & 15u;
            CHECK(field <= 12u, "mode %d run %d: field %u", m, k, field);
            for (uint32_t b = 0; b < count; ++b, ++bits) printf(" %s%u", FIELD[field], (run & 0x1000u) ? low + count - 1 - b : low + b);
        }
        printf("\n");
        CHECK(bits == (d.regions == 2 ? 82 : 65), "mode %d: %d bits in front of the indices", m, bits);
    }
    for (int k = 0; k < 32; ++k) {
        printf("partition %d anchor %d regions ", k, BC6H_ANCHOR[k]);
        for (int t = 0; t < 16; ++t) printf("%d", (BC6H_PARTITION[k] >> t) & 1);
        printf("\n");
        CHECK(!(BC6H_PARTITION[k] & 1) && ((BC6H_PARTITION[k] >> BC6H_ANCHOR[k]) & 1), "partition %d: texel 0 in region 0, the anchor in region 1", k);
    }
    // black and 0x7BFF come back exactly at every precision the encoder uses
    for (uint32_t p : {6u, 7u, 9u, 10u}) {
        CHECK(bc6h_decoded(bc6h_unquantise(bc6h_quantise(0u, p), p), bc6h_unquantise(bc6h_quantise(0u, p), p), 27u) == 0u, "black at %u bits", p);
        const uint32_t top = bc6h_unquantise(bc6h_quantise(BC6H_HALF_MAX, p), p);
        CHECK(top == 0xFFFFu && bc6h_decoded(top, top, 27u) == BC6H_HALF_MAX, "0x7BFF at %u bits", p);
    }
    CHECK(bc6h_half(-1.0f) == 0u && bc6h_half(NAN) == 0u && bc6h_half(INFINITY) == BC6H_HALF_MAX && bc6h_half(7e4f) == BC6H_HALF_MAX && bc6h_half(-INFINITY) == 0u && bc6h_half(1.0f) == 0x3C00u, "texel to half");
    // both launch shapes: lone images of awkward sizes, one past a workgroup's share in each shape, and chains down to edge 1
    std::vector<uint8_t> q0, q1;
    const int shapes[6][2] = {{4, 4}, {8, 8}, {5, 7}, {1, 1}, {2, 2}, {132, 36}};
    for (const auto& s : shapes) launch({s[0]}, {s[1]}, 1, 99u + (uint32_t)s[0], &q0, &q1);
    launch({8, 4, 2, 1}, {8, 4, 2, 1}, 6, 7u, &q0, &q1);
    CHECK(q0.size() == bc6h_payload_bytes(8, 4) && q0.size() == 6u * 7u * 16u, "the payload of E = 8, L = 4");
    launch({32, 16, 8}, {32, 16, 8}, 6, 8u, &q0, &q1);
    CHECK(q1.size() == bc6h_payload_bytes(32, 3), "the payload of E = 32, L = 3");
    for (size_t k = 0; k < q0.size(); k += 16) CHECK((q0[k] & 31) == 3, "quality 0 emits mode 11 alone (block %zu)", k / 16);
    // a constant block of 0x7BFF: mode 11 with both ends all ones and every index 0, at both qualities
    {
        float* p = (float*)malloc(16 * 3 * sizeof(float));
        for (int k = 0; k < 48; ++k) p[k] = INFINITY;
        Bc6hArgs a; memset(&a, 0, sizeof a);
        a.src[0] = p; a.w[0] = a.h[0] = 4; a.images = 1; a.first[1] = 1; a.per_face = 1; a.total = 1;
        uint32_t rg[16], bb[16], words[4], order; uint64_t err;
        bc6h_load_block(a, 0, rg, bb);
        bc6h_encode_q0(rg, bb, words);
        CHECK(words[0] == 0xFFFFFFE3u && words[1] == 0xFFFFFFFFu && words[2] == 1u && words[3] == 0u, "the block of +Inf: %08x %08x %08x %08x", words[0], words[1], words[2], words[3]);
        bc6h_lane_q1(rg, bb, 0, &err, &order, words);
        CHECK(err == 0 && order == 0 && words[0] == 0xFFFFFFE3u, "ties go to mode 11");
        free(p);
    }
    CHECK(bc6h_settings_fault(0, 0) == nullptr && bc6h_settings_fault(1, 1) == nullptr && bc6h_settings_fault(2, 0) && bc6h_settings_fault(1, 2) && bc6h_settings_fault(1, -1), "the settings");
    uint8_t* front = (uint8_t*)malloc(IBL_DDS_HEADER);
    bc6h_dds_header(256, 6, front);
    uint32_t w[37];
    memcpy(w, front, sizeof w);
    CHECK(memcmp(front, "DDS ", 4) == 0 && w[1] == 124 && w[2] == 0x000A1007u && w[3] == 256 && w[4] == 256 && w[5] == 65536 && w[7] == 6 && w[32] == 95 && w[33] == 3 && w[34] == 4 && w[35] == 1, "the DDS front");
    free(front);
    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("bc6h bodies: every thread replayed, no sanitizer report\n");
    return 0;
}

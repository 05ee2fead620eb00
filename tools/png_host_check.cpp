// png_host_check.cpp — the host side of the PNG output (csrc/png_tables.h) as a stand-alone program, so that the address and
// undefined-behaviour sanitizers can watch every index it forms: the table builder (the CRC-32 byte table, the shift-by-2^k-bytes operators, deflate's
// length codes), the capacity arithmetic and the front of the file.  No GPU, no library.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_host_check.cpp -o png_host_check && ./png_host_check
// Checks, each against an independent statement: the CRC of "123456789" is 0xCBF43926; shifting a register by n zero bytes with the operators equals
// feeding n zero bytes through the byte table, for every n that sets one or several bits below 2^17; a CRC computed in pieces and combined the way
// the deflate kernel combines them equals the CRC computed in one go; Adler partials joined (png_adler_join) chunk by chunk and in the scan kernel's two
// levels equal the serial Adler-32; every match length 3 ... 258 lies in its code's range; the capacity is
// front + N + 24 per chunk + 28 and every slot holds a stored chunk with its overhead; the front has 33 or 49 bytes and its chunks' CRCs verify.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../digital_earth_amd/csrc/png_tables.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static uint32_t feed(const PngTables& t, uint32_t r, const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) r = t.crc[(r ^ p[i]) & 0xffu] ^ (r >> 8);
    return r;
}
static uint32_t shift_by(const PngTables& t, uint32_t r, uint32_t bytes) {      // as the deflate kernel does
    for (int m = 0; m < PNG_SHIFT_OPS; ++m)
        if ((bytes >> m) & 1u) r = png_gf2_times(t.shift[m], r);
    return r;
}

int main() {
    std::vector<PngTables> heap(1);      // on the heap: one index past a table is the sanitizer's to find
    PngTables& t = heap[0];
    png_make_tables(&t);
    CHECK(png_crc(t, (const uint8_t*)"123456789", 9) == 0xCBF43926u, "the CRC-32 check value");

    // the shift operators against zero bytes fed through the byte table
    std::vector<uint8_t> zeros(1u << 17, 0);
    const uint32_t regs[4] = {0xffffffffu, 1u, 0x80000000u, 0xdeadbeefu};
    const uint32_t counts[] = {0, 1, 2, 3, 4, 255, 256, 1023, 1024, 4097, 65535, 65536, 65559, 131071};
    for (uint32_t r : regs)
        for (uint32_t n : counts) CHECK(shift_by(t, r, n) == feed(t, r, zeros.data(), n), "shift by %u zero bytes of %08x", n, r);

    // a CRC in pieces, combined: register 0xFFFFFFFF in front of the first piece, 0 in front of the others
    std::vector<uint8_t> data(65559);
    uint32_t lcg = 12345u;
    for (uint8_t& b : data) { lcg = lcg * 1664525u + 1013904223u; b = (uint8_t)(lcg >> 24); }
    for (size_t total : {(size_t)4, (size_t)5, (size_t)511, (size_t)512, (size_t)513, (size_t)16400, data.size()}) {
        const size_t threads = 512, piece = (total + threads - 1) / threads;
        uint32_t combined = 0;
        for (size_t k = 0; k < threads; ++k) {
            const size_t p0 = k * piece, p1 = p0 + piece < total ? p0 + piece : total;
            if (p0 >= total) continue;
            combined ^= shift_by(t, feed(t, k == 0 ? 0xffffffffu : 0u, data.data() + p0, p1 - p0), (uint32_t)(total - p1));
        }
        CHECK((combined ^ 0xffffffffu) == png_crc(t, data.data(), total), "the CRC of %zu bytes in pieces", total);
    }

    // the Adler join: the chunks' partials taken from (0, 0) as the deflate kernel takes them, joined one by one from (1, 0), and joined in two levels
    // as the scan kernel does (a run of chunks per thread from (0, 0), then the 1024 threads' states from (1, 0)), against the serial Adler-32
    {
        std::vector<uint8_t> bytes(2500u * 1024u + 77u);      // at 1024 per chunk: 2501 chunks, three per thread of the scan, the last owner has two
        for (uint8_t& b : bytes) { lcg = lcg * 1664525u + 1013904223u; b = (lcg >> 28) == 0u ? 0xffu : (uint8_t)(lcg >> 16); }
        uint32_t sa = 1u, sb = 0u;
        for (uint8_t b : bytes) { sa = (sa + b) % PNG_ADLER; sb = (sb + sa) % PNG_ADLER; }
        for (size_t chunk : {(size_t)1024, (size_t)16384, (size_t)65535}) {
            const size_t chunks = (bytes.size() + chunk - 1) / chunk, threads = 1024, run = (chunks + threads - 1) / threads;
            std::vector<uint32_t> pa(chunks), pb(chunks), pn(chunks);
            for (size_t k = 0; k < chunks; ++k) {
                const size_t base = k * chunk, n = bytes.size() - base < chunk ? bytes.size() - base : chunk;
                unsigned long long a = 0, b = 0;
                for (size_t i = 0; i < n; ++i) { a += bytes[base + i]; b += (unsigned long long)(n - i) * bytes[base + i]; }
                pa[k] = (uint32_t)(a % PNG_ADLER); pb[k] = (uint32_t)(b % PNG_ADLER); pn[k] = (uint32_t)n;
            }
            unsigned long long A = 1, B = 0;
            for (size_t k = 0; k < chunks; ++k) png_adler_join(&A, &B, pn[k], pa[k], pb[k]);
            CHECK(A == sa && B == sb, "the Adler-32 of chunks of %zu joined one by one", chunk);
            A = 1; B = 0;
            for (size_t t = 0; t < threads; ++t) {
                unsigned long long ta = 0, tb = 0, tn = 0;
                for (size_t k = t * run; k < (t + 1) * run && k < chunks; ++k) { png_adler_join(&ta, &tb, pn[k], pa[k], pb[k]); tn += pn[k]; }
                png_adler_join(&A, &B, tn, (uint32_t)ta, (uint32_t)tb);
            }
            CHECK(A == sa && B == sb, "the Adler-32 of chunks of %zu joined in the scan's groups of %zu", chunk, run);
        }
    }

    // deflate's length codes
    for (int L = 3; L <= 258; ++L) {
        const int i = t.len_code[L - 3];
        CHECK(i >= 0 && i < 29 && t.len_base[i] <= L && L - t.len_base[i] < (1 << t.len_extra[i]) && (i == 28) == (L == 258), "the code of length %d", L);
    }

    // geometry and the front
    const int shapes[][4] = {{1, 1, 3, 8}, {7, 5, 3, 8}, {7, 5, 4, 8}, {33, 17, 3, 16}, {1920, 1080, 3, 8}, {1920, 1080, 4, 8}, {1920, 1080, 3, 16}, {4727, 4727, 3, 16}};
    for (const auto& s : shapes)
        for (int chunk : {1024, 4096, 16384, 65535}) {
            const PngGeometry g = png_geometry(s[0], s[1], s[2], s[3], chunk);
            CHECK(g.filtered == (size_t)s[1] * (1 + (size_t)s[0] * s[2] * s[3] / 8) && g.filtered <= PNG_MAX_FILTERED, "N of %d x %d", s[0], s[1]);
            CHECK(g.chunks == (g.filtered + chunk - 1) / chunk && (g.chunks - 1) * (size_t)chunk < g.filtered, "the chunks of %d x %d", s[0], s[1]);
            CHECK(g.slot_bytes % 16 == 0 && g.slot_bytes >= (size_t)chunk + PNG_CHUNK_OVERHEAD && g.slot_bytes <= 65535 + PNG_CHUNK_OVERHEAD + 15, "the slot at %d", chunk);
            CHECK(g.capacity == g.front + g.filtered + PNG_CHUNK_OVERHEAD * g.chunks + PNG_TRAILER_BYTES && g.capacity < (1ull << 32), "the capacity");
            std::vector<uint8_t> front(PNG_FRONT_MAX, 0xA5);
            const uint8_t cicp[4] = {9, 16, 0, 1};
            const size_t n = png_write_front(t, g, cicp, front.data());
            CHECK(n == g.front && n == (s[3] == 16 ? 49u : 33u), "the front's length");
            CHECK(front[n] == 0xA5, "nothing written behind the front");
            size_t at = 8;
            while (at < n) {
                const uint32_t len = (uint32_t)front[at] << 24 | (uint32_t)front[at + 1] << 16 | (uint32_t)front[at + 2] << 8 | front[at + 3];
                const uint8_t* c = front.data() + at + 8 + len;
                CHECK(at + 12 + len <= n && png_crc(t, front.data() + at + 4, 4 + len) == ((uint32_t)c[0] << 24 | (uint32_t)c[1] << 16 | (uint32_t)c[2] << 8 | c[3]), "a front chunk's CRC");
                at += 12 + len;
            }
            CHECK(at == n, "the front's chunks end at its length");
        }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("png_host_check: tables, CRC combination, Adler join, length codes, geometry and front are clean\n");
    return 0;
}

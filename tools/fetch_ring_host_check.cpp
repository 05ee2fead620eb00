// fetch_ring_host_check.cpp — the ring arithmetic of the lagged fetches (the top of csrc/de_fetch.h: plain integers, no HIP) compiled for the HOST under
// the address and undefined-behaviour sanitizers (tests/test_fetch_ring_host.py builds and runs this).
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fetch_ring_host_check.cpp -o fetch_ring_host_check
// A model ring of DEPTH cells walks 2^32 + 9 begins and as many ends: the counters are SET to UINT_MAX - 4 (they are 32-bit and wrap, which is what the
// walk is about) and then driven through every legal interleaving of begins and ends of 14 steps — from each of the depths 0 .. 4 in flight, a begin
// wherever fewer than four are in flight, an end wherever one is — so that every interleaving crosses the wrap somewhere else.  The walk from 0 to
// UINT_MAX - 4 itself is the same congruence: 2^32 is a multiple of the depth.  Checked at every step:
//   * a begin is refused exactly when four are in flight, an end exactly when none is, and in_flight is the model's count;
//   * the cell a begin fills is the one after the cell the previous begin filled, cyclically, and so for the ends: both visit 0, 1, 2, 3, 0, ..;
//   * the cell a begin fills holds no fetch in flight, and the n-th end hands out the cell, and the fetch, of the n-th begin.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define DE_FETCH_STANDALONE
#include "../digital_earth_amd/csrc/de_fetch.h"

static const unsigned DEPTH = 4;      // DE_FETCH_RING (csrc/de_context.h)

struct Model {
    unsigned begun, ended;             // the library's counters
    uint64_t begun64, ended64;         // the same calls, counted without a wrap
    uint64_t cell[DEPTH];              // the number of the fetch each cell holds; 0: none in flight
    int last_begin, last_end;          // the cells the previous begin and end used
};

static void die(const char* what, const Model& m) {
    fprintf(stderr, "fetch ring: %s (begun %u, ended %u, calls %llu / %llu)\n", what, m.begun, m.ended, (unsigned long long)m.begun64, (unsigned long long)m.ended64);
    exit(1);
}

static bool begin(Model& m) {
    const uint64_t deep = m.begun64 - m.ended64;
    if (ring_in_flight(m.begun, m.ended) != deep) die("in_flight differs from the model's count", m);
    if (ring_full(m.begun, m.ended, DEPTH) != (deep >= DEPTH)) die("begin refused, or not, at the wrong depth", m);
    if (deep >= DEPTH) return false;
    const int k = ring_cell(m.begun, DEPTH);
    if (k < 0 || k >= (int)DEPTH) die("begin: cell out of range", m);
    if (k != (m.last_begin + 1) % (int)DEPTH) die("begin left the order of the cells", m);
    if (m.cell[k] != 0) die("begin fills a cell whose fetch is in flight", m);
    m.cell[k] = ++m.begun64;
    m.begun++; m.last_begin = k;
    return true;
}

static bool end(Model& m) {
    if (ring_empty(m.begun, m.ended) != (m.begun64 == m.ended64)) die("end refused, or not, at the wrong depth", m);
    if (m.begun64 == m.ended64) return false;
    const int k = ring_cell(m.ended, DEPTH);
    if (k < 0 || k >= (int)DEPTH) die("end: cell out of range", m);
    if (k != (m.last_end + 1) % (int)DEPTH) die("end left the order of the cells", m);
    if (m.cell[k] != m.ended64 + 1) die("end hands out another fetch than the oldest in flight", m);
    m.cell[k] = 0;
    m.ended64++; m.ended++; m.last_end = k;
    return true;
}

static unsigned long long g_paths = 0;

// every legal continuation of `steps` more calls; the refused call is tried too, once per state, and must leave the ring as it was
static void walk(Model m, int steps) {
    if (steps == 0) { ++g_paths; return; }
    { Model b = m; if (begin(b)) walk(b, steps - 1); }
    { Model e = m; if (end(e)) walk(e, steps - 1); }
}

int main() {
    static_assert(UINT_MAX == 0xffffffffu, "the counters are 32 bits wide");
    for (unsigned deep = 0; deep <= DEPTH; ++deep) {
        // 2^32 - 5 begins lie behind, `deep` of them in flight: the 14 steps below take the begins to at most 2^32 + 9 calls
        Model m;
        m.begun = UINT_MAX - 4u; m.ended = m.begun - deep;
        m.begun64 = (uint64_t)m.begun; m.ended64 = m.begun64 - deep;
        for (unsigned k = 0; k < DEPTH; ++k) m.cell[k] = 0;
        for (uint64_t n = m.ended64 + 1; n <= m.begun64; ++n) m.cell[(n - 1) % DEPTH] = n;      // fetch n lies in cell (n - 1) mod 4: the first begin filled cell 0
        m.last_begin = (int)((m.begun64 + DEPTH - 1) % DEPTH);
        m.last_end = (int)((m.ended64 + DEPTH - 1) % DEPTH);
        walk(m, 14);
    }
    printf("fetch_ring_host_check: %llu interleavings across the wrap of the counters, cells in order, never more than %u in flight, no sanitizer report\n", g_paths, DEPTH);
    return 0;
}

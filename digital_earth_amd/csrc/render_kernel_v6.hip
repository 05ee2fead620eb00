// render_kernel_v6.hip — path_tracer (pathtracer.py:316-469) as ONE PERSISTENT KERNEL whose stage queues live in LDS: one stage
// scheduler per workgroup (two workgroups of twelve waves per CU).
//
// Why.  render_kernel_v5 showed that the seven stage bodies of render_kernel_v3 can run inside one launch with coherent waves (lane
// utilisation 0.67) — and that handing 64-byte records from wave to wave through HBM chunks and device-wide rings costs what the
// coherence wins: every hop is a write-through, a ticket on a contended control word and a cold L2 read, and four single-class
// waves per SIMD cannot cover those latencies.  Here a path never leaves the CU that started it.  A workgroup owns DE_V6_P record
// slots in LDS (its half of the CU's 160 KB); a path keeps ONE slot from its first ray to its contribution, and what travels between
// the stages is the 16-bit slot number, through eight small rings (seven stages + the free slots) that also live in LDS.  A wave
// asks the scheduler for the fullest ring, claims up to 64 slot numbers with one LDS compare-and-swap, runs the stage body — the
// loop stages with persistent lanes that refill from the ring, as in v3 / v5 — writes the records back in place and appends the
// slot numbers to the rings of the next stages.  No HBM queue traffic at all: the only global memory the scheduler touches is the
// work counter (one fetch-add per 256 new paths), the paths' cold records (64 bytes per SLOT: 37 MB for the whole GPU, L2 / MALL
// resident) and the contribution of a path when it ends.
//
// Results are IDENTICAL to render_kernel_v2 / _v3 / _v5 / the CPU oracle: every path runs the same arithmetic in the same order on
// its own RNG stream; only where and when changes.
//
// Visibility.  All waves of a workgroup share the CU's LDS and its L1: LDS operations of a wave execute in order, a record is
// written (ds_write) before its slot number is (after a workgroup-scope release fence, which also drains the cold-record stores to
// the L1/L2 both waves use); a ring entry is taken only after it has been seen non-empty (acquire).  A producer takes a ticket
// (fetch-add on the ring's tail) and then stores the entries; the consumer that claimed a ticket early waits for the entry — a few
// LDS round trips.  Every wait is bounded: a wave that waits too long raises the abort word and the host reports DE_ERR_HIP.
//
// What makes it fast (profiles/experiments/README.md): (1) YIELD — a loop-stage wave whose ring is dry and that is left
// with few busy lanes suspends its records (the loop's state travels in the record and in spare words of the cold record, bit for bit) and
// hands them back to its own ring, where they fill the idle lanes of another wave; (2) every stage is a separate, non-inlined device
// function: 76-80 VGPRs each instead of 128 + spills for the seven inlined, so six waves per SIMD fit; (3) 56-byte records: the LDS holds
// 1.46 record slots per lane at that occupancy, and slots per lane is what bounds the design; (4) THE TAIL (round 5, see "The tail" below):
// a launch with another one queued behind it does not keep half a CU's LDS for its last handful of paths — a workgroup exports them to a
// pool in HBM and exits, and a 64-workgroup launch of this same kernel (TAIL = true) finishes them.
#include "de_stages.h"

namespace bs {

using wf::Path;
using wf::NQ;
using wf::Q_ST; using wf::Q_GAS; using wf::Q_CLOUD; using wf::Q_EVENT; using wf::Q_SURF; using wf::Q_SCFIN; using wf::Q_SURFFIN;

enum { Q_FREE = NQ, NR = NQ + 1, Q_PRIMARY = NQ + 1, Q_EXIT = NQ + 2, Q_EXPORT = NQ + 3 };
// Geometry.  The stage functions are separate (non-inlined) device functions: each gets the registers ITS body needs (36 ... 78, as the
// stage kernels of render_kernel_v3.hip) instead of the 128 + spills the register allocator gives the seven stages inlined into one
// function, so the kernel fits 80 VGPRs = 6 waves per SIMD.  24 waves per CU = two workgroups of twelve waves, 80 KB of LDS each.
// (One workgroup of sixteen waves with 1984 slots at 128 VGPRs: 138 ms per frame; twelve of those waves: 177 ms — the kernel is bound by
// VALU issue and latency hiding, both of which are waves per SIMD.)
#ifndef DE_V6_WAVES
#define DE_V6_WAVES 12                     // waves per workgroup
#endif
#ifndef DE_V6_WG_PER_CU
#define DE_V6_WG_PER_CU 2
#endif
#ifndef DE_V6_WPE
#define DE_V6_WPE 6                        // waves per SIMD the kernel is compiled for (DE_V6_WAVES x DE_V6_WG_PER_CU / 4)
#endif
#ifndef DE_V6_P
#define DE_V6_P 1120u                      // record slots per workgroup, 56 B each (61 KB): with the rings and the rest the 80 KB a workgroup can have (1008 slots of 64 B: +5.6 % time; 960: +7 %; 768: +19 %)
#endif
#ifndef DE_V6_CAP
#define DE_V6_CAP 1128u                    // entries per ring (> DE_V6_P: a ring can hold every slot number); indices are taken modulo this
#endif
// A ring cell is 16 bits: bits 11-15 = lap (index / DE_V6_CAP, modulo 32), bits 0-10 = a slot number, or all ones when the cell is EMPTY and
// waits for the entry of that lap.  Ticket i may only be STORED into a cell that reads "empty, lap(i)" and only be TAKEN from a cell that reads
// "slot, lap(i)"; the take leaves "empty, lap(i) + 1".  So a cell's states form one chain — empty(0), full(0), empty(1), full(1), ... — and every
// transition has exactly ONE writer (tickets are unique: one fetch-add per push, one compare-and-swap per claim), whatever the waves' relative
// speeds: a producer a whole lap ahead of a stalled consumer waits for that consumer's take instead of overwriting its entry, a consumer a lap
// ahead waits for its own producer instead of taking the stalled one's entry.  Thirty-two laps cannot be open at one cell: each open lap holds a
// different wave in a bounded wait (a wave's tickets of one push / claim are consecutive, fewer than DE_V6_CAP: one per cell), and a workgroup
// has DE_V6_WAVES of them.  (Round 4's rings relied on "at most DE_V6_P slot numbers exist for DE_V6_CAP cells", which bounds what is QUEUED,
// not what a stalled wave has claimed and not yet taken — a ring that was full at the claim needs DE_V6_CAP - DE_V6_P = 8 further entries to come
// round to that cell: an argument about time, VERDICT r4 weak #7.)  Cost: five vector instructions per entry on either side.
#define DE_V6_EMPTY 0xffffu                // take()'s "timed out" value: never a slot number
#define DE_V6_SLOT_MASK 0x7ffu
static_assert(DE_V6_P < DE_V6_SLOT_MASK, "slot numbers take 11 bits of a ring cell; the all-ones pattern marks an empty cell");
static_assert(DE_V6_CAP >= DE_V6_P, "a ring must be able to hold every slot number");
static_assert(DE_V6_WAVES <= 31, "the lap tag of a ring cell has five bits: one open lap per blocked wave at most");
#define DE_V6_CTL_STRIDE 32u
// global control words (index x DE_V6_CTL_STRIDE dwords): 0 work counter, 8.. statistics (64-bit)
// 1-3 (64-bit, 100 MHz real-time counter; every build): the launch's first workgroup start, the first wave that found the work counter exhausted, the last wave's exit
// — the launch's DRAIN, the time its last paths take once nothing is left to start, is what separates a rank's 1/N share from 1/N of the frame (de_last_launch_phases)
// G_WORKX + x: the work counter of image band x (see run_primary: one band per XCD)
// G_DRAIN + k (STATS builds): the launch's drain in 0.25 ms buckets since G_T_EXHAUSTED — [k] paths alive in the workgroups that are still resident at the start of bucket k, [32 + k] those workgroups
enum { G_WORK = 0, G_T_START = 1, G_T_EXHAUSTED = 2, G_T_END = 3, G_STAT0 = 8, G_STAT2 = 8 + 64, G_WORKX = 8 + 64 + 64, G_DRAIN = 8 + 64 + 64 + 8, G_POOL = 8 + 64 + 64 + 8 + 64, G_WORDS = 8 + 64 + 64 + 8 + 64 + 8 };
// G_POOL + 2 l: entries written to the pool that launch level l exports to; G_POOL + 2 l + 1: entries of that pool handed out to level l + 1 (see "The tail" below)
// statistics: 0-7 records taken per stage (7 = new paths), 8-15 wave time per stage (100 MHz ticks; 15 = new paths), 16 idle rounds,
// 17 stage entries, 18 failed claims, 19 wave time in the scheduler, 20 yields of a loop stage, 21 records handed back by them, 22 wave time between the end of the work items and the wave's exit, 24-30 stage entries per stage (calls of the stage function), 32-38 trips of the loop stages / passes of the straight-line stages, 40-46 busy lanes summed over them,
// cloud stage's occupancy bound: 23 lane-steps that needed the exact density lookup, 31 trips in which none did, 39 lookups of the bound map
// region statistics (G_STAT2 + k; STATS builds only): where a wave's time goes and how many lanes the region's vector code runs for.  Per loop stage q
// (sphere trace, gas, cloud) fourteen words at 14 q: shader-clock ticks and ticks x active lanes of R_STEP (the stage's step(), lanes = busy), R_EPI (finish()
// + the record's write-back, lanes = finished), R_PUSH (release + ring appends), R_REFILL (claim, take, record load, begin() / restore(), lanes = refilled),
// R_YIELD (suspend + hand back), R_HEAD (the trip's own control: ballots, thresholds; no vector work: lanes 0), then [12] services, [13] trips.  Per
// straight-line stage q (event, surface, volume finish, surface finish) four words at 42 + 4 (q - 3): ticks and ticks x lanes of the body, ticks of the
// pass's ring work (claim, take, record load / store, appends), passes.  The same four for new paths (primary sphere trace included) at 58.
enum { R_STEP = 0, R_EPI, R_PUSH, R_REFILL, R_YIELD, R_HEAD, R_N };
enum { ST_RECS = 0, ST_CYC = 8, ST_IDLE = 16, ST_ENTRIES = 17, ST_CLAIMFAIL = 18, ST_SCHED = 19, ST_YIELD = 20, ST_YIELDED = 21, ST_DRAIN = 22, ST_CLOUD_EXACT = 23, ST_ENTRY_Q = 24, ST_CLOUD_NOEXACT = 31, ST_TRIPS = 32, ST_CLOUD_LOOKUPS = 39, ST_LANETRIPS = 40, ST_N = 48 };
enum { ERR_ENTRY_TIMEOUT = 1, ERR_CELL_BUSY_TIMEOUT = 2, ERR_IDLE_WATCHDOG = 3, ERR_POOL_FULL = 4 };
// cell values as the 16-bit stores truncate them (the lap's high bits fall off)
DE_DEV uint32_t cell_empty(uint32_t lap) { return (lap << 11) | DE_V6_SLOT_MASK; }
DE_DEV uint32_t cell_full(uint32_t lap, uint32_t slot) { return (lap << 11) | slot; }
// what a cell read as v holds FOR lap: a slot number (< DE_V6_SLOT_MASK), DE_V6_SLOT_MASK = empty and waiting for this lap's entry, anything larger = another lap
DE_DEV uint32_t cell_for(uint32_t v, uint32_t lap) { return (v ^ (lap << 11)) & 0xffffu; }

struct Args {
    const RenderArgs* ra;       // the launch's RenderArgs in device memory (written by v6_init_kernel)
    wf::Cold* cold;             // [workgroups x DE_V6_P] cold records, one per record slot
    uint32_t* ctl;              // G_WORDS x DE_V6_CTL_STRIDE dwords
    uint32_t* status;           // host-visible: [0] abort code (0 = clean)
    uint32_t n_items;
    uint32_t idle_limit;        // watchdog: scheduler rounds without work before a wave raises the abort word
    // tuning (de_api.hip: DE_V6_* environment)
    uint32_t svc[3];            // idle lanes at which a loop stage (sphere trace, gas, cloud) services: pushes finished records, refills ...
    uint32_t svc_area[3];       // ... or (> 0) the idle LANE-TRIPS since its last service at which it does: see run_loop
    uint32_t yield_max;         // a loop-stage wave whose ring is dry hands its records back when at most this many lanes are busy ...
    uint32_t elsewhere_min;     // ... and another ring (or the free slots, while paths are left to start) holds at least this many entries
    uint32_t retry;             // trips between two looks at a dry ring
    uint32_t enter_min;         // the scheduler prefers rings with at least this many entries (a loop stage entered with fewer runs part-filled)
    uint32_t flat_min;          // a straight-line stage is entered with fewer entries than this only when the loop stages' rings are empty (0: off; measured flat)
    uint32_t flat_again;        // a straight-line stage runs a FURTHER pass only when its ring holds at least this many entries (1: until the ring is dry)
    uint32_t bands;             // work counters: 8 = one band of the image per XCD (run_primary), 1 = one counter for the whole launch
    // the tail (see "The tail" below): this launch's level in the frame's chain, when its workgroups export, and the pools on either side
    uint32_t level;             // 0: the launch that starts the frame's paths; k > 0: the k-th tail launch — its "new paths" are what level k - 1 exported
    uint32_t export_at;         // > 0: a workgroup with nothing left to start and at most this many paths alive exports them to pool_out and exits
    uint4* pool_in; uint4* pool_out;
    uint32_t cap_in, cap_out;   // entries the pools hold
    const uint32_t* issued;     // host-visible: the number of the context's newest launch that has a successor on another stream — a workgroup only exports when this launch (seq) has one, see schedule()
    uint32_t seq;               // this launch's number in that count; 0xffffffff: export whether or not anything follows (tests, de_tuning.v6_tail_when_alone)
};
template <int... T> struct Targets {};

// The tail.  Once the work counter has run out a workgroup's population decays — BASELINE cfg2: 96 % of the slots 0.5 ms later, 50 % after 1.25 ms, 8 %
// after 2.25 ms — but its last path ends 3 ... 8 ms later (a 25-vertex cloud path is a chain of ~150 dependent stage passes), and until then the
// workgroup keeps half a CU's LDS for a handful of paths: 4.15 ms x 512 workgroup slots held per launch where 1.43 would do at full workgroups
// (profiles/r5_lanes: the drain table), a quarter of a rank's 1/8 share of a frame.  So a launch does not wait for its stragglers: a workgroup with
// nothing left to start and at most export_at paths alive has its loop stages hand their records back (the yield path: the loop's state is in the
// record and its cold record), copies every queued record — 56 bytes of LDS, the 64-byte cold record, the ring it waits in — to a pool in HBM and
// exits; the next launch of the chain (same stream: the pool is complete when it starts) has few workgroups whose "new paths" are the pool's
// entries, and may export in turn.  A path's arithmetic does not know where it runs: results are unchanged bit for bit.
struct Pool {
    uint4 *a, *b, *c, *cold; uint2* d; uint32_t* q;
    DE_DEV Pool(uint4* base, uint32_t cap) : a(base), b(base + cap), c(base + 2u * cap), cold(base + 3u * cap), d(reinterpret_cast<uint2*>(base + 7u * (size_t)cap)), q(reinterpret_cast<uint32_t*>(base + 7u * (size_t)cap) + 2u * (size_t)cap) {}
};
#define DE_V6_POOL_ENTRY_BYTES 124u        // 3 x 16 + 8 (the record) + 64 (its cold record) + 4 (its ring)

// what every stage function needs of the launch: written to LDS once per workgroup, read (wave-uniform) at each stage entry
struct Cfg {
    const RenderArgs* ra;
    const FrameConsts* fc;
    wf::Cold* cold;             // this workgroup's DE_V6_P cold records
    uint32_t* ctl;
    uint32_t* status;
    uint32_t n_items, idle_limit;
    uint32_t svc[3];
    uint32_t svc_area[3];
    uint32_t yield_max, elsewhere_min, retry, enter_min;
    uint32_t flat_min, flat_again;
    uint32_t bands, xcd;        // xcd: the XCD this workgroup runs on (HW_REG_XCC_ID)
    uint4* pool_in; uint4* pool_out;
    const uint32_t* issued;
    uint32_t level, export_at, cap_in, cap_out, seq, pad_;
};
static_assert(sizeof(Cfg) % 4 == 0 && sizeof(Cfg) <= 160, "Cfg is copied dword by dword");

__shared__ uint4 s_rec[3u * DE_V6_P];                // the record slots: three 16-byte parts, part-major ...
__shared__ uint2 s_rec2[DE_V6_P];                    // ... and one of 8 bytes
__shared__ uint16_t s_rings[(NQ + 1) * DE_V6_CAP];   // NR rings of slot numbers
__shared__ uint32_t s_cw[32];                        // head[NR] at 0, tail[NR] at 8, abort at 16, drain statistics at 17, "exporting" at 18, image bands left behind (>= the launch's band count: nothing left to start) at 19, the export decision at 20
__shared__ float s_node_val[64];
__shared__ unsigned long long s_stats[64];
__shared__ uint32_t s_cfg[40];

// (the lane's index from the execution-mask counters, not from threadIdx: a stage function that never asks for the work-item id does not receive it — one VGPR
// more for its allocator, and the scheduler loop has no packed id to keep alive, i.e. to reload from scratch, for every stage call)
DE_DEV int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
DE_DEV uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// What a stage reads of the launch (map descriptors, table pointers, frame constants) arrives through a pointer the optimiser cannot see through
// — as flat loads into VECTOR registers, although every lane gets the same value.  Broadcast to scalar registers: a map's seven dwords in
// VGPRs were what pushed the cloud map's base pointer out to scratch inside the tracking loop (round 5), and a scalar base lets the tap be a
// global_load_dword with the 32-bit offset in one VGPR (de_device.h: map_dword).
DE_DEV float unif(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
template <typename T>
DE_DEV const T* uni_ptr(const T* p) {
    const unsigned long long u = (unsigned long long)p;
    const unsigned long long lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return reinterpret_cast<const T*>((hi << 32) | lo);
}
DE_DEV TexR8 uni_tex(const TexR8& t) {
    TexR8 o;
    o.data = uni_ptr(t.data);
    o.w = __builtin_amdgcn_readfirstlane(t.w); o.h = __builtin_amdgcn_readfirstlane(t.h); o.tiles_x = __builtin_amdgcn_readfirstlane(t.tiles_x);
    o.wf = unif(t.wf); o.hf = unif(t.hf);
    return o;
}
DE_DEV uint32_t ld_wg(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
DE_DEV uint32_t add_wg(uint32_t* p, uint32_t v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
DE_DEV uint32_t ld_e(const uint16_t* p) { return (uint32_t)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
DE_DEV void st_e(uint16_t* p, uint32_t v) { __hip_atomic_store(p, (uint16_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
DE_DEV void release_wg() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); }
DE_DEV void acquire_wg() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }

// records in LDS: 56 bytes — meta, the generator, P, W, x[0..4] (x[5] is never read; the path's id lives in its cold record: a stage
// that can end a path reads that line anyway) — as three 16-byte parts and one of 8, part-major
DE_DEV void load_rec(const uint4* rec, uint32_t s, Path& p) {
    const uint4 a = rec[s], b = rec[DE_V6_P + s], c = rec[2u * DE_V6_P + s];
    const uint2 d = s_rec2[s];
    p.pid = 0u; p.meta = a.x; p.rng.s0 = a.y; p.rng.s1 = a.z; p.rng.draws = 0;
    p.P = v3(wf::asf(a.w), wf::asf(b.x), wf::asf(b.y)); p.W = v3(wf::asf(b.z), wf::asf(b.w), wf::asf(c.x));
    p.x[0] = wf::asf(c.y); p.x[1] = wf::asf(c.z); p.x[2] = wf::asf(c.w); p.x[3] = wf::asf(d.x); p.x[4] = wf::asf(d.y); p.x[5] = 0.0f;
}
DE_DEV void store_rec(uint4* rec, uint32_t s, const Path& p) {
    rec[s] = make_uint4(p.meta, p.rng.s0, p.rng.s1, wf::asu(p.P.x));
    rec[DE_V6_P + s] = make_uint4(wf::asu(p.P.y), wf::asu(p.P.z), wf::asu(p.W.x), wf::asu(p.W.y));
    rec[2u * DE_V6_P + s] = make_uint4(wf::asu(p.W.z), wf::asu(p.x[0]), wf::asu(p.x[1]), wf::asu(p.x[2]));
    s_rec2[s] = make_uint2(wf::asu(p.x[3]), wf::asu(p.x[4]));
}
// ... of a stage that changes only meta, the generator and x of its record, and reads x[2..4] in its finish() alone (Stage::kSlotKept: the gas
// stage).  What it does not change stays in the slot, and what only finish() reads is read again for it: the stage's loop carries neither P nor
// x[2..4] — six registers it has no room for beside its look-ahead (de_stages.h: GasStageT).
DE_DEV void reload_rec_tail(const uint4* rec, uint32_t s, Path& p) {
    const uint2 d = s_rec2[s];
    p.x[2] = wf::asf(reinterpret_cast<const uint32_t*>(rec + 2u * DE_V6_P + s)[3]); p.x[3] = wf::asf(d.x); p.x[4] = wf::asf(d.y);
}
DE_DEV void store_rec_finished(uint4* rec, uint32_t s, const Path& p) {
    uint32_t* a = reinterpret_cast<uint32_t*>(rec + s);
    a[0] = p.meta; a[1] = p.rng.s0; a[2] = p.rng.s1;
    rec[2u * DE_V6_P + s] = make_uint4(wf::asu(p.W.z), wf::asu(p.x[0]), wf::asu(p.x[1]), wf::asu(p.x[2]));
    s_rec2[s] = make_uint2(wf::asu(p.x[3]), wf::asu(p.x[4]));
}
DE_DEV void store_rec_suspended(uint4* rec, uint32_t s, const Path& p) {      // suspend() changes x[0] only
    uint32_t* a = reinterpret_cast<uint32_t*>(rec + s);
    a[0] = p.meta; a[1] = p.rng.s0; a[2] = p.rng.s1;
    reinterpret_cast<uint32_t*>(rec + 2u * DE_V6_P + s)[1] = wf::asu(p.x[0]);
}

// the cold record of the path in THIS lane's slot (the stage bodies index by path id; here the slot decides)
struct ColdAt {
    wf::Cold* c;
    DE_DEV void get_thr_ls(uint32_t, float& thr, float& Ls) const { thr = c->thr; Ls = c->Ls; }
    DE_DEV float get_ls(uint32_t) const { return c->Ls; }
    DE_DEV void set_thr_ls(uint32_t, float thr, float Ls) const { c->thr = thr; c->Ls = Ls; }
    DE_DEV vec3 get_dir(uint32_t) const { return v3(c->dx, c->dy, c->dz); }
    DE_DEV void set_dir(uint32_t, vec3 D) const { c->dx = D.x; c->dy = D.y; c->dz = D.z; }
    DE_DEV void set_surf(uint32_t, vec3 N, float alb, float ocean, float bathy) const { c->nx = N.x; c->ny = N.y; c->nz = N.z; c->alb = alb; c->ocean = ocean; c->bathy = bathy; }
    DE_DEV void get_surf(uint32_t, vec3& N, float& alb, float& ocean, float& bathy) const { N = v3(c->nx, c->ny, c->nz); alb = c->alb; ocean = c->ocean; bathy = c->bathy; }
};

// Everything a wave carries between stages: wave-uniform.
template <bool CLAMP, bool STATS>
struct Wave {
    Cfg A;                      // wave-uniform copy of the workgroup's configuration
    uint4* rec;                 // LDS: the workgroup's record slots
    uint16_t* rings;            // LDS: NR rings of DE_V6_CAP slot numbers
    uint32_t* cw;               // LDS: head[NR] at 0, tail[NR] at 8, abort at 16
    wf::Cold* cold;             // the workgroup's cold records
    unsigned long long* s_st;   // LDS: statistics
    bool primary_left, aborted;      // primary_left: the workgroup's band progress (cw[19]) as this wave last read it — see starters()
    unsigned long long t_mark;
    unsigned long long r_t[R_N], r_l[R_N], r_last, r_cnt[2];      // region statistics of the running stage (STATS builds only)

    DE_DEV void regions_begin() {
        if (!STATS) return;
#pragma unroll
        for (int k = 0; k < R_N; ++k) { r_t[k] = 0ull; r_l[k] = 0ull; }
        r_cnt[0] = r_cnt[1] = 0ull;
        r_last = __builtin_amdgcn_s_memtime();
    }
    // the time since the last call belongs to region R, whose vector code ran for `lanes` lanes
    template <int R>
    DE_DEV void tick(unsigned long long lanes) {
        if (!STATS) return;
        const unsigned long long t = __builtin_amdgcn_s_memtime(), dt = t - r_last;
        r_t[R] += dt; r_l[R] += dt * lanes; r_last = t;
    }
    DE_DEV void stat2(int k, unsigned long long v) {
        if (STATS && lane_id() == 0 && v) __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(A.ctl + (G_STAT2 + k) * DE_V6_CTL_STRIDE), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    DE_DEV void regions_end_loop(int q) {
        if (!STATS) return;
#pragma unroll
        for (int k = 0; k < R_N; ++k) { stat2(14 * q + 2 * k, r_t[k]); stat2(14 * q + 2 * k + 1, r_l[k]); }
        stat2(14 * q + 12, r_cnt[0]); stat2(14 * q + 13, r_cnt[1]);
    }
    // straight-line stages (base = 42 + 4 (q - 3)) and new paths (base = 58): R_STEP = the body, R_PUSH = the pass's ring work
    DE_DEV void regions_end_flat(int base) {
        if (!STATS) return;
        stat2(base, r_t[R_STEP]); stat2(base + 1, r_l[R_STEP]); stat2(base + 2, r_t[R_PUSH]); stat2(base + 3, r_cnt[0]);
    }

    // a stage function's view of the wave: the configuration from LDS (scalar registers after the broadcast), the wave's own flag
    // (Round 6: a wave carries NOTHING from one stage to the next.  What used to travel — the rest of a 256-item work claim, the wave's own "nothing left to
    // start" flag — is gone: work items are claimed 64 at a time AFTER the free slots, and how far the workgroup has come through the image bands is one word of
    // LDS, cw[19].  With the stage functions' callee-saved registers gone (build.py: -enable-ipra) every value the kernel kept live across a stage call cost a
    // scratch store and a load per stage entry; now the scheduler loop re-reads the few configuration words it needs from LDS and keeps none.)
    DE_DEV static Wave enter() {
        Wave W;
        uint32_t* dst = reinterpret_cast<uint32_t*>(&W.A);
#pragma unroll
        for (uint32_t k = 0; k < sizeof(Cfg) / 4u; ++k) dst[k] = uni(s_cfg[k]);
        W.rec = s_rec; W.rings = s_rings; W.cw = s_cw; W.cold = W.A.cold; W.s_st = s_stats;
        W.primary_left = true; W.aborted = false; W.t_mark = 0ull;
        return W;
    }

    // the cloud stage's occupancy bound (STATS builds): lane-steps that needed the exact density lookup, trips in which no lane of the wave did
    // (the whole wave branched past it), lookups of the bound map
    template <typename Stage>
    DE_DEV void cloud_stats(const Stage& st, bool stepping) {
        if constexpr (Stage::kBound) {
            const unsigned long long n_exact = (unsigned long long)__popcll(__ballot(stepping && st.exact));
            stat(ST_CLOUD_EXACT, n_exact);
            stat(ST_CLOUD_NOEXACT, n_exact == 0ull && __ballot(stepping) != 0ull ? 1ull : 0ull);
            stat(ST_CLOUD_LOOKUPS, (unsigned long long)__popcll(__ballot(stepping && st.looked)));
        }
    }
    DE_DEV void stat(int k, unsigned long long v) { if (STATS && lane_id() == 0) __hip_atomic_fetch_add(s_st + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    template <int STAGE>
    DE_DEV void mark() {
        if (!STATS) return;
        const unsigned long long t = __builtin_amdgcn_s_memrealtime();
        stat(STAGE >= 0 ? ST_CYC + STAGE : ST_SCHED, t - t_mark);
        t_mark = t;
    }
    DE_DEV uint32_t* head(uint32_t q) const { return cw + q; }
    DE_DEV uint32_t* tail(uint32_t q) const { return cw + 8u + q; }
    DE_DEV void raise(uint32_t code) {
        if (lane_id() == 0) {
            __hip_atomic_store(cw + 16, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(A.status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        aborted = true;
    }

    // Can this workgroup still start paths?  cw[19] counts the image bands it has found exhausted (run_primary; a tail launch's import stores all ones when
    // the pool is): below the launch's band count, yes.  Monotonic, so a "no" is final — from then on the workgroup's population only falls.
    DE_DEV bool starters() { primary_left = uni(ld_wg(cw + 19)) < A.bands; return primary_left; }

    // claim between kmin and kmax entries of ring q: a compare-and-swap on its head, never past its tail
    DE_DEV uint32_t claim(uint32_t q, uint32_t kmin, uint32_t kmax, uint32_t* first) {
        uint32_t got = 0, hh = 0;
        if (lane_id() == 0) {
            uint32_t h = ld_wg(head(q));
#pragma nounroll
            for (int tries = 0; tries < 16; ++tries) {
                const uint32_t t = ld_wg(tail(q));
                const int avail = (int)(t - h);
                if (avail < (int)kmin) break;
                const uint32_t k = (uint32_t)avail < kmax ? (uint32_t)avail : kmax;
                uint32_t expected = h;
                if (__hip_atomic_compare_exchange_strong(head(q), &expected, h + k, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) { got = k; hh = h; break; }
                h = expected;
            }
        }
        *first = uni(hh);
        return uni(got);
    }
    // A cell that does not hold what its lap's ticket expects yet: wait for it (bounded).  Rare — a consumer that claimed a ticket before its
    // producer stored, a producer a lap ahead of a stalled consumer — and kept out of line: the common path of take / push is one look, decided
    // for the whole wave with one branch (a per-lane bounded loop around every look cost 25 scalar instructions per append: +4 % frame time).
    __device__ __attribute__((noinline)) uint32_t wait_cell(uint16_t* e, uint32_t lap, bool want_entry) {
        uint32_t x = DE_V6_SLOT_MASK + 1u;
#pragma nounroll
        for (uint32_t spins = 0; spins < (1u << 20); ++spins) {
            x = cell_for(ld_e(e), lap);
            if (want_entry ? x < DE_V6_SLOT_MASK : x == DE_V6_SLOT_MASK) return x;
            __builtin_amdgcn_s_sleep(1);
        }
        return DE_V6_SLOT_MASK + 1u;      // timed out
    }
    // the slot number in entry idx of ring q (claimed by this wave): the entry ITS producer (same lap) stored; the cell is left empty for the next lap
    DE_DEV uint32_t take(uint32_t q, uint32_t idx) {
        const uint32_t lap = idx / DE_V6_CAP;
        uint16_t* e = rings + q * DE_V6_CAP + (idx - lap * DE_V6_CAP);
        uint32_t x = cell_for(ld_e(e), lap);
        if (__ballot(x >= DE_V6_SLOT_MASK) != 0ull) {
            if (x >= DE_V6_SLOT_MASK) x = wait_cell(e, lap, true);
            if (x >= DE_V6_SLOT_MASK) return DE_V6_EMPTY;
        }
        st_e(e, cell_empty(lap + 1u));
        return x;
    }
    // append the slot numbers of the lanes with pred to ring Q (their records are written and released): one fetch-add for the wave's tickets;
    // a cell is stored once the take of the previous lap has emptied it (with DE_V6_CAP > DE_V6_P that is so at the first look unless a consumer
    // stalls).  What counts here is the instruction count, not the LDS round trips — the SIMD's other waves cover those, the kernel is bound by
    // instruction issue: a version that took the tickets of all target rings with ONE LDS instruction halved a service's time in its own wave
    // and cost the frame 4 % (more vector instructions, executed for every target whether it had records or not).
    template <int Q>
    DE_DEV void push(uint32_t slot, bool pred) {
        const unsigned long long mask = __ballot(pred);
        if (mask == 0ull) return;
        const uint32_t n = (uint32_t)__popcll(mask), rank = (uint32_t)__popcll(mask & ((1ull << lane_id()) - 1ull));
        uint32_t base = 0;
        if (lane_id() == 0) base = add_wg(tail(Q), n);
        base = uni(base);
        if (pred) {
            const uint32_t idx = base + rank, lap = idx / DE_V6_CAP;
            uint16_t* e = rings + Q * DE_V6_CAP + (idx - lap * DE_V6_CAP);
            bool ok = cell_for(ld_e(e), lap) == DE_V6_SLOT_MASK;
            if (__ballot(!ok) != 0ull) {
                if (!ok) ok = wait_cell(e, lap, false) == DE_V6_SLOT_MASK;
                if (__ballot(!ok) != 0ull) raise(ERR_CELL_BUSY_TIMEOUT);
            }
            if (ok) st_e(e, cell_full(lap, slot));
        }
    }

    // STATS builds: the workgroup's population once the work items are gone, sampled by whichever wave passes the scheduler first in each 0.25 ms bucket
    DE_DEV void drain_sample(uint32_t live) {
        if (lane_id() != 0) return;
        const unsigned long long t0 = __hip_atomic_load(reinterpret_cast<unsigned long long*>(A.ctl + G_T_EXHAUSTED * DE_V6_CTL_STRIDE), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        if (now < t0) return;
        const unsigned long long bb = (now - t0) / 25000ull + 1ull;
        const uint32_t b = bb < 32ull ? (uint32_t)bb : 32u;
        const uint32_t old = __hip_atomic_fetch_max(cw + 17, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        for (uint32_t k = old; k < b; ++k) {
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(A.ctl + (G_DRAIN + k) * DE_V6_CTL_STRIDE), (unsigned long long)live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(A.ctl + (G_DRAIN + 32u + k) * DE_V6_CTL_STRIDE), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // ---- the scheduler: which stage this wave runs next — a queue id, Q_PRIMARY, or Q_EXIT
    DE_DEV int schedule() {
        uint32_t idle = 0;
        for (;;) {
            // ONE batch of LDS reads per round: the control words 16 .. 23 (abort, drain, exporting, band progress, the export decision) in lanes 0 .. 7 and the
            // rings' depths, issued back to back and waited for once (the abort word used to be a round trip of its own before the others were even issued).
            // The band word is READ before the ring counters — LDS executes a wave's operations in order —: once it says "nothing left to start" the free ring
            // read after it bounds the population for good.
            const uint32_t l = (uint32_t)lane_id();
            const uint32_t misc = ld_wg(cw + 16 + (l & 7u));
            int ready = 0;
            if (l < (uint32_t)NR) ready = (int)(ld_wg(tail(l)) - ld_wg(head(l)));
            if (!aborted && __builtin_amdgcn_readlane((int)misc, 0) != 0) aborted = true;
            if (aborted) return Q_EXIT;      // the workgroup's own word: the workgroups share nothing but the work counters, the others finish their paths
            primary_left = (uint32_t)__builtin_amdgcn_readlane((int)misc, 3) < A.bands;
            int best_q = -1, best = 0, low_q = -1, low = 0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int r = __builtin_amdgcn_readlane(ready, q);
                const bool shallow_flat = q > Q_CLOUD && r < (int)A.flat_min;      // the straight-line stages wait for a fuller pass while the loop stages have work
                if (!shallow_flat && r > best) { best = r; best_q = q; }
                if (shallow_flat && r > low) { low = r; low_q = q; }
            }
            if (best_q < 0) { best_q = low_q; best = low; }
            // a shallow ring is left alone for a few rounds (its records fill the idle lanes of the waves already in that stage, or it
            // deepens) unless nothing else is there
            if (best_q >= 0 && best < (int)A.enter_min && idle < 4u) best_q = -1;
            const int free_slots = __builtin_amdgcn_readlane(ready, Q_FREE);
            if (STATS && !primary_left) drain_sample((uint32_t)((int)DE_V6_P - free_slots));
            if (A.export_at != 0u && !primary_left) {
                // the tail: nothing left to start and few paths alive — from here on this workgroup only exports (see "The tail")
                const uint32_t live = DE_V6_P - (uint32_t)free_slots;
                // (nothing is left to start for the WHOLE workgroup — cw[19], read before the rings above: from then on the population can only fall — a wave that
                // is still inside run_primary holds its 64 slots out of the free ring, so they count as alive — and a workgroup exports at most export_at records:
                // the pool cannot overflow)
                bool exporting = __builtin_amdgcn_readlane((int)misc, 2) != 0;
                if (!exporting && live != 0u && live <= A.export_at) {
                    // Export only if another launch of this context is queued behind this one: the slots this workgroup frees are then taken at once, which is
                    // what the chain is for; a launch with nothing behind it (a frame rendered alone, the last call before a fetch) would only end later for it —
                    // the tail launch cannot start before the last workgroup here has exported.  Decided once per workgroup (one read of host memory).
                    uint32_t dec = (uint32_t)__builtin_amdgcn_readlane((int)misc, 4);      // 0: not decided, 1: export, 2: finish in place
                    if (dec == 0u) {
                        if (lane_id() == 0) {
                            dec = (A.seq == 0xffffffffu || (int)(__hip_atomic_load(A.issued, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - A.seq) >= 0) ? 1u : 2u;
                            __hip_atomic_store(cw + 20, dec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                        dec = uni(dec);
                    }
                    if (dec == 1u) {
                        if (lane_id() == 0) __hip_atomic_store(cw + 18, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        exporting = true;
                    }
                }
                if (exporting) {
                    if (best > 0) return Q_EXPORT;
                    if (free_slots == (int)DE_V6_P) return Q_EXIT;
                    if (++idle > A.idle_limit) { raise(ERR_IDLE_WATCHDOG); return Q_EXIT; }
                    __builtin_amdgcn_s_sleep(8);      // records are still in the lanes of a loop stage (they come back at its next dry service) or in a straight-line pass
                    continue;
                }
            }
            // new paths as soon as a wave-load of slots is free: the population stays at the pool's size, the rings stay deep
            if (primary_left && free_slots >= 64) return Q_PRIMARY;
            if (best_q >= 0) { stat(ST_ENTRIES, 1); return best_q; }
            if (!primary_left && free_slots == (int)DE_V6_P) return Q_EXIT;      // every slot is home and nothing is left to start
            stat(ST_IDLE, 1);
            if (++idle > A.idle_limit) { raise(ERR_IDLE_WATCHDOG); return Q_EXIT; }
            // An idle wave backs off: a scheduler round is ~100 instructions, and in a launch's drain — most of a one-sample launch — eleven of a workgroup's twelve
            // waves are idle: at one round per ~0.5 us they took a third of the instructions such a launch executes, from the working waves of the launches that
            // overlap with it.  With twelve waves waking at different times a record still waits only a fraction of one sleep.
            // (no back-off, or one capped at s_sleep 32: within noise of this on every workload measured — profiles/experiments/README.md, round 6)
            if (idle < 8u) __builtin_amdgcn_s_sleep(2);
            else if (idle < 24u) __builtin_amdgcn_s_sleep(16);
            else if (idle < 64u) __builtin_amdgcn_s_sleep(48);
            else __builtin_amdgcn_s_sleep(100);
        }
    }

    // ---- a loop stage: persistent lanes.  A lane takes a slot, loads its record, runs the stage's loop on it one step per trip of the
    // wave loop, keeps the finished record until the wave's next service; a service writes the finished records back, appends their
    // slots to the next stages' rings and refills the idle lanes from this stage's ring.
    template <int Q, typename Stage, int... TARGETS>
    DE_DEV void run_loop(Stage& st, Targets<TARGETS...>) {
        // When to service.  Idle lanes waste a fraction of every trip; a service (epilogue, appends, claim, record loads, begin()) costs a fixed
        // number of trips' worth of issue slots whatever the number of lanes it serves.  With records ending at a rate of r lanes per trip the
        // waste since the last service grows like r t^2 / 2 lane-trips, and the cost per trip (waste + service) / t is least when the waste
        // accumulated EQUALS the service's cost: service when the idle lane-trips since the last one reach AREA = 64 x (service cost / trip
        // cost) — a property of the stage's code, not of the view.  A fixed idle-lane threshold (rounds 3-4: 24 / 24 / 20, the BASELINE cfg2 optimum)
        // is that rule for ONE rate r: cloud segments of the limb view are five times longer and wanted 12 (VERDICT r4 #1b).
        const int SERVICE = (int)A.svc[Q];
        const uint32_t AREA = A.svc_area[Q];
        uint32_t idle_acc = 0;
        Path p;
        uint32_t slot = 0;
        bool busy = false, fin = false;
        int target = -1;
        bool dry = false;
        uint32_t trips = 0, retry_at = 0;
        regions_begin();
        // Two loops: the OUTER one decides about a service when one is due (and is where the stage ends); the INNER one is nothing but steps — one
        // ballot, one add and one scalar compare per trip — until the idle lane-trips reach AREA.  (One loop with the four-way service condition at
        // its head: 4.7 % more vector and 17 % more scalar instructions per frame; with a one-compare head in ONE loop: cfg2 108.9 -> 105.8 ms, limb
        // view 317 -> 300 on one box — the compiler's code for a loop with many exits carries its exit state through every trip.)
        for (;;) {
            const int nb = __popcll(__ballot(busy));
            const bool may_refill = !dry || trips >= retry_at;
            if (nb == 0 || ((AREA != 0u || 64 - nb >= SERVICE) && (may_refill || __ballot(fin) != 0ull))) {
                idle_acc = 0u;
                tick<R_HEAD>(0ull);
                if (STATS) r_cnt[0]++;
                if (__ballot(fin) != 0ull) {
                    // the stage's epilogue for all the lanes that finished since the last service at once (run where a lane finishes it
                    // would execute for two or three lanes of 64 in most trips)
                    const unsigned long long n_fin = STATS ? (unsigned long long)__popcll(__ballot(fin)) : 0ull;
                    if (fin) {
                        if constexpr (Stage::kSlotKept) { reload_rec_tail(rec, slot, p); target = st.finish(p); store_rec_finished(rec, slot, p); }
                        else { target = st.finish(p); store_rec(rec, slot, p); }
                    }
                    tick<R_EPI>(n_fin);
                    release_wg();
                    (push<TARGETS>(slot, fin && target == TARGETS), ...);
                    fin = false;
                    tick<R_PUSH>(n_fin);
                }
                if (may_refill || nb == 0) {
                    dry = false;
                    const unsigned long long m_need = __ballot(!busy);
                    uint32_t first = 0;
                    const uint32_t got = claim(Q, 1u, (uint32_t)__popcll(m_need), &first);
                    if (got == 0u) {
                        dry = true; retry_at = trips + A.retry;
                        tick<R_REFILL>(0ull);
                        // Nothing to refill from, a few long records left, and other work waits: hand the records back — the loop's
                        // state goes to the spare words of their cold records — so that they fill the idle lanes of another wave of this
                        // stage instead of running here at a fraction of the wave (cloud segments have a heavy tail)
                        // (or the workgroup is exporting its last paths — "The tail": whatever runs here goes back to the ring, from there to the pool)
                        if (nb > 0 && ((nb <= (int)A.yield_max && work_elsewhere(Q)) || (A.export_at != 0u && uni(ld_wg(cw + 18)) != 0u))) {
                            if (busy) {
                                st.suspend(p, cold + slot);
                                p.meta |= 0x80000000u;
                                if constexpr (Stage::kSlotKept) store_rec_suspended(rec, slot, p);
                                else store_rec(rec, slot, p);
                            }
                            release_wg();
                            push<Q>(slot, busy);
                            stat(ST_YIELD, 1); stat(ST_YIELDED, (unsigned long long)nb);
                            busy = false;
                            tick<R_YIELD>((unsigned long long)nb);
                            break;
                        }
                    } else {
                        const uint32_t my = (uint32_t)__popcll(m_need & ((1ull << lane_id()) - 1ull));
                        const bool mine = !busy && my < got;
                        uint32_t s = 0;
                        if (mine) s = take(Q, first + my);
                        if (__ballot(mine && s == DE_V6_EMPTY) != 0ull) { raise(ERR_ENTRY_TIMEOUT); break; }
                        acquire_wg();
                        if (mine) {
                            slot = s; load_rec(rec, slot, p);
                            const bool resumed = (p.meta & 0x80000000u) != 0u;
                            p.meta &= 0x7fffffffu;
                            st.begin(p);
                            if (resumed) st.restore(cold + slot); else st.start(p);
                            busy = true;
                        }
                        stat(ST_RECS + Q, got);
                        tick<R_REFILL>((unsigned long long)got);
                    }
                }
                if (__ballot(busy) == 0ull) { if (dry || aborted) break; else continue; }
            }
            const bool was_busy = busy;           // a lane that is busy now and not after the steps has finished its record: one mask to keep per trip, not two
            do {
                const unsigned long long n_step = STATS ? (unsigned long long)__popcll(__ballot(busy)) : 0ull;
                if (STATS) { stat(ST_TRIPS + Q, 1); stat(ST_LANETRIPS + Q, n_step); r_cnt[1]++; }
                tick<R_HEAD>(0ull);
                const bool stepping = busy;
                if (busy) {
                    if (st.step(p)) busy = false;
                }
                if constexpr (STATS && Q == Q_CLOUD) cloud_stats(st, stepping);
                tick<R_STEP>(n_step);
                trips++;
                idle_acc += (uint32_t)(64 - __popcll(__ballot(busy)));
            } while (idle_acc < AREA);
            fin = fin || (was_busy && !busy);
        }
        tick<R_HEAD>(0ull);
        regions_end_loop(Q);
    }
    // is there a wave-load of work outside ring q (another stage's ring, or free slots for new paths)?
    DE_DEV bool work_elsewhere(uint32_t q) {
        int ready = 0;
        const uint32_t l = (uint32_t)lane_id();
        if (l < (uint32_t)NR && l != q) ready = (int)(ld_wg(tail(l)) - ld_wg(head(l)));
        if (l == (uint32_t)Q_FREE && !starters()) ready = 0;
        return __ballot(ready >= (int)A.elsewhere_min) != 0ull;
    }

    // ---- the tail: every queued record of ring Q to the pool (its slot goes home); the records in the lanes of the loop stages follow when those yield
    template <int Q>
    DE_DEV void export_ring(const Pool& pool) {
        for (;;) {
            uint32_t first = 0;
            const uint32_t n = claim(Q, 1u, 64u, &first);
            if (n == 0u) break;
            const bool active = (uint32_t)lane_id() < n;
            uint32_t slot = 0;
            if (active) slot = take(Q, first + (uint32_t)lane_id());
            if (__ballot(active && slot == DE_V6_EMPTY) != 0ull) { raise(ERR_ENTRY_TIMEOUT); break; }
            acquire_wg();
            uint32_t base = 0;
            if (lane_id() == 0) base = __hip_atomic_fetch_add(A.ctl + (G_POOL + 2u * A.level) * DE_V6_CTL_STRIDE, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            base = uni(base);
            if (base + n > A.cap_out) { raise(ERR_POOL_FULL); break; }      // cannot happen: a workgroup exports at most export_at records, the pool holds that many per workgroup
            if (active) {
                const uint32_t i = base + (uint32_t)lane_id();
                pool.a[i] = rec[slot]; pool.b[i] = rec[DE_V6_P + slot]; pool.c[i] = rec[2u * DE_V6_P + slot]; pool.d[i] = s_rec2[slot];
                const uint4* cs = reinterpret_cast<const uint4*>(cold + slot);
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) pool.cold[(size_t)k * A.cap_out + i] = cs[k];
                pool.q[i] = (uint32_t)Q;
            }
            push<Q_FREE>(slot, active);
        }
    }
    template <int... QS>
    DE_DEV void run_export(Targets<QS...>) {
        const Pool pool(A.pool_out, A.cap_out);
        (export_ring<QS>(pool), ...);
    }
    // ---- a tail launch's "new paths": up to 64 entries of the pool the previous level exported, each to the ring it waited in
    DE_DEV void run_import() {
        uint32_t first = 0;
        if (claim(Q_FREE, 64u, 64u, &first) == 0u) { stat(ST_CLAIMFAIL, 1); return; }
        uint32_t slot = take(Q_FREE, first + (uint32_t)lane_id());
        if (__ballot(slot == DE_V6_EMPTY) != 0ull) { raise(ERR_ENTRY_TIMEOUT); return; }
        acquire_wg();
        uint32_t w = 0, total = 0;
        if (lane_id() == 0) {
            w = __hip_atomic_fetch_add(A.ctl + (G_POOL + 2u * (A.level - 1u) + 1u) * DE_V6_CTL_STRIDE, 64u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            total = __hip_atomic_load(A.ctl + (G_POOL + 2u * (A.level - 1u)) * DE_V6_CTL_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // final: the exporting launch has ended
        }
        w = uni(w); total = min(uni(total), A.cap_in);
        const uint32_t n = w < total ? min(64u, total - w) : 0u;
        const bool active = (uint32_t)lane_id() < n;
        uint32_t q = 0xffu;
        if (active) {
            const Pool pool(A.pool_in, A.cap_in);
            const uint32_t i = w + (uint32_t)lane_id();
            rec[slot] = pool.a[i]; rec[DE_V6_P + slot] = pool.b[i]; rec[2u * DE_V6_P + slot] = pool.c[i]; s_rec2[slot] = pool.d[i];
            uint4* cd = reinterpret_cast<uint4*>(cold + slot);
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) cd[k] = pool.cold[(size_t)k * A.cap_in + i];
            q = pool.q[i];
        }
        stat(ST_RECS + NQ, n);
        release_wg();
        push<Q_ST>(slot, q == (uint32_t)Q_ST); push<Q_GAS>(slot, q == (uint32_t)Q_GAS); push<Q_CLOUD>(slot, q == (uint32_t)Q_CLOUD); push<Q_EVENT>(slot, q == (uint32_t)Q_EVENT);
        push<Q_SURF>(slot, q == (uint32_t)Q_SURF); push<Q_SCFIN>(slot, q == (uint32_t)Q_SCFIN); push<Q_SURFFIN>(slot, q == (uint32_t)Q_SURFFIN);
        push<Q_FREE>(slot, !active);      // the slots claimed beyond the pool's end go home
        if (n < 64u && lane_id() == 0) __hip_atomic_store(cw + 19, 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // the pool is exhausted: nothing left to start
    }

    // ---- a straight-line stage: up to 64 slots per pass, one record per lane, written back in place
    template <int Q, typename Body, int... TARGETS>
    DE_DEV void run_flat(Body body, Targets<TARGETS...>) {
        regions_begin();
        uint32_t kmin = 1u;
        for (;;) {
            uint32_t first = 0;
            const uint32_t n = claim(Q, kmin, 64u, &first);
            if (n == 0u) break;
            kmin = A.flat_again;      // what arrived during the pass is left to deepen unless it is worth a pass of its own (a thin pass costs a full one's instructions)
            const bool active = (uint32_t)lane_id() < n;
            uint32_t slot = 0;
            if (active) slot = take(Q, first + (uint32_t)lane_id());
            if (__ballot(active && slot == DE_V6_EMPTY) != 0ull) { raise(ERR_ENTRY_TIMEOUT); break; }
            acquire_wg();
            Path p;
            int target = -2;
            if (active) {
                load_rec(rec, slot, p);
                p.pid = wf::asu(cold[slot].pad0);
            }
            tick<R_PUSH>(0ull);
            if (active) {
                target = body(p, ColdAt{cold + slot});
            }
            tick<R_STEP>((unsigned long long)n);
            if (active && target >= 0) store_rec(rec, slot, p);
            stat(ST_RECS + Q, n);
            if (STATS) { stat(ST_TRIPS + Q, 1); stat(ST_LANETRIPS + Q, n); r_cnt[0]++; }
            release_wg();
            (push<TARGETS>(slot, target == TARGETS), ...);
            push<Q_FREE>(slot, target == -1);
            tick<R_PUSH>(0ull);
        }
        tick<R_PUSH>(0ull);
        regions_end_flat(42 + 4 * (Q - 3));
    }

    // ---- new paths: 64 work items = the 64 pixels of one screen tile for one sample; the primary sphere trace runs here (coherent rays)
    DE_DEV void run_primary(const RenderArgs& a, const FrameConsts& fc) {      // (two or four batches per visit: no gain — profiles/experiments/README.md, round 6)
        regions_begin();
        primary_batch(a, fc);
        regions_end_flat(58);
    }
    // one batch of 64 new paths
    DE_DEV void primary_batch(const RenderArgs& a, const FrameConsts& fc) {
        // a wave-load of free slots FIRST, then the work items for them: a wave holds no claim from one call to the next (a failed slot claim used to keep the
        // rest of a 256-item claim in the wave's registers across stage calls)
        uint32_t first = 0;
        if (claim(Q_FREE, 64u, 64u, &first) == 0u) { stat(ST_CLAIMFAIL, 1); return; }      // another wave was quicker: back to the scheduler
        uint32_t slot = take(Q_FREE, first + (uint32_t)lane_id());
        if (__ballot(slot == DE_V6_EMPTY) != 0ull) { raise(ERR_ENTRY_TIMEOUT); return; }
        // Work items (64 = one screen tile x one sample; a tile's samples are consecutive) are handed out 64 per atomic from EIGHT counters, one per band
        // of the launch's tiles, and a workgroup draws from the band of the XCD it runs on: the workgroups that share an L2 render neighbouring tiles at
        // the same time, the eight L2s hold eight different parts of the maps (one counter for the launch dealt a tile's samples to sixteen workgroups on
        // all eight XCDs: every L2 held the same lines).  A band that has run out sends its workgroups to the next XCD's — cw[19] counts the bands this
        // workgroup has left behind, for all its waves — so the launch ends as it did before.
        const uint32_t nb = A.bands, spp = (uint32_t)a.spp_count, per = ((uint32_t)a.n_tiles + nb - 1u) / nb;
        uint32_t tries = uni(ld_wg(cw + 19)), w0 = 0u, n = 0u;
        for (;;) {
            if (tries >= nb) {
                primary_left = false;
                const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                if (lane_id() == 0) __hip_atomic_fetch_min(reinterpret_cast<unsigned long long*>(A.ctl + G_T_EXHAUSTED * DE_V6_CTL_STRIDE), now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            const uint32_t band = (A.xcd + tries) % nb;
            const uint32_t lo = min(band * per, (uint32_t)a.n_tiles) * 64u * spp, hi = min((band + 1u) * per, (uint32_t)a.n_tiles) * 64u * spp;
            uint32_t w = 0;
            if (lane_id() == 0) w = __hip_atomic_fetch_add(A.ctl + (G_WORKX + band) * DE_V6_CTL_STRIDE, 64u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            w = uni(w);
            if (w < hi - lo) { w0 = lo + w; n = min(64u, hi - lo - w); break; }
            tries++;
            if (lane_id() == 0) __hip_atomic_fetch_max(cw + 19, tries, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        const uint32_t w = w0 + (uint32_t)lane_id();
        const bool active = (uint32_t)lane_id() < n;
        acquire_wg();
        const float MAX_RAY_DIST = (float)(6371e3 * 10.0);
        Path p;
        int target = -2;
        tick<R_PUSH>(0ull);
        if (active) {
            wf::new_path(a, fc, bs::s_node_val, w, p);
            const float t = wf::sphere_trace<CLAMP>(a, p, fc.land_height_scale, DE_PLANET_R + de_max(fc.land_height_scale, 0.0f) + 8100.0f, MAX_RAY_DIST);
            target = wf::after_sphere_trace(p, t, MAX_RAY_DIST);
            // (the first gas steps of the primary ray run inline here — all 64 lanes start a gas segment at once —: bit-identical, flat; profiles/experiments/r6_primary_gas.patch)
            store_rec(rec, slot, p);
            cold[slot].pad0 = wf::asf(p.pid);
        }
        tick<R_STEP>((unsigned long long)n);
        stat(ST_RECS + NQ, n);
        if (STATS) r_cnt[0]++;
        release_wg();
        push<Q_GAS>(slot, target == Q_GAS);
        push<Q_CLOUD>(slot, target == Q_CLOUD);
        push<Q_EVENT>(slot, target == Q_EVENT);
        push<Q_FREE>(slot, !active);      // no work item came for these slots (the launch's last claims): they go home
        tick<R_PUSH>(0ull);
    }
};

}  // namespace bs


// zero the control words and put the launch's RenderArgs where the persistent kernel reads them
__global__ void v6_init_kernel(uint32_t* ctl, RenderArgs a, RenderArgs* dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (uint32_t)bs::G_WORDS) {
        const uint32_t fill = (i == (uint32_t)bs::G_T_START || i == (uint32_t)bs::G_T_EXHAUSTED) ? 0xffffffffu : 0u;      // the two minima start at the maximum
        ctl[i * DE_V6_CTL_STRIDE] = fill; ctl[i * DE_V6_CTL_STRIDE + 1u] = fill;
    }
    if (i == 0u) *dst = a;
}

// ---- the stage functions: NOT inlined into the kernel — one register allocation per stage (see "Geometry").  A stage function builds
// its view of the wave from LDS, runs the stage until its ring is dry (or it hands its records back) and returns to the scheduler.
#define DE_V6_STAGE template <bool CLAMP, bool STATS> static __device__ __attribute__((noinline)) void
DE_V6_STAGE v6_stage_st() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    const RenderArgs& a = *W.A.ra;
    const FrameConsts& fc = *W.A.fc;
    const float MAX_RAY_DIST = (float)(6371e3 * 10.0);
    // (the topography's descriptor stays in vector registers: as scalars its fields meet the one-scalar-operand limit of a vector instruction in
    // the tap's address arithmetic — 13 more instructions per sphere-trace step)
    StStage<CLAMP> st{a.topo, fc.land_height_scale, DE_PLANET_R + de_max(fc.land_height_scale, 0.0f) + 8100.0f, MAX_RAY_DIST, 0.0f, 0};
    W.template run_loop<Q_ST>(st, Targets<Q_GAS, Q_CLOUD, Q_EVENT, Q_SURFFIN>{});
}
DE_V6_STAGE v6_stage_gas() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    const RenderArgs& a = *W.A.ra;
#if defined(DE_GAS_EVAL) || defined(DE_FAST_MATH)
    GasStage st{uni_ptr(a.nodes), uni_ptr(a.dens_table)};           // the profiles evaluated: A/B (tools/ab_build.sh), and the fast-math unit, whose exponentials are not the altitude table's
#else
    GasStageAhead st{uni_ptr(a.nodes), uni_ptr(a.dens_table)};      // densities from the context's altitude table, read one step ahead (de_stages.h)
#endif
    W.template run_loop<Q_GAS>(st, Targets<Q_CLOUD, Q_EVENT, Q_SCFIN, Q_SURFFIN>{});
}
DE_V6_STAGE v6_stage_cloud() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    const RenderArgs& a = *W.A.ra;
#ifndef DE_NO_CLOUD_BOUND
    CloudStage<CLAMP, true> st{uni_tex(a.clouds), uni_ptr(a.cloud_bound)};      // exact density lookups only where the occupancy bound allows a cloud (de_stages.h)
#else
    CloudStage<CLAMP> st{uni_tex(a.clouds)};
#endif
    W.template run_loop<Q_CLOUD>(st, Targets<Q_EVENT, Q_SCFIN, Q_SURFFIN>{});
}
DE_V6_STAGE v6_stage_event() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    const RenderArgs& a = *W.A.ra;
    const FrameConsts& fc = *W.A.fc;
    W.template run_flat<Q_EVENT>([&](Path& p, const ColdAt& cold) { return wf::event_body<CLAMP>(a, fc, cold, p); }, Targets<Q_GAS, Q_CLOUD, Q_SCFIN, Q_SURF>{});
}
DE_V6_STAGE v6_stage_surf() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    const RenderArgs& a = *W.A.ra;
    const FrameConsts& fc = *W.A.fc;
    W.template run_flat<Q_SURF>([&](Path& p, const ColdAt& cold) { return wf::surf_body<CLAMP>(a, fc, cold, p); }, Targets<Q_ST>{});
}
DE_V6_STAGE v6_stage_scfin() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    const RenderArgs& a = *W.A.ra;
    const FrameConsts& fc = *W.A.fc;
    W.template run_flat<Q_SCFIN>([&](Path& p, const ColdAt& cold) { return wf::scfin_body(a, fc, cold, p); }, Targets<Q_ST>{});
}
DE_V6_STAGE v6_stage_surffin() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    const RenderArgs& a = *W.A.ra;
    W.template run_flat<Q_SURFFIN>([&](Path& p, const ColdAt& cold) { return wf::surffin_body(a, cold, p); }, Targets<Q_ST>{});
}

// TAIL = false: the launch that starts a frame's paths (level 0).  TAIL = true: a tail launch — the same scheduler and stage functions, its new
// paths are the previous level's pool (its own kernel name, so that a kernel trace tells the two apart).
// the tail's two record movers, out of line like the stages (inlined they cost the kernel's own body — the scheduler and the new paths — its registers)
DE_V6_STAGE v6_stage_export() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    W.run_export(Targets<Q_ST, Q_GAS, Q_CLOUD, Q_EVENT, Q_SURF, Q_SCFIN, Q_SURFFIN>{});
}
DE_V6_STAGE v6_stage_import() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    W.run_import();
}
// new paths (TAIL = false launches): out of line as well — the kernel's own body is the scheduler loop and nothing else
DE_V6_STAGE v6_stage_primary() {
    using namespace bs;
    Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
    const RenderArgs& a = *wf::opaque_ptr(W.A.ra);
    const FrameConsts& fc = *wf::opaque_ptr(W.A.fc);
    W.run_primary(a, fc);
}

template <bool CLAMP, bool STATS, bool TAIL>
__global__ void __attribute__((amdgpu_flat_work_group_size(64 * DE_V6_WAVES, 64 * DE_V6_WAVES), amdgpu_waves_per_eu(DE_V6_WPE, DE_V6_WPE)))
v6_kernel(bs::Args A, const FrameConsts* fcp) {
    using namespace bs;
    for (uint32_t i = threadIdx.x; i < NR * DE_V6_CAP; i += blockDim.x) {
        const uint32_t q = i / DE_V6_CAP, k = i % DE_V6_CAP;
        s_rings[i] = (uint16_t)((q == (uint32_t)Q_FREE && k < DE_V6_P) ? cell_full(0u, k) : cell_empty(0u));
    }
    if (threadIdx.x < 32u) s_cw[threadIdx.x] = (threadIdx.x == 8u + (uint32_t)Q_FREE) ? DE_V6_P : 0u;      // ([19]: image bands this workgroup has left behind, 0 at the start)
    if (threadIdx.x < 64u) { s_node_val[threadIdx.x] = A.ra->node_val[threadIdx.x]; s_stats[threadIdx.x] = 0ull; }
    if (threadIdx.x == 0u) {
        Cfg c;
        c.ra = A.ra; c.fc = fcp; c.cold = A.cold + (size_t)blockIdx.x * DE_V6_P; c.ctl = A.ctl; c.status = A.status;
        c.n_items = A.n_items; c.idle_limit = A.idle_limit;
        c.svc[0] = A.svc[0]; c.svc[1] = A.svc[1]; c.svc[2] = A.svc[2];
        c.svc_area[0] = A.svc_area[0]; c.svc_area[1] = A.svc_area[1]; c.svc_area[2] = A.svc_area[2];
        c.yield_max = A.yield_max; c.elsewhere_min = A.elsewhere_min; c.retry = A.retry; c.enter_min = A.enter_min; c.flat_min = A.flat_min; c.flat_again = A.flat_again;
        c.bands = A.bands == 8u ? 8u : 1u;
        c.pool_in = A.pool_in; c.pool_out = A.pool_out; c.level = A.level; c.export_at = A.export_at; c.cap_in = A.cap_in; c.cap_out = A.cap_out; c.issued = A.issued; c.seq = A.seq; c.pad_ = 0u;
        { uint32_t xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc)); c.xcd = xcc & 7u; }
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&c);
        for (uint32_t k = 0; k < sizeof(Cfg) / 4u; ++k) s_cfg[k] = src[k];
    }
    __syncthreads();
    if (!TAIL && threadIdx.x == 0u) __hip_atomic_fetch_min(reinterpret_cast<unsigned long long*>(A.ctl + G_T_START * DE_V6_CTL_STRIDE), (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // The scheduler loop keeps NOTHING live across a stage call (statistics builds: the time stamp): the stage functions preserve no register (build.py:
    // -enable-ipra), so every value held here would be a scratch store and a load per stage entry, 13.9 M times per BASELINE cfg2 frame.  The wave's view of the
    // workgroup is rebuilt from LDS in every round (the few configuration words schedule() reads).
    unsigned long long t_mark = STATS ? __builtin_amdgcn_s_memrealtime() : 0ull;
    for (;;) {
        Wave<CLAMP, STATS> W = Wave<CLAMP, STATS>::enter();
        W.t_mark = t_mark;
        const int s = __builtin_amdgcn_readfirstlane(W.schedule());      // wave-uniform by construction: said so, the dispatch below is scalar compares instead of an exec-masked branch tree
        W.template mark<-1>();
        if (s == Q_EXIT) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (lane_id() == 0) __hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(A.ctl + G_T_END * DE_V6_CTL_STRIDE), now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (STATS) {      // the wave's drain: from the launch's first "no work item left" to this wave's exit
                const unsigned long long t0 = __hip_atomic_load(reinterpret_cast<unsigned long long*>(A.ctl + G_T_EXHAUSTED * DE_V6_CTL_STRIDE), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (t0 != ~0ull && now > t0) W.stat(ST_DRAIN, now - t0);
            }
            break;
        }
        if (STATS && s < NQ) W.stat(ST_ENTRY_Q + s, 1);
        switch (s) {
        case Q_ST: v6_stage_st<CLAMP, STATS>(); W.template mark<Q_ST>(); break;
        case Q_GAS: v6_stage_gas<CLAMP, STATS>(); W.template mark<Q_GAS>(); break;
        case Q_CLOUD: v6_stage_cloud<CLAMP, STATS>(); W.template mark<Q_CLOUD>(); break;
        case Q_EVENT: v6_stage_event<CLAMP, STATS>(); W.template mark<Q_EVENT>(); break;
        case Q_SURF: v6_stage_surf<CLAMP, STATS>(); W.template mark<Q_SURF>(); break;
        case Q_SCFIN: v6_stage_scfin<CLAMP, STATS>(); W.template mark<Q_SCFIN>(); break;
        case Q_SURFFIN: v6_stage_surffin<CLAMP, STATS>(); W.template mark<Q_SURFFIN>(); break;
        case Q_EXPORT: v6_stage_export<CLAMP, STATS>(); W.template mark<-1>(); break;
        default:
            if (TAIL) v6_stage_import<CLAMP, STATS>(); else v6_stage_primary<CLAMP, STATS>();
            W.template mark<7>();
            break;
        }
        t_mark = W.t_mark;
    }
    if (STATS) {
        __syncthreads();
        if (threadIdx.x < (uint32_t)ST_N && s_stats[threadIdx.x])
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(A.ctl + (G_STAT0 + threadIdx.x) * DE_V6_CTL_STRIDE), s_stats[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// bc6h_kernels.hip — the BC6H_UF16 encoder of the IBL output (include/digital_earth_ibl_bc6h.h): float32 texels -> 16-byte blocks in
// file order.  The per-block body is bc6h_body.h's, the tables bc6h_tables.h's.  Both kernels run ALL levels of ALL faces in one launch over a block
// index; Bc6hArgs carries the small per-level offset table (made on the host) that maps the index to level, face and position.
//   bc6h_q0_kernel   quality 0, mode 11 alone: one block per lane, 256-thread workgroups (BC6H_Q0_GROUP_BLOCKS blocks each).  The block's 48 half
//                    integers sit in 32 registers; the 16 palette entries are walked outside, the 16 texels inside, so that an entry is
//                    interpolated once; the 16 bytes leave as one 128-bit store.
//   bc6h_q1_kernel   quality 1: half a wave per block (BC6H_Q1_GROUP_BLOCKS = 8 blocks a workgroup), lane k of the half takes partition k in the
//                    feasible mode of highest precision, lane 0 mode 11 as well.  All 32 lanes load the same 16 texels (one address per load: a
//                    broadcast), read the partition's bitmap and the mode's layout from constant memory, and hold their candidate's 16 bytes; the
//                    least key (error, order) is found by five xor-shuffles inside the half, and the lane that owns it stores.  The lanes pack in
//                    lockstep: a pack by the winner alone would cost the wave the same instructions.
// No atomics, no LDS, no scratch.  A half wave past the last block repeats the last block and stores nothing, so that every shuffle has its 32 lanes.
// Included into de_api.hip's translation unit behind ibl_kernels.hip; no other kernel is touched.
#include "de_kernels.h"
#include "bc6h_body.h"

__global__ void __launch_bounds__(BC6H_THREADS) bc6h_q0_kernel(Bc6hArgs a) {
    const uint32_t b = blockIdx.x * BC6H_Q0_GROUP_BLOCKS + threadIdx.x;
    if (b >= a.total) return;
    uint32_t rg[16], bb[16], w[4];
    bc6h_load_block(a, b, rg, bb);
    bc6h_encode_q0(rg, bb, w);
    *reinterpret_cast<uint4*>(a.out + (size_t)b * 16) = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ void __launch_bounds__(BC6H_THREADS) bc6h_q1_kernel(Bc6hArgs a) {
    const uint32_t b = blockIdx.x * BC6H_Q1_GROUP_BLOCKS + threadIdx.x / BC6H_Q1_LANES, lane = threadIdx.x % BC6H_Q1_LANES;
    const uint32_t at = b < a.total ? b : a.total - 1u;
    uint32_t rg[16], bb[16], w[4], order;
    uint64_t err;
    bc6h_load_block(a, at, rg, bb);
    bc6h_lane_q1(rg, bb, lane, &err, &order, w);
    uint32_t best_hi = (uint32_t)(err >> 32), best_lo = (uint32_t)err, best_order = order;
    for (int step = 1; step < BC6H_Q1_LANES; step <<= 1) {
        const uint32_t hi = __shfl_xor(best_hi, step, BC6H_Q1_LANES), lo = __shfl_xor(best_lo, step, BC6H_Q1_LANES), o = __shfl_xor(best_order, step, BC6H_Q1_LANES);
        const bool less = hi < best_hi || (hi == best_hi && (lo < best_lo || (lo == best_lo && o < best_order)));
        if (less) { best_hi = hi; best_lo = lo; best_order = o; }
    }
    if (b < a.total && best_order == order) *reinterpret_cast<uint4*>(a.out + (size_t)b * 16) = make_uint4(w[0], w[1], w[2], w[3]);
}

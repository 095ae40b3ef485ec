// qs_state_blk.h - the wave-blocked state allocation of a handle: block layout (BlkOff, blkc), descriptor (StateBlk) and the element
// accessor for code outside the step kernels (blk_at / QS_BLK_AT).  Included by qs_state_rows.h and, alone, by qs_pilot.h.
#pragma once
#include <hip/hip_runtime.h>

#define QS_WAVE 64

// ------------------------------------------------------------------------------------------------
// device buffers
// ------------------------------------------------------------------------------------------------
// The per-drone arrays the step kernels touch every launch live in ONE allocation, so that the kernels address them through a
// single buffer resource: `buffer_load/store vdata, voffset(lane), srsrc, soffset(array + component)` needs one SALU add per
// access where a flat 64-bit address needs three VALU instructions (about 90 accesses per drone-step; the throughput
// regime of the single-wave kernels is VALU-bound).  The typed pointers below still point into the block.
// The per-drone state lives in ONE allocation, wave-blocked: block b holds the drones of the `epb` environments one wave steps
// (epb = 64 / N, lane = local env * N + drone), so that everything a wave loads and stores each step is one contiguous `block_bytes`
// chunk (11 KB in float32) instead of 42 rows scattered over 42 component-major arrays (tools/ubench_hbm.hip: 113.7 -> 97.6 us for
// 2^20 drones).  Inside a block the arrays follow each other - pos | vel | rot | omega | ... | flags | pair mask - and an
// array of `comps` components per drone has one of TWO element orders, fixed per handle (StateBlk::lane_major):
//   rows (0):       component-major, element (q, lane) at q * 64 + lane: every access is one 4-byte element per lane, 256 contiguous
//                   bytes per wave - 45 loads and 45 stores per block and step.  The single-wave throughput kernels and the 4-wave team
//                   kernels (N > 8) run on this order: in the bandwidth regime the narrow rows stream 1 % faster and leave the register
//                   allocator free of tuple constraints (tools/ubench_rowwidth.hip, profiles/r05l_ab_layout.txt).
//   lane-major (1): the components of one drone adjacent, element (q, lane) at lane * comps + q: a lane moves an array with ONE 12- or
//                   16-byte access (`buffer_load_dwordx3/x4`), 14 loads and 14 stores per block and step.  The specialised 8-wave team
//                   kernels (N <= 8: the latency regime of the headline) run on this order: wave 0 issues its loads in 240 instead of 600
//                   clocks and its stores in 250 instead of 400 (same microbenchmark); C2 7.82 -> 7.64 us per step.
// pos .. pair are byte offsets of an array INSIDE a block (the same for both orders); the per-step outputs (newpair, reward, done, ohit)
// stay flat component-major arrays behind the blocks (absolute offsets) - their consumers read them as plain vectors.
// bytes of one state block: 40 x 64 reals (pos 3, vel 3, rot 9, omega 3, rot_damp 4, cmds_damp 4, ou 4, goal 3, ring 4, sums 3), 64 flag
// words (u32), 64 pair masks (u64) - create_typed (quadswarm_hip.hip) lays the arrays out and checks this figure
static inline int qs_block_bytes(int real_size) { return 40 * 64 * real_size + 64 * 4 + 64 * 8; }
// byte offsets of the arrays inside a state block, in the order create_typed lays them out (it checks them)
template <typename real> struct BlkOff {
    static constexpr uint32_t row = 64 * sizeof(real);
    static constexpr uint32_t pos = 0, vel = 3 * row, rot = 6 * row, omega = 15 * row, rot_damp = 18 * row, cmds_damp = 22 * row,
        ou = 26 * row, goal = 30 * row,
                              ring = 33 * row, sums = 37 * row, flags = 40 * row, pair = 40 * row + 256, bytes = 40 * row + 768;
};
// components per drone of the blocked arrays (the lane pitch inside an array, in elements)
namespace blkc { constexpr int pos = 3, vel = 3, rot = 9, omega = 3, rot_damp = 4, cmds_damp = 4, ou = 4, goal = 3, ring = 4, sums = 3,
    flags = 1, pair = 1; }
struct StateBlk { char *base; uint32_t bytes, block_bytes, epb, pos, vel, rot, omega, rot_damp, cmds_damp, ou, goal, ring, sums, flags,
    pair, newpair, reward, done, ohit, lane_major; };
// element (component q of drone i of env e) of a blocked array of `comps` components, for the code outside the step kernels'
// buffer-resource views
template <typename TT> __device__ __forceinline__ TT &blk_at(const StateBlk &b, uint32_t arr, int comps, int q, int e, int i, int N) {
    const int blk = e / (int)b.epb, lane = (e - blk * (int)b.epb) * N + i;
    return *(TT *)(b.base + (size_t)blk * b.block_bytes + arr + (b.lane_major
        ? (size_t)lane * comps + q : (size_t)q * 64 + lane) * sizeof(TT));
}
#define QS_BLK_AT(TT, b, name, q, e, i, N) blk_at<TT>((b), (b).name, blkc::name, (q), (e), (i), (N))

// qs_step_debug.h - debug hooks of the step bodies, all empty in a plain build: the QS_TIMING phase stamps (tools/phase_timing.py,
// tools/wg_times.py) and the QS_POISON_IDLE garbage for idle lanes and unwritten LDS.  Included by qs_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#ifdef QS_TIMING
#define QS_STAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) p.timing[k] = clock64(); } while (0)
// helper waves of the team kernels: stamp k of wave w (1..3) lands in timing[32*w + k]
#define QS_STAMPW(k) do { if (blockIdx.x == 0 && (threadIdx.x & 63) == 0 && threadIdx.x >= 64) p.timing[32 * (threadIdx.x >> 6) + (k)] = clock64(); } while (0)
// start / end of EVERY workgroup (wave 0; s_memtime and the constant 100 MHz wall clock) and where it ran: HW_ID (gfx9: wave 3:0, simd 5:4,
// pipe 7:6, cu 11:8, sh 12, se 15:13) and XCC_ID
#define QS_WG_STRIDE 16
#define QS_STAMP_WG(k) do { if (threadIdx.x == 0) { p.timing[128 + QS_WG_STRIDE * blockIdx.x + (k)] = clock64(); p.timing[128 + QS_WG_STRIDE * blockIdx.x + 4 + (k)] = wall_clock64(); \
        if ((k) == 0) { p.timing[128 + QS_WG_STRIDE * blockIdx.x + 2] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11)); \
                        p.timing[128 + QS_WG_STRIDE * blockIdx.x + 3] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11)); } } } while (0)
// phase boundaries of EVERY workgroup's wave 0 (slots 6..15): which phase makes the slowest workgroup of a launch slow
#define QS_STAMP_WGK(k) do { if (threadIdx.x == 0) p.timing[128 + QS_WG_STRIDE * blockIdx.x + (k)] = clock64(); } while (0)
#else
#define QS_STAMP(k) do { } while (0)
#define QS_STAMPW(k) do { } while (0)
#define QS_STAMP_WG(k) do { } while (0)
#define QS_STAMP_WGK(k) do { } while (0)
#endif

// Debug builds (QS_SPEC_EXTRA_FLAGS="-DQS_POISON_IDLE=1|2 [-DQS_POISON_PARTS=mask]"; tests/test_object_identity_gpu.py): the lanes of a
// wave that own no drone - 64 % N of them, and every lane past the batch's last environment - start from garbage instead of a copy of drone
// 0 (1: NaN, 2: 3e30 in every float; all ones in flags and masks), and the dynamic LDS is filled with the same pattern before its first
// use.  Results must be bit-identical to the plain build's: nothing an active lane computes may depend on an idle lane's registers or on an
// LDS word that nobody wrote in this launch.  QS_POISON_PARTS (default: everything) picks what is poisoned, for bisecting: 1 drone state, 2
// flags / pair mask, 4 LDS, 8 actions, 16 goal / distance sums / ring.
#ifdef QS_POISON_IDLE
#ifndef QS_POISON_PARTS
#define QS_POISON_PARTS 31
#endif
// (opaque: fast-math would fold a literal NaN away)
__device__ __forceinline__ uint32_t qs_poison_bits() { uint32_t u = QS_POISON_IDLE == 1 ? 0x7fc0deadu : 0x7217e7d5u;
    asm volatile("" : "+v"(u)); return u; }
template <typename real> __device__ __forceinline__ real qs_poison() { return (real)__builtin_bit_cast(float, qs_poison_bits()); }
#define QS_POISON_LDS(total_bytes, nthreads) do { if (QS_POISON_PARTS & 4) { for (int w_ = threadIdx.x; w_ < (total_bytes) / 4; w_ += (nthreads)) ((uint32_t *)smem)[w_] = qs_poison_bits(); __syncthreads(); } } while (0)
#define QS_POISON_ARR_(a, n) do { if (!active) { _Pragma("unroll") for (int q_ = 0; q_ < (n); ++q_) (a)[q_] = qs_poison<real>(); } } while (0)
#define QS_POISON_ARR(a, n, part) do { if (QS_POISON_PARTS & (part)) QS_POISON_ARR_(a, n); } while (0)
#define QS_POISON_DRONE(d) do { if (QS_POISON_PARTS & 1) { QS_POISON_ARR_((d).pos, 3); QS_POISON_ARR_((d).vel, 3); QS_POISON_ARR_((d).rot, 9); QS_POISON_ARR_((d).omega, 3); \
                                QS_POISON_ARR_((d).rot_damp, 4); QS_POISON_ARR_((d).cmds_damp, 4); QS_POISON_ARR_((d).ou, 4); } if ((QS_POISON_PARTS & 2) && !active) (d).flags = ~0u; } while (0)
#define QS_POISON_U64(x) do { if ((QS_POISON_PARTS & 2) && !active) (x) = ~0ull; } while (0)
#else
#define QS_POISON_LDS(total_bytes, nthreads) do { } while (0)
#define QS_POISON_ARR(a, n, part) do { } while (0)
#define QS_POISON_DRONE(d) do { } while (0)
#define QS_POISON_U64(x) do { } while (0)
#endif

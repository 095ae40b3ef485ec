// qs_xchg_fused.h - the fused observation exchange of the one-step team kernels (the `_x` instantiations of qs_step_team.inc,
// float32): the protocol that used to be written out inside the step body.  fused_prefetch sits in the body's load phase, fused_push
// behind its observation copy-out; both are inlined into the kernel, with every value they use as an explicit parameter.  Types, flag
// accesses and write-through stores: qs_xchg_dev.h.  (qs_xchg_push_kernel, qs_exchange.hip, pushes staged rows to ONE destination per
// launch; here every lane stores to ALL destinations straight from LDS - different loops on purpose.)
#pragma once
#include "qs_xchg_dev.h"
#include "qs_obs_rows.h"   // qs_f32x4  (QS_TEAM_BARRIER: qs_kernels.h, which includes this file)

namespace qsx {

// The sequence number and the peers' acknowledgements, fetched under the step's state loads (both are uncached system-scope loads:
// ~2 us each if they sat in front of the epilogue).
__device__ __forceinline__ void fused_prefetch(const XchgDev *xchg, int wv, int tid, unsigned long long &xq_seq, unsigned long long &xq_ack) {
    if (xchg != nullptr) {
        // (+ 1 at its use in fused_push: an add in this branch would close it with s_waitcnt vmcnt(0), behind the 45 state loads)
        xq_seq = xchg->loc->push_seq;
        if (wv == 0 && tid < xchg->world) xq_ack = ld_sys(&xchg->mine->ack[tid]);
    }
}

// The workgroup's observation rows (s_obs: nenv * N rows of D floats, complete, behind barrier 6), in the wire type, into slot
// [seq & 1][rank] of EVERY rank's receive window (qs_set_obs_exchange, include/quadswarm_exchange.h) - peer stores over the
// point-to-point links straight from this workgroup's LDS stage, no extra launch.  Flow control and completion flags as in
// qs_xchg_push_kernel (qs_exchange.hip).  Whole workgroup of W waves; s_wire: wire_bytes of LDS that nothing else uses any more (the
// step's reward-term rows), the q8 wire's stage.
template <int W>
__device__ __forceinline__ void fused_push(const XchgDev *xchg, unsigned long long xq_seq, unsigned long long xq_ack, int wv, int tid,
    int first_env, int nenv, int N, int D, int K, int self_dim, const float *s_obs, unsigned int *s_wire, int wire_bytes) {
    if (xchg != nullptr) {
        const int total = nenv * N * D;
        const XchgDev &X = *xchg;
        const unsigned long long seq = xq_seq + 1;            // (push_seq is advanced by the last workgroup of a launch only)
        const int slot = (int)(seq & 1);
        if (wv == 0) {   // every destination must have released what this slot held before (seq - 2)
            bool ok = true;
            if (tid < X.world && seq > 2 && xq_ack < seq - 2) ok = poll_ge(&X.mine->ack[tid], seq - 2, X.timeout_ticks);
            if (__any(!ok) && tid == 0) atomicOr(&X.loc->status, (unsigned int)QS_XCHG_ERR_ACK_TIMEOUT);
        }
        __syncthreads();
        const size_t row0 = (size_t)first_env * N * D, wsz = X.wire == QS_WIRE_BF16 ? 2 : 4;
        const size_t off = X.wire == QS_WIRE_Q8 ? (size_t)slot * (size_t)X.slot_bytes + ((size_t)X.rank * (size_t)(X.n / D) + (size_t)first_env * N) * (size_t)X.q8.row_words * 4
                                                : (size_t)slot * (size_t)X.slot_bytes + ((size_t)X.rank * (size_t)X.n + row0) * wsz;
        const float *src = s_obs;
        const bool vec = ((total & 7) == 0) && ((off & 15) == 0);   // (the windows themselves are 256-byte aligned)
        // the narrow row: bf16 self / SDF columns + 8-bit fixed-point neighbour block (quadswarm_exchange.h)
        if (X.wire == QS_WIRE_Q8) {
            // The layout is rebuilt from the kernel's own constants (literals in a config-specialised object: the row / word index
            // arithmetic folds into multiplications by constants; qs_set_obs_exchange checks that the endpoint was created with
            // this layout) and the six scales are copied into registers: the stores below are `asm volatile` with a memory clobber,
            // so every field read through the descriptor pointer inside the loop would be a fresh load from device memory (a first
            // version did that and divided by a run-time row length: + 14.6 us per C4 step at world size 1 where bf16 costs + 3.8).
            const int q0 = self_dim, q1 = self_dim + 6 * K, w16 = (D - 6 * K + 1) >> 1;
            const float s0 = X.q8.s0, s1 = X.q8.s1, s2 = X.q8.s2, s3 = X.q8.s3, s4 = X.q8.s4, s5 = X.q8.s5;
            const int rw = w16 + ((6 * K + 3) >> 2), words = nenv * N * rw;
            // Two phases where the wire block fits the stage: every lane converts consecutive words into a staged copy of the block -
            // no volatile store in that loop, so its LDS reads and the arithmetic of several words overlap - then the block leaves
            // like the bf16 rows do, one 16-byte LDS read + one 16-byte store per lane and destination.
            if ((off & 15) == 0 && (words & 3) == 0 && words * 4 <= wire_bytes) {
                // (two uniform loops - the bf16 words of every row, then the int8 words - instead of one over all words: in a mixed
                // loop the lanes of a wave diverge between the two word kinds and every iteration pays for both)
                const int rows_here = nenv * N, n8w = rw - w16;
                for (int k = threadIdx.x; k < rows_here * w16; k += 64 * W) {
                    const int r = k / w16, j = k - r * w16;
                    s_wire[r * rw + j] = q8_row_word_v(src + r * D, D, q0, q1, w16, s0, s1, s2, s3, s4, s5, j);
                }
                for (int k = threadIdx.x; k < rows_here * n8w; k += 64 * W) {
                    const int r = k / n8w, j = w16 + (k - r * n8w);
                    s_wire[r * rw + j] = q8_row_word_v(src + r * D, D, q0, q1, w16, s0, s1, s2, s3, s4, s5, j);
                }
                QS_TEAM_BARRIER();
                for (int idx = threadIdx.x; idx < (words >> 2); idx += 64 * W) {
                    const u32x4_t ov = *(const u32x4_t *)(s_wire + 4 * idx);
                    for (int dd = 0; dd < X.world; ++dd) st16_wt(X.data_win[dd] + off + (size_t)idx * 16, ov);
                }
            // 16 bytes per lane and iteration: the volatile stores serialise the iterations, so few, fat ones
            } else if ((off & 15) == 0 && (words & 3) == 0) {
                for (int idx = threadIdx.x; idx < (words >> 2); idx += 64 * W) {
                    const int w0 = 4 * idx, r0 = w0 / rw;
                    int r = r0, j = w0 - r0 * rw;
                    unsigned int o[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        o[u] = q8_row_word_v(src + r * D, D, q0, q1, w16, s0, s1, s2, s3, s4, s5, j);
                        if (++j == rw) { j = 0; ++r; }
                    }
                    const u32x4_t ov = {o[0], o[1], o[2], o[3]};
                    for (int dd = 0; dd < X.world; ++dd) st16_wt(X.data_win[dd] + off + (size_t)idx * 16, ov);
                }
            } else {
#pragma unroll 1
                for (int w = threadIdx.x; w < words; w += 64 * W) {   // consecutive lanes = consecutive words of the wire block
                    const int r = w / rw;
                    const unsigned int o = q8_row_word_v(src + r * D, D, q0, q1, w16, s0, s1, s2, s3, s4, s5, w - r * rw);
                    for (int dd = 0; dd < X.world; ++dd) st4_wt(X.data_win[dd] + off + (size_t)w * 4, o);
                }
            }
        } else if (X.wire == QS_WIRE_BF16) {
            if (vec) {
                for (int idx = threadIdx.x; idx < (total >> 3); idx += 64 * W) {
                    const qs_f32x4 a = *(const qs_f32x4 *)(src + 8 * idx), b = *(const qs_f32x4 *)(src + 8 * idx + 4);
                    u32x4_t o;
                    o.x = f32_to_bf16_rne(a[0]) | (f32_to_bf16_rne(a[1]) << 16);
                    o.y = f32_to_bf16_rne(a[2]) | (f32_to_bf16_rne(a[3]) << 16);
                    o.z = f32_to_bf16_rne(b[0]) | (f32_to_bf16_rne(b[1]) << 16);
                    o.w = f32_to_bf16_rne(b[2]) | (f32_to_bf16_rne(b[3]) << 16);
                    for (int dd = 0; dd < X.world; ++dd) st16_wt(X.data_win[dd] + off + (size_t)idx * 16, o);
                }
            } else {
                for (int idx = threadIdx.x; idx < total; idx += 64 * W) {
                    const unsigned int o = f32_to_bf16_rne(src[idx]);
                    for (int dd = 0; dd < X.world; ++dd) st2_wt(X.data_win[dd] + off + (size_t)idx * 2, o);
                }
            }
        } else {
            if (vec) {
                for (int idx = threadIdx.x; idx < (total >> 2); idx += 64 * W) {
                    const qs_f32x4 a = *(const qs_f32x4 *)(src + 4 * idx);
                    const u32x4_t o = {__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]),
                        __float_as_uint(a[3])};
                    for (int dd = 0; dd < X.world; ++dd) st16_wt(X.data_win[dd] + off + (size_t)idx * 16, o);
                }
            } else {
                for (int idx = threadIdx.x; idx < total; idx += 64 * W)
                    for (int dd = 0; dd < X.world; ++dd) st4_wt(X.data_win[dd] + off + (size_t)idx * 4,
                        __float_as_uint(src[idx]));
            }
        }
        wt_drain();          // this thread's (write-through) rows have reached their windows ...
        __syncthreads();
        if (threadIdx.x == 0) {
            // fenced protocol: EVERY workgroup writes its XCD's L2 back before it takes its ticket
            fence_release_sys(X.fenced);
            const unsigned int tk = atomicAdd(&X.loc->ticket_all, 1u);
            if (tk == X.blocks - 1) {   // ... and this is the last workgroup of the launch: raise the flags
                X.loc->ticket_all = 0;
                for (int dd = 0; dd < X.world; ++dd) st_sys(&X.flag_win[dd]->arrive[slot][X.rank], seq);
                X.loc->push_seq = seq;
                if (X.auto_ack) {   // no in-place reader: wait for the rows of every OTHER rank, then hand the slot back
                    bool ok = true;
                    for (int r = 0; r < X.world; ++r) if (r != X.rank) ok &= poll_ge(&X.mine->arrive[slot][r], seq,
                        X.timeout_ticks);
                    if (!ok) atomicOr(&X.loc->status, (unsigned int)QS_XCHG_ERR_ARRIVE_TIMEOUT);
                    fence_acquire_sys(X.fenced);
                    for (int dd = 0; dd < X.world; ++dd) st_sys(&X.flag_win[dd]->ack[X.rank], seq);
                    X.loc->wait_seq = seq; X.loc->release_seq = seq;
                }
            }
        }
    }
}

}   // namespace qsx

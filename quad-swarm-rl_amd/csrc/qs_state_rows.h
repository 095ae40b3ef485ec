// qs_state_rows.h - what a step / reset kernel is handed of a handle's device memory (Ptrs) and its view of one array of the state
// allocation from one lane (BufRow, QS_ROW / QS_ROWF: buffer-resource loads and stores).  Included by qs_kernels.h.
#pragma once
#include "qs_state_blk.h"
#include "qs_xchg_dev.h"

template <typename real> struct Ptrs {
    StateBlk blk;
    real *pos, *vel, *rot, *omega, *rot_damp, *cmds_damp, *ou, *goal;
    uint32_t *flags;
    uint64_t *pair_mask, *new_pair_mask;
    real *obs, *reward, *rew_info;
    uint8_t *done;
    int32_t *obst_hit_idx;
    uint64_t *unique_col, *obst_new, *room_new;
    int32_t *counters, *tick;
    uint32_t *step_ctr;
    real *obst_pos;
    real *dist_ring, *dist_sums;
    real *ep_stats;
    int32_t *ep_counters;
    real *scen_real;
    int32_t *scen_int;
    uint32_t *error_flag;
    uint64_t *scen_omap;   // [4, E] obstacle map bitsets (scenarios that sample free cells during an episode)
    int32_t *scenario_id;  // [E] active scenario (the sub-scenario under `mix`)
    int32_t *ep_scenario;  // [E] scenario of the last finished episode
    real *run_sums, *ep_sums;   // [QS_SUM_COUNT, T] per-episode sums (running / last finished episode)
    int32_t *obst_count;   // [E] obstacles of the running episode (domain randomisation; the other slots are parked far away)
    real *obst_size_env, *obst_density_env;   // [E] obstacle size / density of the running episode
    const int32_t *dr_count;                  // [QS_MAX_DR_CHOICES] --quads_domain_random choice tables: obstacle count,
    const real *dr_density, *dr_size;         //                     density, size
    uint8_t *reset_mask;   // [E] nonzero => reset kernel re-initialises this env
    unsigned long long *timing;   // [32] phase time stamps of workgroup 0 (only written by -DQS_TIMING builds)
    const real *rew_rt;   // [QS_REW_COUNT + 1] run-time reward coefficients + proximity slope (qs_set_reward_coeffs)
    const qsx::XchgDev *xchg;   // qs_set_obs_exchange: the team step kernels also store their observation rows into every rank's window
    // noise tape (qs_set_noise_tape; consumed by the QS_TAPE kernels only): [E][tape_len] reference draws, per-env cursor
    const double *tape;
    int32_t *tape_pos;
    int64_t tape_len;
};

// One array of the state allocation seen from one lane: element type T; `off` = scalar offset of the array (for a blocked array: of this
// wave's block too), `lane_off` = this lane's first byte inside it, `comp_bytes` = bytes between the components of one lane (a blocked
// array: sizeof(T) in the lane-major order, a row of 64 elements otherwise; a flat component-major array: its row pitch), `wide` = the
// lane's components are adjacent and ldv / stv may move them as 12- / 16-byte pieces.
typedef unsigned int qs_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int qs_u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int qs_u32x4 __attribute__((ext_vector_type(4)));
template <typename T> struct BufRow {
    __amdgpu_buffer_rsrc_t r;
    uint32_t off, comp_bytes, lane_off;
    bool wide;
    __device__ __forceinline__ T ld(int q = 0) const {
        if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T,
            __builtin_amdgcn_raw_buffer_load_b64(r, lane_off, off + (uint32_t)q * comp_bytes, 0));
        else return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(r, lane_off, off + (uint32_t)q * comp_bytes, 0));
    }
    __device__ __forceinline__ void st(T v, int q = 0) const {
        if constexpr (sizeof(T) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(qs_u32x2, v), r, lane_off,
            off + (uint32_t)q * comp_bytes, 0);
        else if constexpr (sizeof(T) == 4) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, lane_off,
            off + (uint32_t)q * comp_bytes, 0);
        else __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v, r, lane_off, off + (uint32_t)q * comp_bytes, 0);
    }
    // the D dwords from byte `at` of this lane's piece of a lane-major array, as the widest accesses that cover them (16, 12, 8, 4 bytes)
    template <int D> __device__ __forceinline__ void ld_dwords(uint32_t *w, uint32_t at) const {
        if constexpr (D >= 4) { const qs_u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(r, lane_off, off + at, 0); w[0] = x.x;
            w[1] = x.y; w[2] = x.z; w[3] = x.w; if constexpr (D > 4) ld_dwords<D - 4>(w + 4, at + 16); }
        else if constexpr (D == 3) { const qs_u32x3 x = __builtin_amdgcn_raw_buffer_load_b96(r, lane_off, off + at, 0); w[0] = x.x;
            w[1] = x.y; w[2] = x.z; }
        else if constexpr (D == 2) { const qs_u32x2 x = __builtin_amdgcn_raw_buffer_load_b64(r, lane_off, off + at, 0); w[0] = x.x;
            w[1] = x.y; }
        else w[0] = __builtin_amdgcn_raw_buffer_load_b32(r, lane_off, off + at, 0);
    }
    template <int D> __device__ __forceinline__ void st_dwords(const uint32_t *w, uint32_t at) const {
        if constexpr (D >= 4) { const qs_u32x4 x = {w[0], w[1], w[2], w[3]};
            __builtin_amdgcn_raw_buffer_store_b128(x, r, lane_off, off + at, 0); if constexpr (D > 4) st_dwords<D - 4>(w + 4, at + 16); }
        else if constexpr (D == 3) { const qs_u32x3 x = {w[0], w[1], w[2]};
            __builtin_amdgcn_raw_buffer_store_b96(x, r, lane_off, off + at, 0); }
        else if constexpr (D == 2) { const qs_u32x2 x = {w[0], w[1]}; __builtin_amdgcn_raw_buffer_store_b64(x, r, lane_off, off + at, 0); }
        else __builtin_amdgcn_raw_buffer_store_b32(w[0], r, lane_off, off + at, 0);
    }
    // all K components of this lane's drone (blocked arrays: K = the array's component count)
    template <int K> __device__ __forceinline__ void ldv(T *dst) const {
        if (!wide) {
#pragma unroll
            for (int k = 0; k < K; ++k) dst[k] = ld(k);
            return;
        }
        constexpr int D = K * (int)sizeof(T) / 4;
        uint32_t w[D];
        ld_dwords<D>(w, 0);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if constexpr (sizeof(T) == 8) dst[k] = __builtin_bit_cast(T, (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32));
            else dst[k] = __builtin_bit_cast(T, w[k]);
        }
    }
    template <int K> __device__ __forceinline__ void stv(const T *src) const {
        if (!wide) {
#pragma unroll
            for (int k = 0; k < K; ++k) st(src[k], k);
            return;
        }
        constexpr int D = K * (int)sizeof(T) / 4;
        uint32_t w[D];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if constexpr (sizeof(T) == 8) { const uint64_t u = __builtin_bit_cast(uint64_t, src[k]); w[2 * k] = (uint32_t)u;
                w[2 * k + 1] = (uint32_t)(u >> 32); }
            else w[k] = __builtin_bit_cast(uint32_t, src[k]);
        }
        st_dwords<D>(w, 0);
    }
};
#define QS_BUF_RSRC(p) __builtin_amdgcn_make_buffer_rsrc((void *)(p).blk.base, 0, (p).blk.bytes, 0x00020000)
// blocked state array: the workgroup's block (blockIdx.x: one block = the environments of one workgroup), lane = position inside the wave;
// component offsets are compile-time constants next to the scalar block offset.  QS_LM: the element order of the handle's blocks - a
// literal in a config-specialised object (lane-major <=> the 8-wave team kernels), the handle's flag in the generic kernels
#define QS_BLK blockIdx.x
#if defined(QS_SPEC_TEAM)
#define QS_LM(p) (QS_SPEC_TEAM == 8)
#else
#define QS_LM(p) ((p).blk.lane_major != 0)
#endif
#define QS_ROW(TYPE, name, rs, p, T, g) const BufRow<TYPE> b_##name = {rs, (uint32_t)(QS_BLK * (p).blk.block_bytes + (p).blk.name), (uint32_t)((QS_LM(p) ? 1 : 64) * sizeof(TYPE)), \
                                                                       (uint32_t)((threadIdx.x & 63) * ((QS_LM(p) ? blkc::name : 1) * sizeof(TYPE))), QS_LM(p)}
// The per-environment rows of every step - collision id sets (64-bit: two rows each), the counters, tick, noise-stream position - are ONE
// allocation of QS_ENVROW_COUNT rows of E 32-bit words that starts at Ptrs::unique_col (create_typed): a second buffer resource with one scalar
// row offset and the lane's env offset per access (the team kernels' one-step body; every other kernel uses the typed pointers).
#define QS_ENVROW_unique 0
#define QS_ENVROW_obst_new 2
#define QS_ENVROW_room_new 4
#define QS_ENVROW_counters 6
#define QS_ENVROW_tick (6 + QS_CNT_COUNT)
#define QS_ENVROW_step_ctr (7 + QS_CNT_COUNT)
#define QS_ENVROW_COUNT (8 + QS_CNT_COUNT)
#define QS_ENV_RSRC(p, E) __builtin_amdgcn_make_buffer_rsrc((void *)(p).unique_col, 0, (uint32_t)(QS_ENVROW_COUNT * 4) * (uint32_t)(E), 0x00020000)
#define QS_ROWE(TYPE, name, rs, E, e) const BufRow<TYPE> b_##name = {rs, (uint32_t)(QS_ENVROW_##name * 4) * (uint32_t)(E), 4u * (uint32_t)(E), (uint32_t)((e) * sizeof(TYPE)), false}
// flat component-major array (per-step outputs): row pitch T elements, lane offset = global drone index
#define QS_ROWF(TYPE, name, rs, p, T, g) const BufRow<TYPE> b_##name = {rs, (p).blk.name, (uint32_t)((T) * sizeof(TYPE)), (uint32_t)((g) * sizeof(TYPE)), false}

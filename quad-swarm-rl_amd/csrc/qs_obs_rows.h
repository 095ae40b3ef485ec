// qs_obs_rows.h - how observation rows leave the workgroup: the row stores (obs_st*), the copy of complete rows out of LDS
// (obs_copy_rows), the obstacle SDF columns (sdf_obs) and the single-wave kernels' staged row output (stream_rows).  Included by
// qs_kernels.h for the step bodies and the reset.
#pragma once
#include "qs_lds_layout.h"
#include "qs_nbr_obs.h"

// ------------------------------------------------------------------------------------------------
// Observation output of the single-wave kernels: rows [r0, r0 + nr) of the workgroup's block, complete, to the row-major
// observation matrix - self columns from the dense self block, the others from the rows stage.  Consecutive lanes write
// consecutive words: every store instruction is one contiguous run.  rowmask (bit = row within the block) selects the rows to
// write (an auto-reset rewrites only the rows of the finished environments).  Whole wave, between barriers.
// ------------------------------------------------------------------------------------------------
// Cache policy of the observation rows' stores.  They are write-once per step and not read again by the stepper (42 % of a step's
// bytes): non-temporal (`nt`), so that they do not displace the state rows - which the next step re-reads - from the 256 MiB
// Infinity Cache.  Measured on MI355X against plain stores, C2 shape at 131072 envs (539 MB per step): 132.2 -> 107.0 us per step,
// 0.50 -> 0.61 of 8 TB/s, same FETCH_SIZE / WRITE_SIZE (profiles/r03b_nt_obs_E131072.txt).
typedef float qs_f32x2 __attribute__((ext_vector_type(2)));
typedef float qs_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void obs_st2(float *dst, qs_f32x2 v) { __builtin_nontemporal_store(v, (qs_f32x2 *)dst); }
__device__ __forceinline__ void obs_st4(float *dst, qs_f32x4 v) { __builtin_nontemporal_store(v, (qs_f32x4 *)dst); }
template <typename real> __device__ __forceinline__ void obs_st1(real *dst, real v) { __builtin_nontemporal_store(v, dst); }

template <typename real>
__device__ __forceinline__ void obs_copy_rows(real *__restrict__ dst_block, const real *s_self, const real *s_rows, int S, int D, int r0,
    int nr, uint64_t rowmask, int tid) {
    const int X = D - S;
    real *dst = dst_block + (size_t)r0 * D;
    if (sizeof(real) == 4 && ((D | S) & 1) == 0) {   // 8-byte elements: rows (D*4 bytes) and the self / other boundary stay 8-byte aligned
        const int half = D >> 1, total = nr * half;
        for (int idx = tid; idx < total; idx += QS_WAVE) {
            const int row = idx / half, c2 = 2 * (idx - row * half);
            const float *src = (c2 < S) ? (const float *)s_self + (r0 + row) * S + c2 : (const float *)s_rows + row * X + (c2 - S);
            if ((rowmask >> (r0 + row)) & 1) obs_st2((float *)dst + 2 * idx, *(const qs_f32x2 *)src);
        }
    } else {
        const int total = nr * D;
        for (int idx = tid; idx < total; idx += QS_WAVE) {
            const int row = idx / D, cc = idx - row * D;
            const real v = (cc < S) ? s_self[(r0 + row) * S + cc] : s_rows[row * X + (cc - S)];
            if ((rowmask >> (r0 + row)) & 1) obs_st1<real>(dst + idx, v);
        }
    }
}

// get_surround_sdfs obstacles/utils.py:5-27 (obstacle xy of the env in LDS)
template <typename real>
__device__ __forceinline__ void sdf_obs(const Consts<real> &c, const real *ox, const real *oy, int M_, real px, real py, real *o,
    real radius) {
    const real res = (real)0.1;
    real gx[3] = {px - res, px, px + res}, gy[3] = {py - res, py, py + res};
    // min over the obstacles of the SQUARED distance, one square root per cell at the end: the square root is monotone, so
    // min_k sqrt(d2_k) == sqrt(min_k d2_k) - 9 instead of 9 * M quarter-rate v_sqrt_f32 per drone and step (the reference's start value
    // 100.0, utils.py:17, is the cap 100^2 on the squared side)
    real mind2[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) mind2[q] = (real)10000;
    for (int k = 0; k < M_; ++k) {
        real x = ox[k], y = oy[k];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                real dx = gx[a] - x, dy = gy[b] - y, d2 = dx * dx + dy * dy;
                mind2[a * 3 + b] = d2 < mind2[a * 3 + b] ? d2 : mind2[a * 3 + b];
            }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) o[q] = M<real>::sqrt(mind2[q]) - radius;
}

// The neighbour and SDF columns of the wave's rows -> rows stage -> HBM together with the self columns (obs_copy_rows), one row
// group at a time.  Whole wave; `live` lanes compute (their rows are the ones in rowmask).  The stage shares LDS with the
// rare-path buffers: nothing of those may be live here; ends with the stage free again (RP < 64) or still being read (RP = 64:
// the caller's next barrier).
template <typename real>
__device__ __forceinline__ void stream_rows(const Consts<real> &c, const LdsLayout &L, real *__restrict__ dst_block, const real *s_self,
    real *s_rows, int N, int i, int le, int base, int tid,
                                            const real *s_pos, const real *s_vel, real *s_metric, const real *s_obst,
                                                const real mypos[3], const real myvel[3],
                                            bool live, int nrows, uint64_t rowmask, real obst_radius) {
    const int B = QS_WAVE, K = c.num_neighbors, D = c.obs_dim, S = c.self_dim, X = D - S, M_ = c.num_obstacles, RP = L.rows_per_pass;
    NbrSel<real> sel;
    if (live) nbr_select<real>(c, N, i, base, B, tid, s_pos, s_vel, s_metric, mypos, myvel, sel);
#ifdef QS_SPEC
    if (RP < B) {   // (config-specialised kernels only: X is a literal <= QS_NV_MAX, the register array below has static indices)
        real nv[QS_NV_MAX];
        if (live) {
            nbr_emit<real>(c, N, i, base, B, tid, s_pos, s_vel, s_metric, mypos, myvel, sel, 0, K, nv);
            if (c.use_obstacles) sdf_obs<real>(c, s_obst + (le * 2 + 0) * M_, s_obst + (le * 2 + 1) * M_, M_, mypos[0], mypos[1],
                nv + 6 * K, obst_radius);
        }
        for (int r0 = 0; r0 < nrows; r0 += RP) {
            if (live && tid >= r0 && tid < r0 + RP) {
                real *o = s_rows + (tid - r0) * X;
#pragma unroll
                for (int q = 0; q < QS_NV_MAX; ++q) if (q < X) o[q] = nv[q];
            }
            __syncthreads();
            obs_copy_rows<real>(dst_block, s_self, s_rows, S, D, r0, (nrows - r0) < RP ? (nrows - r0) : RP, rowmask, tid);
            __syncthreads();   // the group has left the stage
        }
        return;
    }
#endif
    if (live) {   // complete rows at once: straight into the stage
        real *o = s_rows + tid * X;
        nbr_emit<real>(c, N, i, base, B, tid, s_pos, s_vel, s_metric, mypos, myvel, sel, 0, K, o);
        if (c.use_obstacles) sdf_obs<real>(c, s_obst + (le * 2 + 0) * M_, s_obst + (le * 2 + 1) * M_, M_, mypos[0], mypos[1], o + 6 * K,
            obst_radius);
    }
    __syncthreads();
    obs_copy_rows<real>(dst_block, s_self, s_rows, S, D, 0, nrows, rowmask, tid);
}

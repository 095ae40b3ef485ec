// qs_nbr_obs.h - the neighbour columns of a drone's observation: the (metric, index) keys and the one metric every site ranks by, the
// K-nearest selection and emission in its forms (neighbor_obs, nbr_select + nbr_emit) and the team kernels' local ranking
// (team_rank_local).  Included by qs_obs_rows.h, and through it by the step bodies and the reset.
#pragma once
#include "qs_device.h"

using namespace qs;

// (neighbour metric, drone index) as one unsigned key whose order is "smaller metric first, lower index first": the IEEE bit
// pattern of a float is monotone after flipping the sign bit of non-negatives and all bits of negatives
__device__ __forceinline__ unsigned long long nbr_key(float m, int idx) {
    const uint32_t b = __float_as_uint(m), o = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
    return ((unsigned long long)o << 32) | (uint32_t)idx;
}

// neighbour metric of neighborhood_indices (quadrotor_multi.py:247-274) for the relative position rp / velocity rv of a partner:
// max(|rp|, 0.01) + rp.rv / that.  Symmetric in the pair - (-rp).(-rv) = rp.rv and |-rp| = |rp| exactly in IEEE arithmetic - which is
// what lets the team kernels evaluate every unordered pair once.  ONE definition for every site that ranks neighbours.
template <typename real> __device__ __forceinline__ real nbr_metric(const real rp[3], const real rv[3]) {
    const real rd = M<real>::fmax(norm3<real>(rp), (real)0.01);
    return rd + (rp[0] * rv[0] + rp[1] * rv[1] + rp[2] * rv[2]) * M<real>::rcp(rd);
}
// fp32: the multiply-add chain written out (the one the compiler forms from the expression above), so that the two-partners-at-once form
// below (v_pk_mul / v_pk_fma_f32: both halves round like the scalar instruction) gives the same bits as this one
template <> __device__ __forceinline__ float nbr_metric<float>(const float rp[3], const float rv[3]) {
    const float d2 = __builtin_fmaf(rp[2], rp[2], __builtin_fmaf(rp[1], rp[1], rp[0] * rp[0]));
    const float dot = __builtin_fmaf(rp[2], rv[2], __builtin_fmaf(rp[1], rv[1], rp[0] * rv[0]));
    const float rd = fmaxf(__builtin_amdgcn_sqrtf(d2), 0.01f);
    return __builtin_fmaf(dot, __builtin_amdgcn_rcpf(rd), rd);
}
typedef float qs_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ qs_f32x2 nbr_metric_x2(const qs_f32x2 rp[3], const qs_f32x2 rv[3]) {
    const qs_f32x2 d2 = __builtin_elementwise_fma(rp[2], rp[2], __builtin_elementwise_fma(rp[1], rp[1], rp[0] * rp[0]));
    const qs_f32x2 dot = __builtin_elementwise_fma(rp[2], rv[2], __builtin_elementwise_fma(rp[1], rv[1], rp[0] * rv[0]));
    const qs_f32x2 rd = {fmaxf(__builtin_amdgcn_sqrtf(d2.x), 0.01f), fmaxf(__builtin_amdgcn_sqrtf(d2.y), 0.01f)};
    const qs_f32x2 rc = {__builtin_amdgcn_rcpf(rd.x), __builtin_amdgcn_rcpf(rd.y)};
    return __builtin_elementwise_fma(dot, rc, rd);
}
// (metric, index) with the order "smaller metric first, lower index first" = position in the stable argsort
template <typename real> struct NbrKey;
template <> struct NbrKey<float> {
    unsigned long long k;
    static __device__ __forceinline__ NbrKey make(float m, int j) { return {nbr_key(m, j)}; }
    __device__ __forceinline__ bool less(const NbrKey &o) const { return k < o.k; }
    __device__ __forceinline__ int idx() const { return (int)(uint32_t)k; }
    // LDS list entry `slot` of lane tid: keys [slots][B]
    static __device__ __forceinline__ void st(unsigned char *base, int slots, int slot, int B, int tid,
        const NbrKey &v) { ((unsigned long long *)base)[slot * B + tid] = v.k; }
    static __device__ __forceinline__ NbrKey ld(const unsigned char *base, int slots, int slot, int B,
        int tid) { return {((const unsigned long long *)base)[slot * B + tid]}; }
};
template <> struct NbrKey<double> {
    double m; int j;
    static __device__ __forceinline__ NbrKey make(double m, int j) { return {m, j}; }
    __device__ __forceinline__ bool less(const NbrKey &o) const { return (m < o.m) | ((m == o.m) & (j < o.j)); }
    __device__ __forceinline__ int idx() const { return j; }
    // metrics [slots][B] doubles, then indices [slots][B] ints
    static __device__ __forceinline__ void st(unsigned char *base, int slots, int slot, int B, int tid, const NbrKey &v) {
        ((double *)base)[slot * B + tid] = v.m; ((int *)(base + (size_t)slots * B * 8))[slot * B + tid] = v.j; }
    static __device__ __forceinline__ NbrKey ld(const unsigned char *base, int slots, int slot, int B, int tid) {
        return {((const double *)base)[slot * B + tid], ((const int *)(base + (size_t)slots * B * 8))[slot * B + tid]}; }
};

// ------------------------------------------------------------------------------------------------
// K-nearest neighbour observation for one drone (neighborhood_indices quadrotor_multi.py:247-274,
// extend_obs_space :233-245).  pos/vel of the env's drones are in LDS (component-major, stride B).
// The N-1 metrics are evaluated once into an LDS row, then K rounds of arg-min (lowest index wins ties,
// like the stable ordering of argsort on distinct keys).
// ------------------------------------------------------------------------------------------------
// neighborhood_indices quadrotor_multi.py:247-274 + extend_obs_space :233-245.
// pos/vel of the env's drones are in LDS (component-major, stride B).  Measured on MI355X (lone wave per SIMD, every
// LDS round trip exposed): N <= 8 is fastest with all candidates in registers and rank-by-counting (independent
// compares); larger N with a streaming sorted top-K list (insertion by compare-exchange).  Both give the first K
// entries of the stable ascending order of the metric = argsort.
template <typename real>
__device__ __forceinline__ void neighbor_obs(const Consts<real> &c, int N, int i, int base, int B, int tid, const real *s_pos,
    const real *s_vel,
                                             real *s_metric, const real mypos[3], const real myvel[3], real *o) {
    const int K = c.num_neighbors;
    if (K <= 0) return;
    if (K == N - 1 || N <= 8) {
        const bool all_others = (K == N - 1);   // all other drones in index order (:253-254)
        for (int j0 = 0; j0 < N; j0 += 8) {      // (a single chunk unless all_others with N > 8)
            real rp[8][3], rv[8][3];
            int rank[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {        // 48 LDS reads issued before the first use: one round trip
                const int j = (j0 + u < N) ? j0 + u : N - 1;
#pragma unroll
                for (int a = 0; a < 3; ++a) { rp[u][a] = s_pos[a * B + base + j] - mypos[a];
                    rv[u][a] = s_vel[a * B + base + j] - myvel[a]; }
            }
            if (all_others) {
#pragma unroll
                for (int u = 0; u < 8; ++u) rank[u] = (j0 + u < i) ? j0 + u : j0 + u - 1;
            } else {
                real mj[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    real rd = M<real>::fmax(norm3<real>(rp[u]), (real)0.01);
                    real m = rd + (rp[u][0] * rv[u][0] + rp[u][1] * rv[u][1] + rp[u][2] * rv[u][2]) * M<real>::rcp(rd);
                    mj[u] = (u < N && u != i) ? m : (real)3.4e38;
                    rank[u] = 0;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
#pragma unroll
                    for (int u = 0; u < 8; ++u) rank[u] += (int)((mj[k] < mj[u]) | ((mj[k] == mj[u]) & (k < u)));
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u;
                if (j < N && j != i && rank[u] < K) {
                    real *oo = o + rank[u] * 6;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        oo[a] = clipr<real>(rp[u][a], -c.nbr_clip_pos[a], c.nbr_clip_pos[a]);
                        oo[3 + a] = clipr<real>(rv[u][a], -c.nbr_clip_vel[a], c.nbr_clip_vel[a]);
                    }
                }
            }
        }
        return;
    }
    if (K <= 8) {
        // streaming pass over the candidates, 4 per LDS round trip; sorted top-8 (metric, index) list in registers.  A new
        // candidate is inserted behind entries with an equal metric, i.e. lower index first.
        real bm[8];
        int bi[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { bm[k] = (real)3.4e38; bi[k] = 0; }
        for (int j0 = 0; j0 < N; j0 += 4) {
            real rp[4][3], rv[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = (j0 + u < N) ? j0 + u : N - 1;
#pragma unroll
                for (int a = 0; a < 3; ++a) { rp[u][a] = s_pos[a * B + base + j] - mypos[a];
                    rv[u][a] = s_vel[a * B + base + j] - myvel[a]; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                real rd = M<real>::fmax(norm3<real>(rp[u]), (real)0.01);
                real m = rd + (rp[u][0] * rv[u][0] + rp[u][1] * rv[u][1] + rp[u][2] * rv[u][2]) * M<real>::rcp(rd);
                m = (j < N && j != i) ? m : (real)3.4e38;
                int mi = j;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const bool lt = m < bm[k];
                    const real tm = lt ? bm[k] : m;
                    const int ti = lt ? bi[k] : mi;
                    bm[k] = lt ? m : bm[k];
                    bi[k] = lt ? mi : bi[k];
                    m = tm; mi = ti;
                }
            }
        }
        real vals[8][6];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < K) {
#pragma unroll
                for (int a = 0; a < 3; ++a) { vals[k][a] = s_pos[a * B + base + bi[k]] - mypos[a];
                    vals[k][3 + a] = s_vel[a * B + base + bi[k]] - myvel[a]; }
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < K) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    o[k * 6 + a] = clipr<real>(vals[k][a], -c.nbr_clip_pos[a], c.nbr_clip_pos[a]);
                    o[k * 6 + 3 + a] = clipr<real>(vals[k][3 + a], -c.nbr_clip_vel[a], c.nbr_clip_vel[a]);
                }
            }
        }
        return;
    }
    // 8 < K < N-1 (unusual): metrics into this lane's LDS column, then K rounds of arg-min (lowest index wins ties)
    for (int j = 0; j < N; ++j) {
        real rp[3] = {s_pos[0 * B + base + j] - mypos[0], s_pos[1 * B + base + j] - mypos[1], s_pos[2 * B + base + j] - mypos[2]};
        real rv[3] = {s_vel[0 * B + base + j] - myvel[0], s_vel[1 * B + base + j] - myvel[1], s_vel[2 * B + base + j] - myvel[2]};
        real rd = M<real>::fmax(norm3<real>(rp), (real)0.01);
        real mm = rd + (rp[0] * rv[0] + rp[1] * rv[1] + rp[2] * rv[2]) * M<real>::rcp(rd);
        s_metric[j * B + tid] = (j == i) ? (real)3.4e38 : mm;
    }
    uint64_t taken = 1ull << i;
    for (int k = 0; k < K; ++k) {
        int best = -1;
        real bmin = (real)3.4e38;
        for (int j = 0; j < N; ++j) {
            real mm = s_metric[j * B + tid];
            bool better = !(taken >> j & 1) && (best < 0 || mm < bmin);
            best = better ? j : best;
            bmin = better ? mm : bmin;
        }
        taken |= 1ull << best;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o[k * 6 + a] = clipr<real>(s_pos[a * B + base + best] - mypos[a], -c.nbr_clip_pos[a], c.nbr_clip_pos[a]);
            o[k * 6 + 3 + a] = clipr<real>(s_vel[a * B + base + best] - myvel[a], -c.nbr_clip_vel[a], c.nbr_clip_vel[a]);
        }
    }
}

// K-nearest neighbour selection of one drone, split into "select once" + "emit the neighbours of ranks [k0, k1)" so that the
// rows can be staged a few neighbours at a time (same four cases and the same results as neighbor_obs above).
template <typename real> struct NbrSel {
    int bi[8];                 // K <= 8: indices of the (up to 8) nearest in order
    uint64_t taken;            // 8 < K < N-1: drones already emitted (arg-min rounds over the LDS metric column)
};
// fp32, K <= 8: the sorted top-(K + 1) list as ONE 32-bit integer key per entry - the metric's order-preserving bit pattern with its low
// IB bits replaced by the drone index - so that the insertion is one v_med3_i32 per slot (new[k] = med3(cand, old[k-1], old[k]) of a
// sorted list) instead of a compare and four selects.  The truncation is monotone, so two entries with DIFFERENT truncated metrics are
// in the exact order; wherever the exact (metric, index) order could differ from the key order - inside the first K, or across the
// K / K+1 boundary - two neighbouring entries of the sorted first K + 1 share a truncated metric, which is what the return value
// reports (false = within 2^IB ulps of a tie: the caller takes the exact path; ~1e-4 of the drones).  IB = bits of a drone index.
__device__ __forceinline__ int qs_med3_i32(int a, int b, int c) {
    int r; asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
}
// the key list of one drone: K + 1 sorted entries (9 slots for K <= 8), the index / truncation masks
struct NbrKeys {
    int key[9];
    int IM, TM;
    __device__ __forceinline__ void init(int N) {
        const int IB = N <= 8 ? 3 : (N <= 16 ? 4 : (N <= 32 ? 5 : 6));
        IM = (1 << IB) - 1;
#ifdef QS_NBR_TRUNC_BITS   // (tests: a wider truncation than the index needs - the exact path is taken often, inside the same waves)
        TM = (1 << QS_NBR_TRUNC_BITS) - 1;
#else
        TM = IM;
#endif
#pragma unroll
        for (int k = 0; k < 9; ++k) key[k] = 0x7fffffff;
    }
    // candidate j with metric m (valid: a partner, i.e. j < N and j != i)
    __device__ __forceinline__ void insert(float m, int j, bool valid, int K) {
        const int b = __float_as_int(m);
        int cand = ((b ^ ((b >> 31) & 0x7fffffff)) & ~TM) | (j & IM);   // signed order = float order; -inf-wards truncation
        cand = valid ? cand : ((0x7fffffff & ~TM) | (j & IM));
        int below = key[0];
        key[0] = cand < key[0] ? cand : key[0];
#pragma unroll
        for (int k = 1; k < 9; ++k)   // (K is a literal in the specialised objects: K + 1 slots)
            if (k <= K) { const int nk = qs_med3_i32(cand, below, key[k]); below = key[k]; key[k] = nk; }
    }
    // indices of the K nearest in order; false: two neighbouring entries of the first K + 1 share a truncated metric
    __device__ __forceinline__ bool finish(int K, int bi[8]) const {
        uint32_t closest = 0xffffffffu;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t x = (uint32_t)(key[k] ^ key[k + 1]);
            closest = (k < K && x < closest) ? x : closest;
            bi[k] = key[k] & IM;
        }
        return closest > (uint32_t)TM;
    }
};
template <typename real>
__device__ __forceinline__ bool nbr_select_keys(const Consts<real> &c, int N, int i, int base, int B, const real *s_pos, const real *s_vel,
                                                const real mypos[3], const real myvel[3], int bi[8]) {
    const int K = c.num_neighbors;
    NbrKeys L;
    L.init(N);
    for (int j0 = 0; j0 < N; j0 += 4) {
        float m4[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {   // two partners per packed instruction (neighbouring LDS words = an aligned register pair)
            const int ja = (j0 + 2 * h < N) ? j0 + 2 * h : N - 1, jb = (j0 + 2 * h + 1 < N) ? j0 + 2 * h + 1 : N - 1;
            qs_f32x2 rp[3], rv[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const qs_f32x2 pj = {(float)s_pos[a * B + base + ja], (float)s_pos[a * B + base + jb]};
                const qs_f32x2 vj = {(float)s_vel[a * B + base + ja], (float)s_vel[a * B + base + jb]};
                rp[a] = pj - (float)mypos[a]; rv[a] = vj - (float)myvel[a];
            }
            const qs_f32x2 m = nbr_metric_x2(rp, rv);
            m4[2 * h] = m.x; m4[2 * h + 1] = m.y;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) L.insert(m4[u], j0 + u, (j0 + u < N) & (j0 + u != i), K);
    }
    return L.finish(K, bi);
}

template <typename real>
__device__ __forceinline__ void nbr_select(const Consts<real> &c, int N, int i, int base, int B, int tid, const real *s_pos,
    const real *s_vel,
                                           real *s_metric, const real mypos[3], const real myvel[3], NbrSel<real> &S) {
    const int K = c.num_neighbors;
    S.taken = 1ull << i;
    if (K <= 0 || K == N - 1) return;
#ifndef QS_EXACT_NBR_SELECT   // (-DQS_EXACT_NBR_SELECT: every drone on the exact path below; tests/test_object_identity_gpu.py)
    if constexpr (sizeof(real) == 4) {
        // (N <= 8: rank-by-counting below stays - measured at 8 x 131072, profiles/r06s2_ab_keys_packed_scan.txt: 97.8 us against 99.2 with keys)
        if (K <= 8 && N > 8 && nbr_select_keys<real>(c, N, i, base, B, s_pos, s_vel, mypos, myvel, S.bi)) return;
    }
#endif
    if (N <= 8) {   // all candidates at once, rank-by-counting (independent compares), then the inverse permutation: only the 8 indices
        real mj[8];  // stay live (the emit re-reads the chosen drones from LDS: registers decide the occupancy of this kernel)
        int rank[8];
        {
            real rp[8][3], rv[8][3];
#pragma unroll
            for (int u = 0; u < 8; ++u) {        // 48 LDS reads issued before the first use: one round trip
                const int j = (u < N) ? u : N - 1;
#pragma unroll
                for (int a = 0; a < 3; ++a) { rp[u][a] = s_pos[a * B + base + j] - mypos[a];
                    rv[u][a] = s_vel[a * B + base + j] - myvel[a]; }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                real rd = M<real>::fmax(norm3<real>(rp[u]), (real)0.01);
                real m = rd + (rp[u][0] * rv[u][0] + rp[u][1] * rv[u][1] + rp[u][2] * rv[u][2]) * M<real>::rcp(rd);
                mj[u] = (u < N && u != i) ? m : (real)3.4e38;
                rank[u] = 0;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int u = 0; u < 8; ++u) rank[u] += (int)((mj[k] < mj[u]) | ((mj[k] == mj[u]) & (k < u)));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int b = 0;
#pragma unroll
            for (int u = 1; u < 8; ++u) b = (rank[u] == k) ? u : b;   // the ranks are a permutation of 0..7
            S.bi[k] = b;
        }
        return;
    }
    if (K <= 8) {   // streaming sorted top-8 (metric, index) list; a candidate goes behind entries with an equal metric (lower index first)
        real bm[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { bm[k] = (real)3.4e38; S.bi[k] = 0; }
        for (int j0 = 0; j0 < N; j0 += 4) {
            real rp[4][3], rv[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = (j0 + u < N) ? j0 + u : N - 1;
#pragma unroll
                for (int a = 0; a < 3; ++a) { rp[u][a] = s_pos[a * B + base + j] - mypos[a];
                    rv[u][a] = s_vel[a * B + base + j] - myvel[a]; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                real rd = M<real>::fmax(norm3<real>(rp[u]), (real)0.01);
                real m = rd + (rp[u][0] * rv[u][0] + rp[u][1] * rv[u][1] + rp[u][2] * rv[u][2]) * M<real>::rcp(rd);
                m = (j < N && j != i) ? m : (real)3.4e38;
                int mi = j;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const bool lt = m < bm[k];
                    const real tm = lt ? bm[k] : m;
                    const int ti = lt ? S.bi[k] : mi;
                    bm[k] = lt ? m : bm[k];
                    S.bi[k] = lt ? mi : S.bi[k];
                    m = tm; mi = ti;
                }
            }
        }
        return;
    }
    for (int j = 0; j < N; ++j) {   // 8 < K < N-1: metrics into this lane's LDS column
        real rp[3] = {s_pos[0 * B + base + j] - mypos[0], s_pos[1 * B + base + j] - mypos[1], s_pos[2 * B + base + j] - mypos[2]};
        real rv[3] = {s_vel[0 * B + base + j] - myvel[0], s_vel[1 * B + base + j] - myvel[1], s_vel[2 * B + base + j] - myvel[2]};
        real rd = M<real>::fmax(norm3<real>(rp), (real)0.01);
        real mm = rd + (rp[0] * rv[0] + rp[1] * rv[1] + rp[2] * rv[2]) * M<real>::rcp(rd);
        s_metric[j * B + tid] = (j == i) ? (real)3.4e38 : mm;
    }
}
// neighbours of ranks [k0, k1) -> o[(rank - k0) * 6 ..]   (o = this lane's dense stage row of (k1 - k0) * 6 columns)
template <typename real>
__device__ __forceinline__ void nbr_emit(const Consts<real> &c, int N, int i, int base, int B, int tid, const real *s_pos,
    const real *s_vel,
                                         const real *s_metric, const real mypos[3], const real myvel[3], NbrSel<real> &S, int k0, int k1,
                                             real *o) {
    const int K = c.num_neighbors;
    for (int k = k0; k < k1; ++k) {
        int j;
        if (K == N - 1) j = (k < i) ? k : k + 1;   // all other drones in index order (:253-254)
        else if (K <= 8) {
            j = S.bi[0];
#pragma unroll
            for (int q = 1; q < 8; ++q) j = (q == k) ? S.bi[q] : j;   // register array: select, no dynamic indexing
        } else {   // arg-min round over the LDS metric column (lowest index wins ties)
            int best = -1;
            real bmin = (real)3.4e38;
            for (int jj = 0; jj < N; ++jj) {
                real mm = s_metric[jj * B + tid];
                bool better = !(S.taken >> jj & 1) && (best < 0 || mm < bmin);
                best = better ? jj : best;
                bmin = better ? mm : bmin;
            }
            S.taken |= 1ull << best;
            j = best;
        }
        real vals[6];
#pragma unroll
        for (int a = 0; a < 3; ++a) { vals[a] = s_pos[a * B + base + j] - mypos[a]; vals[3 + a] = s_vel[a * B + base + j] - myvel[a]; }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o[(k - k0) * 6 + a] = clipr<real>(vals[a], -c.nbr_clip_pos[a], c.nbr_clip_pos[a]);
            o[(k - k0) * 6 + 3 + a] = clipr<real>(vals[3 + a], -c.nbr_clip_vel[a], c.nbr_clip_vel[a]);
        }
    }
}

// Team kernels, more than 8 drones, K <= 8 (qs_step_team.inc, pair-once): wave wv >= 1 ranks ITS candidates j = (wv-1), (wv-1) + (W-1), ...
// of drone i's row of the metric matrix by counting inside the stripe (all keys in registers; every compare feeds two ranks), and
// publishes the 8 nearest of them compacted by local rank: s_topk slot (wv-1)*8 + rank.  recompute: the metrics are evaluated from the
// current positions / velocities instead of read from the matrix (environments whose velocities changed after the pair scan).
// (the candidate count is a literal in a config-specialised object: register arrays sized for 64 drones there keep the compiler from
// promoting the kernel's constant block out of scratch memory)
#ifdef QS_SPEC_N
#define QS_TEAM_NMAX QS_SPEC_N
#else
#define QS_TEAM_NMAX QS_MAX_AGENTS
#endif
template <typename real, int W>
__device__ __forceinline__ void team_rank_local(int N, int i, int base, int B, int tid, int wv, const real *s_pos, const real *s_vel,
                                                const real *s_metric, unsigned char *s_topk, bool recompute) {
    constexpr int RW = W - 1, CMAX = (QS_TEAM_NMAX + RW - 1) / RW, SL = RW * 8;
    const int C = (N + RW - 1) / RW;
    NbrKey<real> key[CMAX];
    int lr[CMAX];
    real mp[3] = {0, 0, 0}, mv[3] = {0, 0, 0};
    if (recompute) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { mp[q] = s_pos[q * B + tid]; mv[q] = s_vel[q * B + tid]; }
    }
#pragma unroll
    for (int u = 0; u < CMAX; ++u) {
        lr[u] = 0;
        if (u < C) {
            const int j = (wv - 1) + RW * u, jc = j < N ? j : N - 1;
            const bool valid = (j < N) & (j != i);
            real m;
            if (recompute) {
                const real rp[3] = {s_pos[0 * B + base + jc] - mp[0], s_pos[1 * B + base + jc] - mp[1], s_pos[2 * B + base + jc] - mp[2]};
                const real rv[3] = {s_vel[0 * B + base + jc] - mv[0], s_vel[1 * B + base + jc] - mv[1], s_vel[2 * B + base + jc] - mv[2]};
                m = nbr_metric<real>(rp, rv);
            } else {
                m = s_metric[jc * B + tid];
            }
            key[u] = NbrKey<real>::make(valid ? m : (real)3.4e38, valid ? j : 0x7fffff00 + u);
        }
    }
#pragma unroll
    for (int u = 0; u < CMAX; ++u) {
#pragma unroll
        for (int k = u + 1; k < CMAX; ++k) {
            if (k < C) {   // keys are distinct (the index breaks ties): exactly one of the two is the smaller
                const int lt = (int)key[u].less(key[k]);
                lr[k] += lt; lr[u] += 1 - lt;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < CMAX; ++u) {
        if (u < C && lr[u] < 8) NbrKey<real>::st(s_topk, SL, (wv - 1) * 8 + lr[u], B, tid, key[u]);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        // fewer candidates than slots
        if (q >= C) NbrKey<real>::st(s_topk, SL, (wv - 1) * 8 + q, B, tid, NbrKey<real>::make((real)3.4e38, 0x7fffff00 + q));
    }
}

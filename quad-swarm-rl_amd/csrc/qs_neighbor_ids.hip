// qs_neighbor_ids.hip - the neighbour identities behind include/quadswarm_neighbors.h: which drone stands behind each of the K neighbour
// slots of an observation row, found by redoing the slot's one subtraction from the stored state and comparing exactly; and the scatter
// of per-slot values into drone-by-drone matrices.  Launches of their own beside the step kernel: no step, reset or encoder kernel knows
// of them.
//
// Mapping of qs_neighbor_ids_kernel: one wave per state block, lane = the drone's lane of the step kernels (local env * N + drone), as in
// qs_pilot.hip.  The wave first puts the positions and velocities of its block into LDS (component-major, 6 x 64 elements per wave); then
// each lane takes the slots of its row 8 at a time (4 in double) and passes once over the at most 64 drones of its environment per chunk -
// the lanes of one environment read the same LDS word (a broadcast), the environments of a block words N apart - noting the matches of
// every slot as a bit per drone; the drones already given to a slot are a 64-bit mask in registers.  Lanes behind the block's last drone (N does not divide 64; N > 32, where a block is one environment), environments behind
// the last one (a partial last block) and the waves a rounded-up grid adds wait at the barrier and leave: they read no state and write
// nothing.  Per drone 24 bytes of state and 24 K bytes of the row in, 4 K bytes out (float32) - less than a step moves.
//
// The arithmetic is the emitting side's (qs_nbr_obs.h): clip(x_j - x_i, -c, +c), a subtraction and a clamp - nothing a contraction or a
// fast-math flag could change.  The clamp is written as two compares; the step kernels' float32 form (v_med3_f32) gives the same value
// for every finite x.
#include "qs_neighbors.h"   // with qs_state_blk.h: StateBlk, QS_BLK_AT, QS_WAVE - the block layout the state is read from

#include <string>

template <typename real> struct NbrClip { real p[3], v[3]; };   // +-nbr_clip_pos / +-nbr_clip_vel in the handle's precision, by value

template <typename real> __device__ __forceinline__ real nbr_ids_clip(real x, real c) { return x < -c ? -c : (x > c ? c : x); }

// LM: the element order of the handle's blocks as a literal (StateBlk::lane_major), so that the accessor's order test folds away
template <typename real, int LM>
__device__ __forceinline__ void nbr_ids_stage(StateBlk B, int N, int e, int i, int lane, real *sp, real *sv) {
    B.lane_major = LM;
#pragma unroll
    for (int q = 0; q < 3; ++q) { sp[q * QS_WAVE + lane] = QS_BLK_AT(real, B, pos, q, e, i, N); sv[q * QS_WAVE + lane] = QS_BLK_AT(real, B, vel, q, e, i, N); }
}

template <typename real>
__global__ void __launch_bounds__(256) qs_neighbor_ids_kernel(const StateBlk B, const NbrClip<real> c, int E, int N, int K, int nblk,
    const real *obs, int obs_dim, int self_dim, int32_t *ids) {
    __shared__ real s_state[4][6][QS_WAVE];   // per wave: pos x y z, vel x y z of the block's 64 lanes
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int blk = blockIdx.x * (blockDim.x >> 6) + wv;
    const int el = lane / N, i = lane - el * N, e = blk * (int)B.epb + el;
    const bool live = blk < nblk && el < (int)B.epb && e < E;
    real *sp = &s_state[wv][0][0], *sv = &s_state[wv][3][0];
    if (live) {   // (a live lane reads only the words of its own environment's lanes, which are live too)
        if (B.lane_major) nbr_ids_stage<real, 1>(B, N, e, i, lane, sp, sv);
        else nbr_ids_stage<real, 0>(B, N, e, i, lane, sp, sv);
    }
    __syncthreads();
    if (!live) return;                               // idle lanes of a block, a partial last block, the waves a rounded-up grid adds
    const size_t g = (size_t)e * N + i;
    const real *row = obs + g * (size_t)obs_dim + self_dim;
    int32_t *out = ids + g * (size_t)K;
    const int base = el * N;
    real mp[3], mv[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { mp[q] = sp[q * QS_WAVE + lane]; mv[q] = sv[q * QS_WAVE + lane]; }
    unsigned long long taken = 1ull << i;            // the drone itself is nobody's neighbour
    // SC slots at a time: their 6 SC columns are loaded at once (one memory round trip per chunk instead of one per slot), then ONE pass over
    // the environment's drones forms each difference once and notes per slot, as a bit per drone, whose position matches (pm) and whose
    // velocity matches as well (vm); the slots then choose in order.  No branch inside the pass.
    constexpr int SC = sizeof(real) == 4 ? 8 : 4;
    for (int s0 = 0; s0 < K; s0 += SC) {
        real want[SC][6];
#pragma unroll
        for (int u = 0; u < SC; ++u) {
            const int s = s0 + u < K ? s0 + u : K - 1;   // (behind the last slot: that slot again, inside the row)
#pragma unroll
            for (int q = 0; q < 6; ++q) want[u][q] = row[6 * s + q];
        }
        unsigned long long pm[SC], vm[SC];
#pragma unroll
        for (int u = 0; u < SC; ++u) { pm[u] = 0ull; vm[u] = 0ull; }
        for (int j = 0; j < N; ++j) {
            real d[6];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                d[q] = nbr_ids_clip<real>(sp[q * QS_WAVE + base + j] - mp[q], c.p[q]);
                d[3 + q] = nbr_ids_clip<real>(sv[q * QS_WAVE + base + j] - mv[q], c.v[q]);
            }
            const unsigned long long bit = 1ull << j;
#pragma unroll
            for (int u = 0; u < SC; ++u) {
                const bool p = (d[0] == want[u][0]) & (d[1] == want[u][1]) & (d[2] == want[u][2]);
                const bool v = p & (d[3] == want[u][3]) & (d[4] == want[u][4]) & (d[5] == want[u][5]);
                pm[u] |= p ? bit : 0ull;
                vm[u] |= v ? bit : 0ull;
            }
        }
#pragma unroll
        for (int u = 0; u < SC; ++u) {
            if (s0 + u < K) {
                const unsigned long long cand = pm[u] & ~taken, pref = vm[u] & cand;   // the lowest free index: of the velocity matches first
                const int id = pref ? __builtin_ctzll(pref) : (cand ? __builtin_ctzll(cand) : -1);
                if (id >= 0) taken |= 1ull << id;
                out[s0 + u] = id;
            }
        }
    }
}

// one thread per output row (e, i): zero the N entries, then one entry per slot whose id names another drone of the environment
__global__ void __launch_bounds__(256) qs_neighbor_scatter_kernel(const int32_t *ids, const float *w, long long rows, int N, int K, float *out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= rows) return;
    const int i = (int)(g % N);
    float *o = out + (size_t)g * N;
    for (int j = 0; j < N; ++j) o[j] = 0.0f;
    for (int s = 0; s < K; ++s) {
        const int j = ids[(size_t)g * K + s];
        if (j >= 0 && j < N && j != i) o[j] = w[(size_t)g * K + s];
    }
}

template <typename real> static void nbr_ids_launch(const QsNeighborsView &v, const void *obs, int32_t *ids, hipStream_t s) {
    NbrClip<real> c;
    for (int q = 0; q < 3; ++q) { c.p[q] = (real)v.cfg->nbr_clip_pos[q]; c.v[q] = (real)v.cfg->nbr_clip_vel[q]; }
    const int E = v.cfg->num_envs, N = v.cfg->num_agents, nblk = (E + (int)v.blk.epb - 1) / (int)v.blk.epb;
    const int waves = nblk <= 8 * v.cus ? 1 : 4;     // waves per workgroup: spread a small batch over the CUs (as qs_pilot.hip)
    hipLaunchKernelGGL(qs_neighbor_ids_kernel<real>, dim3((nblk + waves - 1) / waves), dim3(QS_WAVE * waves), 0, s, v.blk, c, E, N,
        (int)v.cfg->num_neighbors, nblk, (const real *)obs, v.obs_dim, v.self_dim, ids);
}

extern "C" {

int qs_neighbor_ids(qs_handle *h, const void *obs_dev, int32_t *ids_out_dev, void *stream) {
    QsNeighborsView v;
    if (int rc = qs_neighbors_view(h, &v)) return rc;
    const int N = v.cfg->num_agents, K = v.cfg->num_neighbors;
    if (K < 1) return qs_neighbors_fail(QS_ERR_INVALID, "qs_neighbor_ids: the handle's rows have no neighbour slots (num_neighbors is 0)");
    if (!ids_out_dev) return qs_neighbors_fail(QS_ERR_INVALID, "qs_neighbor_ids: ids_out_dev is NULL");
    if (N < 2 || N > QS_MAX_AGENTS || K > N - 1 || (int)v.blk.epb < 1 || (int)v.blk.epb * N > QS_WAVE || v.self_dim < 0 ||
        v.self_dim + 6 * K > v.obs_dim)
        return qs_neighbors_fail(QS_ERR_INVALID, "qs_neighbor_ids: bad handle shape");
    if (v.gate_resident) return qs_neighbors_fail(QS_ERR_UNSUPPORTED,
        "qs_neighbor_ids: a gated launch of this handle is resident and holds the state (qs_sync first)");
    const void *obs = obs_dev ? obs_dev : v.obs;
    hipError_t e = hipSetDevice(v.device);
    if (e == hipSuccess) {
        if (v.real_size == 8) nbr_ids_launch<double>(v, obs, ids_out_dev, (hipStream_t)stream);
        else nbr_ids_launch<float>(v, obs, ids_out_dev, (hipStream_t)stream);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return qs_neighbors_fail(QS_ERR_HIP, (std::string("qs_neighbor_ids: ") + hipGetErrorString(e)).c_str());
    return QS_OK;
}

int qs_neighbor_scatter(const int32_t *ids_dev, const float *w_dev, int32_t E, int32_t N, int32_t K, float *out_dev, void *stream) {
    if (!ids_dev || !w_dev || !out_dev) return qs_neighbors_fail(QS_ERR_INVALID, "qs_neighbor_scatter: null pointer");
    if (N < 2 || N > QS_MAX_AGENTS || K < 1 || K > N - 1 || E < 1)
        return qs_neighbors_fail(QS_ERR_INVALID, "qs_neighbor_scatter: 2 <= N <= QS_MAX_AGENTS, 1 <= K <= N - 1 and E >= 1 wanted");
    const long long rows = (long long)E * N;
    hipLaunchKernelGGL(qs_neighbor_scatter_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ids_dev, w_dev, rows,
        (int)N, (int)K, out_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qs_neighbors_fail(QS_ERR_HIP, (std::string("qs_neighbor_scatter: ") + hipGetErrorString(e)).c_str());
    return QS_OK;
}

}   // extern "C"

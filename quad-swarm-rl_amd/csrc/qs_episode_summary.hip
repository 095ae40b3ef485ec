// qs_episode_summary.hip - the episode summary behind include/quadswarm_summary.h: per-scenario sums and counts of what the finished
// episodes of a handle left in ep_sums / ep_stats / ep_counters, added up on the device in two launches.
//
// Launch 1 (qs_summary_partial_kernel): 128-thread workgroups; a workgroup takes a contiguous range of TILES, a tile being the
// max(1, 128 / N) consecutive environments whose agents fit one workgroup.  Per tile:
//   0  thread = environment: the done rows of the call -> ended / overrun flags, the two scenario ids, the replay flag, the 11 episode
//      counters (adjacent threads read adjacent environments).  A tile without an end stops here.
//   1  thread = agent (lane = agent: a row of ep_sums / ep_stats is read as consecutive elements): the 8 action-moment rows and the three
//      flag rows of ep_stats go to LDS
//   2  thread = environment: its N agents' moments and flags, in agent order -> the episode's rates and its action mean / std
//   3  thread = agent: the 17 reward rows, true_reward and the three distances go to LDS
//   4  thread = table column: walks the tile's agents (or environments) in index order and adds each into the workgroup's LDS table at the
//      row of the environment's scenario - one owner per element, no atomics, and an order that depends on (E, N) alone
// and at the end the workgroup's table goes to its slot of the partials.  Launch 2 (qs_summary_fold_kernel): one thread per table element
// adds the partials in workgroup order to the table.  All sums are doubles or 64-bit integers; the unit is compiled without FMA contraction
// (native.UNIT_FLAGS), so true_reward and the variance round as the host's numpy expressions do.
//
// Bounds: scenario ids are masked to [0, 16) before they index a row; every global read is at e < E, agent < E*N, done row < steps.
#include "qs_summary.h"

#include <hip/hip_runtime.h>

#include <string>

#define SUMM_THREADS 128
#define SUMM_MAX_WGS 512
#define SUMM_NV (QS_RI_COUNT + 4)   // per-agent values staged in LDS: the reward rows, true_reward, three distances
#define SUMM_V_TRUE QS_RI_COUNT
#define SUMM_V_DIST (QS_RI_COUNT + 1)
#define SUMM_NE 13                  // per-environment values: 5 rates, 4 action means, 4 action standard deviations
#define SUMM_D (QS_SUMM_SCENARIOS * QS_SUMM_D_COUNT)
#define SUMM_I (QS_SUMM_SCENARIOS * QS_SUMM_I_COUNT)

enum { SUMM_ENDED = 1, SUMM_REPLAY = 2, SUMM_OVERRUN = 4 };

struct SummK {
    int E, N, tile_envs, steps, ep_len, has_sums;
    const uint8_t *done;
    const void *ep_sums, *ep_stats;
    const int32_t *ep_counters, *ep_scenario, *scenario_id;
    const uint8_t *was_replay;
    const int32_t *ep_steps;
    double *part_d;
    long long *part_i;
};

static int summ_tile_envs(int N) { return N >= SUMM_THREADS ? 1 : SUMM_THREADS / N; }
static int summ_wgs(int E, int N) {
    const int te = summ_tile_envs(N), tiles = (E + te - 1) / te;
    return tiles < SUMM_MAX_WGS ? tiles : SUMM_MAX_WGS;
}

template <typename real>
__global__ void __launch_bounds__(SUMM_THREADS) qs_summary_partial_kernel(const SummK k) {
    __shared__ double V[SUMM_NV][SUMM_THREADS];
    __shared__ double EV[SUMM_NE][SUMM_THREADS];
    __shared__ int32_t IC[QS_CNT_COUNT][SUMM_THREADS];
    __shared__ int32_t sc_end[SUMM_THREADS], sc_cur[SUMM_THREADS], fl[SUMM_THREADS], pf[SUMM_THREADS];
    __shared__ double acc_d[SUMM_D];
    __shared__ long long acc_i[SUMM_I];

    const int t = threadIdx.x, N = k.N, E = k.E, TE = k.tile_envs;
    const size_t T = (size_t)E * N;
    const real *sums = (const real *)k.ep_sums, *eps = (const real *)k.ep_stats;
    for (int i = t; i < SUMM_D; i += SUMM_THREADS) acc_d[i] = 0.0;
    for (int i = t; i < SUMM_I; i += SUMM_THREADS) acc_i[i] = 0;

    const int tiles = (E + TE - 1) / TE, per = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int tile0 = (int)blockIdx.x * per, tile1 = tile0 + per < tiles ? tile0 + per : tiles;
    for (int tile = tile0; tile < tile1; ++tile) {
        const int e0 = tile * TE, ne = E - e0 < TE ? E - e0 : TE, na = ne * N;
        // ---- 0: the tile's environments
        int f = 0;
        if (t < ne) {
            const int e = e0 + t;
            int ends = 0;
            for (int s = 0; s < k.steps; ++s) ends += k.done[(size_t)s * T + (size_t)e * N] ? 1 : 0;
            if (ends) {
                f = SUMM_ENDED | (ends > 1 ? SUMM_OVERRUN : 0) | ((k.was_replay && k.was_replay[e]) ? SUMM_REPLAY : 0);
                sc_end[t] = k.ep_scenario[e] & (QS_SUMM_SCENARIOS - 1);
                sc_cur[t] = k.scenario_id[e] & (QS_SUMM_SCENARIOS - 1);
#pragma unroll
                for (int c = 0; c < QS_CNT_COUNT; ++c) IC[c][t] = k.ep_counters[(size_t)c * E + e];
            }
            fl[t] = f;
        }
        if (!__syncthreads_or(f)) continue;   // no end in this tile (the same answer in every thread)
        const int el = t < na ? t / N : 0;
        const bool mine = t < na && (fl[el] & SUMM_ENDED);
        const size_t a = (size_t)e0 * N + t;
        // ---- 1: per agent, the action moments and the three flags
        if (mine) {
#pragma unroll
            for (int q = 0; q < 8; ++q) V[q][t] = k.has_sums ? (double)sums[(size_t)(QS_SUM_ACT + q) * T + a] : 0.0;
            const real reached = eps[(size_t)QS_EPS_REACHED_GOAL * T + a];
            const bool aok = eps[(size_t)QS_EPS_COL_AGENT_OK * T + a] != (real)0, ook = eps[(size_t)QS_EPS_COL_OBST_OK * T + a] != (real)0;
            const bool ok = aok && ook;
            pf[t] = ((ok && reached != (real)0) ? 1 : 0) | ((ok && ((real)1 - reached) != (real)0) ? 2 : 0) | (ok ? 4 : 0) | (aok ? 8 : 0) | (ook ? 16 : 0);
        }
        __syncthreads();
        // ---- 2: per environment, the rates and the action mean / std of the episode
        if (t < ne && (f & SUMM_ENDED)) {
            int cs = 0, cd = 0, cok = 0, ca = 0, co = 0;
            double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = 0; i < N; ++i) {
                const int idx = t * N + i, p = pf[idx];
                cs += p & 1; cd += (p >> 1) & 1; cok += (p >> 2) & 1; ca += (p >> 3) & 1; co += (p >> 4) & 1;
#pragma unroll
                for (int q = 0; q < 4; ++q) { s1[q] += V[q][idx]; s2[q] += V[4 + q][idx]; }
            }
            const double dn = (double)N;
            EV[0][t] = (double)cs / dn; EV[1][t] = (double)cd / dn;
            EV[2][t] = 1.0 - (double)cok / dn; EV[3][t] = 1.0 - (double)ca / dn; EV[4][t] = 1.0 - (double)co / dn;
            const double count = (double)(k.ep_steps ? k.ep_steps[e0 + t] : k.ep_len + 1) * dn;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double a1 = s1[q] / count, a2 = s2[q] / count, var = a2 - a1 * a1;
                EV[5 + q][t] = k.has_sums ? a1 : 0.0;
                EV[9 + q][t] = k.has_sums ? sqrt(var > 0.0 ? var : 0.0) : 0.0;
            }
        }
        __syncthreads();
        // ---- 3: per agent, the reward rows, true_reward, the distances
        if (mine) {
            double main_ = 0.0, quadcol = 0.0;
#pragma unroll
            for (int r = 0; r < QS_RI_COUNT; ++r) {
                const double v = k.has_sums ? (double)sums[(size_t)r * T + a] : 0.0;
                V[r][t] = v;
                if (r == QS_RI_RAW_MAIN) main_ = v;
                if (r == QS_RI_RAW_QUADCOL) quadcol = v;
            }
            V[SUMM_V_TRUE][t] = main_ + 1000.0 * quadcol;
#pragma unroll
            for (int d = 0; d < 3; ++d) V[SUMM_V_DIST + d][t] = (double)eps[(size_t)(QS_EPS_DIST_1S + d) * T + a];
        }
        __syncthreads();
        // ---- 4: per table column, the tile's terms in index order
        if (t < QS_SUMM_D_COUNT) {
            const int c = t;
            const double *src;
            bool per_agent = true, fresh_only = false, by_start = false;
            if (c < QS_SUMM_D_SUCCESS) { src = V[SUMM_V_DIST + c]; fresh_only = true; }
            else if (c < QS_SUMM_D_REW) { src = EV[c - QS_SUMM_D_SUCCESS]; per_agent = false; fresh_only = true; }
            else if (c <= QS_SUMM_D_TRUE_REWARD) src = V[c - QS_SUMM_D_REW];
            else if (c < QS_SUMM_D_START_REW_POS) { src = EV[5 + c - QS_SUMM_D_ACT_MEAN]; per_agent = false; }
            else { src = V[c == QS_SUMM_D_START_REW_POS ? QS_RI_REW_POS : QS_RI_REW_CRASH]; by_start = true; }
            for (int x = 0; x < ne; ++x) {
                const int fx = fl[x];
                if (!(fx & SUMM_ENDED) || (fresh_only && (fx & SUMM_REPLAY))) continue;
                const int slot = (by_start ? sc_cur[x] : sc_end[x]) * QS_SUMM_D_COUNT + c;
                double s = acc_d[slot];
                if (per_agent) { for (int i = 0; i < N; ++i) s += src[x * N + i]; }
                else s += src[x];
                acc_d[slot] = s;
            }
        } else if (t < QS_SUMM_D_COUNT + QS_SUMM_I_COUNT) {
            const int c = t - QS_SUMM_D_COUNT;
            int need = SUMM_ENDED, forbid = 0, cnt_row = -1;
            bool by_start = false;
            if (c == QS_SUMM_I_REPLAYED) need |= SUMM_REPLAY;
            else if (c >= QS_SUMM_I_CNT && c < QS_SUMM_I_COL_REPLAY) { forbid = SUMM_REPLAY; cnt_row = c - QS_SUMM_I_CNT; }
            else if (c == QS_SUMM_I_COL_REPLAY) { need |= SUMM_REPLAY; cnt_row = QS_CNT_COLLISIONS; }
            else if (c == QS_SUMM_I_OBST_REPLAY) { need |= SUMM_REPLAY; cnt_row = QS_CNT_OBST; }
            else if (c == QS_SUMM_I_OVERRUN) need |= SUMM_OVERRUN;
            else if (c == QS_SUMM_I_START_EPISODES) by_start = true;
            for (int x = 0; x < ne; ++x) {
                const int fx = fl[x];
                if ((fx & need) != need || (fx & forbid)) continue;
                acc_i[(by_start ? sc_cur[x] : sc_end[x]) * QS_SUMM_I_COUNT + c] += cnt_row >= 0 ? (long long)IC[cnt_row][x] : 1;
            }
        }
        __syncthreads();   // the next tile overwrites what phase 4 read
    }
    __syncthreads();
    for (int i = t; i < SUMM_D; i += SUMM_THREADS) k.part_d[(size_t)blockIdx.x * SUMM_D + i] = acc_d[i];
    for (int i = t; i < SUMM_I; i += SUMM_THREADS) k.part_i[(size_t)blockIdx.x * SUMM_I + i] = acc_i[i];
}

__global__ void __launch_bounds__(256) qs_summary_fold_kernel(double *tab_d, long long *tab_i, const double *part_d, const long long *part_i,
    int wgs) {
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx < SUMM_D) {
        double s = tab_d[idx];
        for (int w = 0; w < wgs; ++w) s += part_d[(size_t)w * SUMM_D + idx];
        tab_d[idx] = s;
    } else if (idx < SUMM_D + SUMM_I) {
        const int j = idx - SUMM_D;
        long long s = tab_i[j];
        for (int w = 0; w < wgs; ++w) s += part_i[(size_t)w * SUMM_I + j];
        tab_i[j] = s;
    }
}

// the handle's one allocation: [tab_d | tab_i | part_d (wgs tables) | part_i (wgs tables)]
static double *summ_tab_d(void *base) { return (double *)base; }
static long long *summ_tab_i(void *base) { return (long long *)((double *)base + SUMM_D); }
static double *summ_part_d(void *base) { return (double *)base + SUMM_D + SUMM_I; }
static long long *summ_part_i(void *base, int wgs) { return (long long *)(summ_part_d(base) + (size_t)wgs * SUMM_D); }

static int summ_hip_fail(const char *where, hipError_t e) {
    return qs_summary_fail(QS_ERR_HIP, (std::string(where) + ": " + hipGetErrorString(e)).c_str());
}

extern "C" {

int qs_episode_summary_enable(qs_handle *h) {
    QsSummaryView v;
    if (int rc = qs_summary_view(h, &v)) return rc;
    if (*v.store) return QS_OK;
    if (v.N < 1 || v.N > QS_MAX_AGENTS || v.E < 1) return qs_summary_fail(QS_ERR_INVALID, "qs_episode_summary_enable: bad handle shape");
    const int wgs = summ_wgs(v.E, v.N);
    const size_t bytes = (size_t)(SUMM_D + SUMM_I) * 8 * (size_t)(1 + wgs);
    hipError_t e = hipSetDevice(v.device);
    void *p = nullptr;
    if (e == hipSuccess) e = hipMalloc(&p, bytes);
    if (e == hipSuccess) e = hipMemset(p, 0, bytes);
    if (e != hipSuccess) { if (p) (void)hipFree(p); return summ_hip_fail("qs_episode_summary_enable", e); }
    *v.store = p;
    return QS_OK;
}

int qs_episode_summary_accumulate(qs_handle *h, const uint8_t *done_dev, int32_t steps, void *stream) {
    QsSummaryView v;
    if (int rc = qs_summary_view(h, &v)) return rc;
    if (!*v.store) return qs_summary_fail(QS_ERR_INVALID, "qs_episode_summary_accumulate: call qs_episode_summary_enable first");
    if (v.gate_resident) return qs_summary_fail(QS_ERR_UNSUPPORTED,
        "qs_episode_summary_accumulate: a gated launch of this handle is resident (qs_sync first)");
    if (!done_dev) { done_dev = v.done; steps = 1; }
    if (steps < 1) return qs_summary_fail(QS_ERR_INVALID, "qs_episode_summary_accumulate: steps must be >= 1");
    const int wgs = summ_wgs(v.E, v.N);
    SummK k = {v.E, v.N, summ_tile_envs(v.N), steps, v.ep_len, v.episode_sums ? 1 : 0, done_dev, v.ep_sums, v.ep_stats, v.ep_counters,
               v.ep_scenario, v.scenario_id, v.ep_was_replay, v.ep_steps, summ_part_d(*v.store), summ_part_i(*v.store, wgs)};
    hipError_t e = hipSetDevice(v.device);
    if (e == hipSuccess) {
        hipStream_t s = (hipStream_t)stream;
        if (v.real_size == 8) hipLaunchKernelGGL(qs_summary_partial_kernel<double>, dim3(wgs), dim3(SUMM_THREADS), 0, s, k);
        else hipLaunchKernelGGL(qs_summary_partial_kernel<float>, dim3(wgs), dim3(SUMM_THREADS), 0, s, k);
        hipLaunchKernelGGL(qs_summary_fold_kernel, dim3((SUMM_D + SUMM_I + 255) / 256), dim3(256), 0, s, summ_tab_d(*v.store),
                           summ_tab_i(*v.store), (const double *)k.part_d, (const long long *)k.part_i, wgs);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return summ_hip_fail("qs_episode_summary_accumulate", e);
    return QS_OK;
}

int qs_episode_summary_read(qs_handle *h, double *sums_host, int64_t *counts_host, int32_t clear, void *stream) {
    QsSummaryView v;
    if (int rc = qs_summary_view(h, &v)) return rc;
    if (!*v.store) return qs_summary_fail(QS_ERR_INVALID, "qs_episode_summary_read: call qs_episode_summary_enable first");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSetDevice(v.device);
    if (e == hipSuccess && sums_host) e = hipMemcpyAsync(sums_host, summ_tab_d(*v.store), (size_t)SUMM_D * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && counts_host) e = hipMemcpyAsync(counts_host, summ_tab_i(*v.store), (size_t)SUMM_I * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && clear) e = hipMemsetAsync(*v.store, 0, (size_t)(SUMM_D + SUMM_I) * 8, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return summ_hip_fail("qs_episode_summary_read", e);
    return QS_OK;
}

}   // extern "C"

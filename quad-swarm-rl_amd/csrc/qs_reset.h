// qs_reset.h - the episode reset: per-env scenario state between HBM, registers and LDS (scen_lds_*, ScenRegs), reset_body (shared by
// the reset kernels and the auto-reset at the tail of a step) and qs_reset_impl, the body of every reset kernel.  Included by
// qs_kernels.h, behind its team macros (QS_WAVE_SYNC).
#pragma once
#include "qs_obs_rows.h"
#include "qs_scenarios.h"
#include "qs_state_rows.h"

// full-scenario kernels: per-env scenario state HBM <-> LDS (each drone of the env moves a strided part)
template <typename real>
__device__ __forceinline__ void scen_lds_load(const Ptrs<real> &p, const LdsLayout &L, unsigned char *smem, int E, int e, int le, int i,
    int N) {
    real *sr = (real *)(smem + L.off_sr) + le * SR_COUNT;
    int *si = (int *)(smem + L.off_si) + le * SI_COUNT;
    uint64_t *om = (uint64_t *)(smem + L.off_omap) + le * 4;
    for (int k = i; k < SR_COUNT; k += N) sr[k] = p.scen_real[k * E + e];
    for (int k = i; k < SI_COUNT; k += N) si[k] = p.scen_int[k * E + e];
    for (int k = i; k < 4; k += N) om[k] = p.scen_omap[k * E + e];
}
#ifdef QS_SPEC_N
// The same load in two halves for the latency-bound team kernels: the global loads are issued with the state loads, the LDS writes wait
// until the sub-steps are done (a write right behind its load makes the wave wait for EVERY load in flight before it has drawn its noise).
template <typename real> struct ScenRegs {
    real r[(SR_COUNT + QS_SPEC_N - 1) / QS_SPEC_N];
    int n[(SI_COUNT + QS_SPEC_N - 1) / QS_SPEC_N];
    uint64_t o[(4 + QS_SPEC_N - 1) / QS_SPEC_N];
};
template <typename real>
__device__ __forceinline__ void scen_regs_load(const Ptrs<real> &p, int E, int e, int i, ScenRegs<real> &v) {
    constexpr int N = QS_SPEC_N;
#pragma unroll
    for (int j = 0; j < (SR_COUNT + N - 1) / N; ++j) { const int k = i + j * N; v.r[j] = (k < SR_COUNT)
        ? p.scen_real[k * E + e] : (real)0; }
#pragma unroll
    for (int j = 0; j < (SI_COUNT + N - 1) / N; ++j) { const int k = i + j * N; v.n[j] = (k < SI_COUNT) ? p.scen_int[k * E + e] : 0; }
#pragma unroll
    for (int j = 0; j < (4 + N - 1) / N; ++j) { const int k = i + j * N; v.o[j] = (k < 4) ? p.scen_omap[k * E + e] : 0ull; }
}
template <typename real>
__device__ __forceinline__ void scen_regs_to_lds(const LdsLayout &L, unsigned char *smem, int le, int i, const ScenRegs<real> &v) {
    constexpr int N = QS_SPEC_N;
    real *sr = (real *)(smem + L.off_sr) + le * SR_COUNT;
    int *si = (int *)(smem + L.off_si) + le * SI_COUNT;
    uint64_t *om = (uint64_t *)(smem + L.off_omap) + le * 4;
#pragma unroll
    for (int j = 0; j < (SR_COUNT + N - 1) / N; ++j) { const int k = i + j * N; if (k < SR_COUNT) sr[k] = v.r[j]; }
#pragma unroll
    for (int j = 0; j < (SI_COUNT + N - 1) / N; ++j) { const int k = i + j * N; if (k < SI_COUNT) si[k] = v.n[j]; }
#pragma unroll
    for (int j = 0; j < (4 + N - 1) / N; ++j) { const int k = i + j * N; if (k < 4) om[k] = v.o[j]; }
}
#endif
template <typename real>
__device__ __forceinline__ void scen_lds_store(const Ptrs<real> &p, const LdsLayout &L, unsigned char *smem, int E, int e, int le, int i,
    int N) {
    const real *sr = (const real *)(smem + L.off_sr) + le * SR_COUNT;
    const int *si = (const int *)(smem + L.off_si) + le * SI_COUNT;
    const uint64_t *om = (const uint64_t *)(smem + L.off_omap) + le * 4;
    for (int k = i; k < SR_COUNT; k += N) p.scen_real[k * E + e] = sr[k];
    for (int k = i; k < SI_COUNT; k += N) p.scen_int[k * E + e] = si[k];
    for (int k = i; k < 4; k += N) p.scen_omap[k * E + e] = om[k];
}

// ------------------------------------------------------------------------------------------------
// Episode reset of the envs whose lanes have `do_reset` set: QuadrotorEnvMulti.reset quadrotor_multi.py:339-411
// (+ QuadrotorSingle._reset quadrotor_single.py:387-447, obst_generation_given_density quadrotor_multi.py:304-325,
// scenario.reset()).  Shared by the reset kernel and the tail of the step kernel (auto-reset inside step, :720).
// Must be entered by the whole workgroup (contains barriers).  Outputs: d / goal (registers), the obs row in LDS,
// per-env global scratch (obstacle positions, scenario state).  `stale_vel` are the previous episode's final
// velocities: the first neighbour obs of an episode is computed from them (SURVEY App. A reset quirk).
// ------------------------------------------------------------------------------------------------
template <typename real, bool FULL, bool TEAM = false, bool STREAM = false>
__device__ __forceinline__ void reset_body(const Consts<real> *cp, const Ptrs<real> *pp, const LdsLayout *Lp, unsigned char *smem,
    int epb, const RngKey &key,
                                        bool do_reset, Drone<real> *dp, real goal[3], const real stale_vel[3], int blk = -1) {
    const int bidx = blk < 0 ? (int)blockIdx.x : blk;
    const Consts<real> &c = *cp;
    const Ptrs<real> &p = *pp;
    const LdsLayout &L = *Lp;
    Drone<real> &d = *dp;
    const int B = QS_WAVE, N = c.num_agents, E = c.num_envs;
    real *s_pos = (real *)(smem + L.off_pos), *s_vel = (real *)(smem + L.off_vel), *s_spawn = (real *)(smem + L.off_zax);
    real *s_goal = (real *)(smem + L.off_goal), *s_obs = (real *)(smem + L.off_obs), *s_obst = (real *)(smem + L.off_obst);
    real *s_metric = (real *)(smem + L.off_metric);
    uint32_t *s_envflag = (uint32_t *)(smem + L.off_envflag);
    const int tid = threadIdx.x, le = tid / N, i = tid - le * N, e = bidx * epb + le, base = le * N;
    const int M_ = c.num_obstacles;
    // STREAM: dense self block + rows stage
    real *myobs = STREAM ? (real *)(smem + L.off_self) + tid * c.self_dim : s_obs + tid * c.obs_dim;
    int *tidx = (int *)(smem + L.off_scratch) + le * (2 * L.scr_cap + 32), *tval = tidx + L.scr_cap, *prev_row = tidx + 2 * L.scr_cap,
        *cur_row = prev_row + 16;

#ifdef QS_TAPE
    int *s_cur = (int *)(smem + L.off_cur);
#endif
    // ---- per-env part (one lane): obstacle map + scenario.reset() ----
    if (do_reset && i == 0) {
#ifdef QS_TAPE
        if (QS_ON_TAPE(key)) *key.cur = s_cur[le];   // this lane consumes the env's tape sequentially
#endif
        real *goals = s_goal + le * L.goal_rows * 3;
        uint32_t have_spawn = 0;
        uint64_t omap[4] = {0, 0, 0, 0};   // obstacle map bitset, cell id = rid*W + cid
        const int Lr = c.obst_area[0], W = c.obst_area[1], cells = Lr * W;
        if (FULL) for (int q = 0; q < 4; ++q) ((uint64_t *)(smem + L.off_omap))[le * 4 + q] = 0;
        int Me = M_;   // obstacles of this episode
        if (c.use_obstacles) {
            // --quads_domain_random: this episode's density / size (quad_experience_replay.py:106-118,:191-206 -> reset(obst_density,
            // obst_size))
            if (c.dr_on) {
                if (c.dr_num_density > 0) {
                    const int k = rng_index<real>(key, QS_SITE_REPLAY, 2, c.dr_num_density);
                    Me = p.dr_count[k];
                    p.obst_density_env[e] = p.dr_density[k];
                }
                if (c.dr_num_size > 0) {
                    const int k = rng_index<real>(key, QS_SITE_REPLAY, 3, c.dr_num_size);
                    p.obst_size_env[e] = p.dr_size[k];
                    s_envflag[2 * epb + le] = (uint32_t)k;   // for the first observation of the episode, later in this launch
                }
                p.obst_count[e] = Me;
            }
            // np.random.choice(cells, M, replace=False): partial Fisher-Yates on a virtual pool
            int nt = 0;
            for (int k = 0; k < M_; ++k) {
                if (k >= Me) {   // unused slot: parked where no first-hit test and no SDF minimum can see it
                    p.obst_pos[(size_t)e * M_ + k] = (real)1e6; p.obst_pos[(size_t)E * M_ + (size_t)e * M_ + k] = (real)1e6;
                    s_obst[(le * 2 + 0) * M_ + k] = (real)1e6; s_obst[(le * 2 + 1) * M_ + k] = (real)1e6;
                    continue;
                }
                int vj;
                if (QS_ON_TAPE(key)) vj = (int)tape_pop(key);   // the tape holds the chosen cell ids (quadrotor_multi.py:313)
                else {
                    int j = k + rng_index<real>(key, QS_SITE_OBST_MAP, k, cells - k);
                    int vk = k, pj = -1;
                    vj = j;
                    for (int q = 0; q < nt; ++q) { if (tidx[q] == k) vk = tval[q]; if (tidx[q] == j) { vj = tval[q]; pj = q; } }
                    if (pj >= 0) tval[pj] = vk; else { tidx[nt] = j; tval[nt] = vk; ++nt; }   // pool[j] = pool[k]; the pick is old pool[j]
                }
                int id = vj, rid = id / W, cid = id - rid * W;
                omap[id >> 6] |= 1ull << (id & 63);
                if (FULL) ((uint64_t *)(smem + L.off_omap))[le * 4 + (id >> 6)] |= 1ull << (id & 63);
                // cell centre index rid + L*cid (quadrotor_multi.py:321); centres per obstacles/utils.py:47-58
                int ci = rid + Lr * cid, ii = ci / W, jj = (W - 1) - (ci - ii * W);
                real ox = (real)ii + (real)0.5 - (real)(Lr / 2), oy = (real)jj + (real)0.5 - (real)(W / 2);
                p.obst_pos[(size_t)e * M_ + k] = ox;
                p.obst_pos[(size_t)E * M_ + (size_t)e * M_ + k] = oy;
                s_obst[(le * 2 + 0) * M_ + k] = ox;
                s_obst[(le * 2 + 1) * M_ + k] = oy;
            }
        }
        Formation<real> F;
        if (FULL) {
            ScenCtx<real> x = {(real *)(smem + L.off_sr) + le * SR_COUNT, (int *)(smem + L.off_si) + le * SI_COUNT,
                               (uint64_t *)(smem + L.off_omap) + le * 4, goals, s_spawn, B, base, N};
            scenario_reset_full<real>(c, key, x, tidx);
            have_spawn = (uint32_t)x.si[SI_HAVE_SPAWN];
            s_envflag[epb + le] = (uint32_t)x.si[SI_PERIOD];
            p.scenario_id[e] = x.si[SI_SCEN];
        } else if (c.scenario == QS_SCENARIO_STATIC_SAME_GOAL) {
            update_formation<real>(c.scenario, key, 0, N, F);
            real center[3] = {0, 0, 2};
            const int rows = generate_goals<real>(F, N, 1, center, goals, 3);
            if (QS_ON_TAPE(key)) tape_skip(key, rows);   // np.random.shuffle(goals) of base.py:151: the rows are all the same point
            (void)rows;
        } else if (c.scenario == QS_SCENARIO_O_STATIC_SAME_GOAL) {
            // obstacles/o_static_same_goal.py:27-48 + o_base.py:69-81,:124-153
            int nfree = cells - Me;
            int nt = 0;
            const bool on_tape = QS_ON_TAPE(key);
            if (on_tape) tape_skip(key, 1);   // the duration draw of o_static_same_goal.py:29 (unused by a static goal)
            for (int k = 0; k < N; ++k) {
                int vj;
                if (on_tape) vj = (int)tape_pop(key);   // np.random.choice(free cells, N, replace=False): the ids themselves
                else {
                    int j = k + rng_index<real>(key, QS_SITE_SCEN, 16 + k, nfree - k);
                    int vk = k, pj = -1;
                    vj = j;
                    for (int q = 0; q < nt; ++q) { if (tidx[q] == k) vk = tval[q]; if (tidx[q] == j) { vj = tval[q]; pj = q; } }
                    if (pj >= 0) tval[pj] = vk; else { tidx[nt] = j; tval[nt] = vk; ++nt; }
                }
                int seen = 0, cell = 0;   // vj-th free cell in row-major order (np.where(obst_map == 0))
                for (int id = 0; id < cells; ++id) if (!(omap[id >> 6] >> (id & 63) & 1)) { if (seen == vj) { cell = id; break; } ++seen; }
                int x = cell / W, y = cell - x * W, index = x + Lr * y, ii = index / W, jj = (W - 1) - (index - ii * W);
                s_spawn[0 * B + base + k] = (real)ii + (real)0.5 - (real)(Lr / 2);
                s_spawn[1 * B + base + k] = (real)jj + (real)0.5 - (real)(W / 2);
                if (!on_tape) s_spawn[2 * B + base + k] = rng_uniform1<real>(key, QS_SITE_SCEN, 96 + k, 0, 0, (real)1, (real)3);
            }
            // the N heights follow the N ids (o_base.py:69-81)
            if (on_tape) for (int k = 0; k < N; ++k) s_spawn[2 * B + base + k] = (real)tape_pop(key);
            have_spawn = 1;
            // max_square_area_center o_base.py:124-153 (two-row dynamic programme)
            int max_size = 0, cx = 0, cy = 0;
            for (int q = 0; q < W; ++q) prev_row[q] = (int)(omap[q >> 6] >> (q & 63) & 1);
            for (int r = 1; r < Lr; ++r) {
                int id0 = r * W;
                cur_row[0] = (int)(omap[id0 >> 6] >> (id0 & 63) & 1);
                for (int q = 1; q < W; ++q) {
                    int id = r * W + q;
                    cur_row[q] = 0;
                    if (!(omap[id >> 6] >> (id & 63) & 1)) {
                        int m = prev_row[q] < cur_row[q - 1] ? prev_row[q] : cur_row[q - 1];
                        if (prev_row[q - 1] < m) m = prev_row[q - 1];
                        cur_row[q] = m + 1;
                        if (cur_row[q] > max_size) { max_size = cur_row[q]; cx = r - (max_size - 1) / 2; cy = q - (max_size - 1) / 2; }
                    }
                }
                for (int q = 0; q < W; ++q) prev_row[q] = cur_row[q];
            }
            int index = cx + W * cy, ii = index / W, jj = (W - 1) - (index - ii * W);
            real end[3] = {(real)ii + (real)0.5 - (real)(Lr / 2), (real)jj + (real)0.5 - (real)(W / 2), 0};
            end[2] = rng_uniform1<real>(key, QS_SITE_SCEN, 9, 0, 0, (real)1.5, (real)3);
            // update_formation_and_relate_param (:41): formation index, size, layer distance - unused here
            if (on_tape) tape_skip(key, 3);
            for (int k = 0; k < N; ++k) for (int q = 0; q < 3; ++q) goals[k * 3 + q] = end[q];
        } else {
            // swarm_vs_swarm.py:80-94 (reset) + :17-50 (formation_centers) + scenarios/utils.py:170-181 (get_z_value)
            const int period = draw_period<real>(key, 8, 4.0, 6.0, c.control_freq);
            p.scen_int[e] = period;
            s_envflag[epb + le] = (uint32_t)period;
            update_formation<real>(c.scenario, key, 0, N, F);
            real box = c.spawn_box, xy[2];
            rng_uniform<real, 2>(key, QS_SITE_SCEN, 9, 0, 0, -box, box, xy);
            real z = rng_uniform1<real>(key, QS_SITE_SCEN, 10, 0, 0, (real)-0.5 * box, (real)0.5 * box) + (real)2, zlb = (real)0.25;
            const int f = F.f;
            if (f == 3 || f == 1 || f == 2) zlb = F.size + (real)0.25;
            else if (f == 5 || f == 6) { int rn = N < F.per_layer ? N : F.per_layer, d1, d2; grid_dim(rn, &d1, &d2);
                zlb = (real)d1 * F.size + (real)0.25; }
            z = M<real>::fmax(zlb, z);
            real c1[3] = {xy[0], xy[1], z}, c2[3];
            real dist = rng_uniform1<real>(key, QS_SITE_SCEN, 11, 0, 0, box / (real)4, box);
            real phi = rng_uniform1<real>(key, QS_SITE_SCEN, 12, 0, 0, (real)-QS_PI_D, (real)QS_PI_D);
            real theta = rng_uniform1<real>(key, QS_SITE_SCEN, 13, 0, 0, (real)(-0.5 * QS_PI_D), (real)(0.5 * QS_PI_D));
            real st, ct, sp, cph; M<real>::sincos(theta, &st, &ct); M<real>::sincos(phi, &sp, &cph);
            c2[0] = c1[0] + dist * (st * cph); c2[1] = c1[1] + dist * (st * sp); c2[2] = c1[2] + dist * ct;
            int s = f_suffix(f), ax = (s == 0) ? 2 : ((s == 1) ? 1 : ((s == 2) ? 0 : -1));
            if (ax >= 0) {
                real df = c2[ax] - c1[ax];
                if (M<real>::fabs(df) < F.lo) { real sg = (real)((df > 0) - (df < 0)); c2[ax] = sg * F.lo + c1[ax]; }
            }
            for (int q = 0; q < 3; ++q) { p.scen_real[q * E + e] = c1[q]; p.scen_real[(3 + q) * E + e] = c2[q]; }
            svs_create_formations<real>(key, F, N, QS_CUBE_FD(c), c1, c2, false, goals);
        }
        s_envflag[le] = have_spawn;
#ifdef QS_TAPE
        if (QS_ON_TAPE(key)) s_cur[le] = *key.cur;
#endif
    }
    if (TEAM) QS_WAVE_SYNC(); else __syncthreads();   // team kernels: only wave 0 is here

    // ---- per-drone part: QuadrotorSingle._reset quadrotor_single.py:387-447 ----
    auto per_drone = [&]() {
        real spawn[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            goal[q] = s_goal[(le * L.goal_rows + i) * 3 + q];
            spawn[q] = s_envflag[le] ? s_spawn[q * B + tid] : goal[q];
        }
        real u[3];
        rng_uniform<real, 3>(key, QS_SITE_SPAWN, 0, i, 0, -c.spawn_box, c.spawn_box, u);
#pragma unroll
        for (int q = 0; q < 3; ++q) d.pos[q] = u[q] + spawn[q];
        if (d.pos[2] < (real)0.75) d.pos[2] = (real)0.75;
        real xy[3] = {-d.pos[0], -d.pos[1], 0}, n = norm3<real>(xy);
        if (n >= (real)0.00001) { xy[0] /= n; xy[1] /= n; }
        for (int t = 0; t < 256; ++t) {   // yaw rejection (:431-434)
            real th = rng_uniform1<real>(key, QS_SITE_SPAWN_YAW, t, i, 0, (real)-QS_PI_D, (real)QS_PI_D);
            yaw_rot<real>(th, d.rot);
            if (!(d.rot[0] * xy[0] + d.rot[3] * xy[1] < (real)0.5)) break;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) { s_vel[q * B + tid] = stale_vel[q]; s_pos[q * B + tid] = d.pos[q]; d.vel[q] = 0; d.omega[q] = 0; }
#pragma unroll
        for (int q = 0; q < 4; ++q) { d.rot_damp[q] = 0; d.cmds_damp[q] = 0; }
        d.flags = F_COL_AGENT_OK | F_COL_OBST_OK | (d.flags & F_SVD_MASK);   // since_last_svd persists (App. A)
        SensNoise<real> sn;
        if (c.sense_noise) sensor_noise_draw<real>(c, key, i, 0, sn);
        self_obs<real>(c, sn, d, goal, myobs);
    };
#ifdef QS_TAPE
    // the reference resets the drones one after the other (spawn draw, yaw rejection loop, sensor noise): take turns
    if (QS_ON_TAPE(key)) {
        for (int turn = 0; turn < N; ++turn) {
            if (do_reset && i == turn) { *key.cur = s_cur[le]; per_drone(); s_cur[le] = *key.cur; }
            __syncthreads();
        }
    } else
#endif
    if (do_reset) per_drone();
    if (TEAM) QS_WAVE_SYNC(); else __syncthreads();
    if (STREAM) {   // single-wave kernels: the rows of the re-initialised envs go out through the rows stage
        const uint64_t rowmask = __ballot(do_reset);
        const int first_env = bidx * epb;
        int nenv = E - first_env; nenv = nenv < epb ? nenv : epb;
        stream_rows<real>(c, L, p.obs + (size_t)first_env * N * c.obs_dim, (const real *)(smem + L.off_self),
            (real *)(smem + L.off_rows), N, i, le, base, tid,
                          s_pos, s_vel, s_metric, s_obst, d.pos, stale_vel, do_reset, nenv * N, rowmask,
                          c.dr_num_size > 0 ? (real)0.5 * p.dr_size[s_envflag[2 * epb + (le < epb ? le : 0)] & 7] : c.obst_radius);
    } else if (do_reset) {
        neighbor_obs<real>(c, N, i, base, B, tid, s_pos, s_vel, s_metric, d.pos, stale_vel, myobs + c.self_dim);
        if (c.use_obstacles)
            sdf_obs<real>(c, s_obst + (le * 2 + 0) * M_, s_obst + (le * 2 + 1) * M_, M_, d.pos[0], d.pos[1],
                myobs + c.self_dim + 6 * c.num_neighbors,
                          c.dr_num_size > 0 ? (real)0.5 * p.dr_size[s_envflag[2 * epb + le] & 7] : c.obst_radius);
    }
}

template <typename real, bool FULL>
__device__ __forceinline__ void qs_reset_impl(const Consts<real> &c, Ptrs<real> &p, const LdsLayout &L, int epb) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Consts<real> *cp = &c;
    const int N = c.num_agents, E = c.num_envs, T = E * N;
    const int tid = threadIdx.x, le = tid / N, i = tid - le * N, e = blockIdx.x * epb + le;
    const bool in_range = (le < epb) && (e < E);
    const bool do_reset = in_range && p.reset_mask[e] != 0;
    const int g = in_range ? e * N + i : 0;
    // an explicit reset takes the env's next draw counter, like a step does: consecutive resets (or a reset right after the
    // auto-reset of a finished episode) start different episodes
    const uint32_t ctr = in_range ? p.step_ctr[e] + 1u : 0u;
#ifdef QS_TAPE
    int *s_cur = (int *)(smem + L.off_cur);
    int cursor = 0;
    const double *tape_env = p.tape ? p.tape + (size_t)(in_range ? e : 0) * (size_t)p.tape_len : nullptr;
    if (tape_env && in_range && i == 0) s_cur[le] = p.tape_pos[e];
    __syncthreads();
    RngKey key = {c.seed_lo, c.seed_hi, (uint32_t)(c.env_id_offset + (in_range ? e : 0)), ctr, tape_env, &cursor};
#else
    RngKey key = {c.seed_lo, c.seed_hi, (uint32_t)(c.env_id_offset + (in_range ? e : 0)), ctr};
#endif
    Drone<real> d;
    real goal[3] = {0, 0, 0}, stale_vel[3];
    const int es = in_range ? e : 0;   // (inactive lanes read drone 0's slot of a valid env, as before)
#pragma unroll
    for (int q = 0; q < 3; ++q) stale_vel[q] = QS_BLK_AT(real, p.blk, vel, q, es, in_range ? i : 0, N);
    d.flags = QS_BLK_AT(uint32_t, p.blk, flags, 0, es, in_range ? i : 0, N);
    if (FULL && in_range) scen_lds_load<real>(p, L, smem, E, e, le, i, N);
    if (FULL) __syncthreads();
    reset_body<real, FULL, false, true>(cp, &p, &L, smem, epb, key, do_reset, &d, goal, stale_vel);   // writes the obs rows itself
    if (FULL) { __syncthreads(); if (do_reset) scen_lds_store<real>(p, L, smem, E, e, le, i, N); }
    if (do_reset) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            QS_BLK_AT(real, p.blk, pos, q, e, i, N) = d.pos[q]; QS_BLK_AT(real, p.blk, vel, q, e, i, N) = 0;
            QS_BLK_AT(real, p.blk, omega, q, e, i, N) = 0; QS_BLK_AT(real, p.blk, goal, q, e, i, N) = goal[q];
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) QS_BLK_AT(real, p.blk, rot, q, e, i, N) = d.rot[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) { QS_BLK_AT(real, p.blk, rot_damp, q, e, i, N) = 0;
            QS_BLK_AT(real, p.blk, cmds_damp, q, e, i, N) = 0; QS_BLK_AT(real, p.blk, ring, q, e, i, N) = 0; }
#pragma unroll
        // the step kernels leave the sums alone until the episode's 5-s window opens (qs_step_sem.h)
        for (int q = 0; q < 3; ++q) QS_BLK_AT(real, p.blk, sums, q, e, i, N) = 0;
        QS_BLK_AT(uint32_t, p.blk, flags, 0, e, i, N) = d.flags;
        QS_BLK_AT(uint64_t, p.blk, pair, 0, e, i, N) = 0;
        p.new_pair_mask[g] = 0;
        p.obst_hit_idx[g] = -1;
        if (c.episode_sums) {
            for (int q = 0; q < QS_SUM_COUNT; ++q) p.run_sums[q * T + g] = 0;
        }
        if (i == 0) {
            for (int q = 0; q < QS_CNT_COUNT; ++q) p.counters[q * E + e] = 0;
            p.tick[e] = 0;
            p.unique_col[e] = 0; p.obst_new[e] = 0; p.room_new[e] = 0;
            p.reset_mask[e] = 0;
            p.step_ctr[e] = ctr;
#ifdef QS_TAPE
            if (tape_env) p.tape_pos[e] = s_cur[le];
#endif
        }
    }
}

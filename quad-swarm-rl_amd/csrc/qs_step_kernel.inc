// qs_step_kernel.inc - body of the step kernel, included twice by qs_step_kernel_modes.inc (the tape flavour: by qs_step_flavours.inc):
//   QS_MULTI 0 -> qs_step_kernel<real>    : one control step per launch (qs_step)
//   QS_MULTI 1 -> qs_rollout_kernel<real> : `ksteps` control steps per launch, state in registers in between (qs_step_many)
// Textual inclusion (instead of a template flag) keeps the two kernels' code generation independent: register /
// SGPR pressure of this kernel is at the edge, and a shared instantiation cost the single-step kernel 8-25 %.
// ------------------------------------------------------------------------------------------------
// THE step kernel: `ksteps` control steps of every environment (= QuadrotorEnvMulti.step incl. the auto-reset tail,
// ksteps times with actions[t] = actions + t*T*4).  The dynamic state is loaded once at the top and stored once at the
// bottom; in between the wave works in registers + LDS only.  ksteps = 1 is the interactive step (qs_step); an
// open-loop rollout with pre-generated actions (qs_step_many) keeps the state in registers across its steps, so per
// step only the action is read and obs / reward / done (+ bookkeeping masks) are written.
// ------------------------------------------------------------------------------------------------
// Throughput layout (this file is what large batches run: thousands of one-wave workgroups, several per SIMD):
//   * observation rows leave through a small rows stage, a row group at a time, as whole contiguous rows (stream_rows /
//     obs_copy_rows, qs_obs_rows.h): ~9.5 KB of LDS per workgroup instead of ~21 KB, i.e. 16 instead of 7 workgroups per CU;
//   * the single-step kernel (QS_MULTI 0) loads a value when it is first needed and stores it when it is final (motor filters
//     and OU state right after the sub-steps, distance ring / sums / counters inside the bookkeeping) instead of "all loads
//     first, all stores last": the latency this exposes is hidden by the other waves of the SIMD, and the register file is what
//     decides how many of them there are.  The rollout kernel keeps its state in registers across steps as before.
#undef e_state_or_e
#undef QS_LATE
#if QS_MULTI
#define QS_LATE 0
#else
#define QS_LATE 1
#endif
// per-step outputs of one drone / env (NP new-pair mask, OI obstacle hit index, UQ / ON / RM the env's id sets of this step)
#undef QS_STORE_OUTPUTS
#define QS_STORE_OUTPUTS(NP, OI, UQ, ON, RM) \
    if (active) { \
        {   /* lane offsets from this step's (opaque) g: see the note at the top of the loop */ \
            QS_ROWF(uint64_t, newpair, rs, p, T, g); QS_ROWF(int32_t, ohit, rs, p, T, g); QS_ROWF(real, reward, rs, p, T, g); QS_ROWF(uint8_t, done, rs, p, T, g); \
            if (np_store) b_newpair.st(NP);            /* (wave-uniform: some lane has a new pair, or had one stored last time) */ \
            if (c.use_obstacles) b_ohit.st(OI);        /* without obstacles the word keeps the -1 of the reset */ \
            b_reward.st(rew); b_done.st(done ? 1 : 0); \
        } \
        if (c.write_rew_info) { \
            _Pragma("unroll") for (int q = 0; q < QS_RI_COUNT; ++q) p.rew_info[q * T + g] = ri[q]; \
        } \
        if (c.episode_sums) {   /* reward_shaping.py:78-110 on the device: running sums in HBM (read-modify-write; no registers held across steps) */ \
            const bool fin = done;   /* the sums of a finished episode include its last step, then restart from zero */ \
            _Pragma("unroll") for (int q = 0; q < QS_SUM_COUNT; ++q) { \
                const real add = q < QS_RI_COUNT ? ri[q < QS_RI_COUNT ? q : 0] : (q < QS_SUM_ACT2 ? act[(q - QS_SUM_ACT) & 3] : act[(q - QS_SUM_ACT2) & 3] * act[(q - QS_SUM_ACT2) & 3]); \
                const real v = p.run_sums[q * T + g] + add; \
                if (fin) p.ep_sums[q * T + g] = v; \
                p.run_sums[q * T + g] = fin ? (real)0 : v; \
            } \
        } \
        if (i == 0) { p.unique_col[e] = (UQ); p.obst_new[e] = (ON); p.room_new[e] = (RM); } \
    }
#define QS_PCHUNK 8   // partners per batch of LDS reads in the pair scan
#if QS_MULTI
#define e_state_or_e e_state
#else
#define e_state_or_e e
#endif
#ifdef QS_SPEC
// Occupancy target of the single-step throughput kernel: 4 waves per SIMD = 128 VGPRs (the fp32 kernels need ~126-128; the LDS
// layout above allows 16 workgroups per CU).  -DQS_WAVES_PER_EU=n overrides (0 = no hint); the f64 parity kernels and the
// rollout kernel (state of all steps in registers) are left alone.
#undef QS_OCC
#if QS_MULTI || (QS_SPEC_PRECISION == 8 && !defined(QS_WAVES_PER_EU))
#define QS_OCC
#elif !defined(QS_WAVES_PER_EU)
#define QS_OCC __attribute__((amdgpu_waves_per_eu(4, 4)))
#elif QS_WAVES_PER_EU == 0
#define QS_OCC
#else
#define QS_OCC __attribute__((amdgpu_waves_per_eu(QS_WAVES_PER_EU, QS_WAVES_PER_EU)))
#endif
#if QS_MULTI
extern "C" __global__ void QS_OCC __launch_bounds__(QS_WAVE) qs_spec_rollout(QS_KARGS, int QS_EPB_ARG, int ksteps) {
#else
extern "C" __global__ void QS_OCC __launch_bounds__(QS_WAVE) qs_spec_step(QS_KARGS, int QS_EPB_ARG) {
    const int t = 0;
#endif
#else
template <typename real>
#if QS_MULTI && QS_SCEN_FULL
__global__ void __launch_bounds__(QS_WAVE) qs_rollout_kernel_full(QS_KARGS, int QS_EPB_ARG, int ksteps) {
#elif QS_MULTI
__global__ void __launch_bounds__(QS_WAVE) qs_rollout_kernel(QS_KARGS, int QS_EPB_ARG, int ksteps) {
#elif QS_SCEN_FULL
__global__ void __launch_bounds__(QS_WAVE) qs_step_kernel_full(QS_KARGS, int QS_EPB_ARG) {
    const int t = 0;
#else
__global__ void __launch_bounds__(QS_WAVE) qs_step_kernel(QS_KARGS, int QS_EPB_ARG) {
    const int t = 0;
#endif
#endif
    extern __shared__ __align__(16) unsigned char smem[];
    QS_SPEC_PROLOGUE
    const Consts<real> *cp = &c;
    // reward coefficients + proximity slope: read from device memory on every launch, so that the reward-shaping wrapper's
    // updates (qs_set_reward_coeffs) also reach launches that were captured into a HIP graph
    real rewc[QS_REW_COUNT + 1];
#pragma unroll
    for (int q = 0; q <= QS_REW_COUNT; ++q) rewc[q] = p.rew_rt[q];
#define QS_OBST_SIZE (c.dr_on ? p.obst_size_env[ee] : c.obst_size)   /* --quads_domain_random: the running episode's obstacle size */
    const int B = QS_WAVE, N = c.num_agents, E = c.num_envs, T = E * N, M_ = c.num_obstacles;
    uint64_t *s_mask = (uint64_t *)(smem + L.off_mask);
    uint32_t *s_envflag = (uint32_t *)(smem + L.off_envflag);
    real *s_pos = (real *)(smem + L.off_pos), *s_vel = (real *)(smem + L.off_vel), *s_zax = (real *)(smem + L.off_zax);
    real *s_om = (real *)(smem + L.off_om), *s_goal = (real *)(smem + L.off_goal), *s_obs = (real *)(smem + L.off_obs);
    real *s_obst = (real *)(smem + L.off_obst), *s_metric = (real *)(smem + L.off_metric);
    QS_POISON_LDS(L.total, QS_WAVE);

    const int tid = threadIdx.x, le = tid / N, i = tid - le * N, e = blockIdx.x * epb + le, base = le * N;
    const bool active = (le < epb) && (e < E);
    const int g = active ? e * N + i : 0, ee = active ? e : 0;
    const uint64_t nmask = (N >= 64) ? ~0ull : ((1ull << N) - 1);
    real *myobs = (real *)(smem + L.off_self) + tid * c.self_dim;   // this lane's row of the dense self block (obs_copy_rows, qs_obs_rows.h)
    const int first_env = blockIdx.x * epb, nrows = ((E - first_env) < epb ? (E - first_env) : epb) * N;
    real *const obs_block = p.obs + (size_t)first_env * N * c.obs_dim;   // the workgroup's rows of the row-major observation matrix
#ifdef QS_TAPE   // noise-tape flavour (qs_tape_kernels.hip): the env's cursor lives in LDS, the lane that draws works on a private copy
    int *s_cur = (int *)(smem + L.off_cur);
    int cursor = 0;
    const double *tape_env = p.tape ? p.tape + (size_t)(active ? e : 0) * (size_t)p.tape_len : nullptr;
    if (tape_env && active && i == 0) s_cur[le] = p.tape_pos[e];
    int *const s_cur_env = s_cur + le;
    const double *const tape_env_or_null = tape_env;
#else
    int *const s_cur_env = nullptr;
    const double *const tape_env_or_null = nullptr;
#endif
    const __amdgpu_buffer_rsrc_t rs = QS_BUF_RSRC(p);
    QS_ROW(real, pos, rs, p, T, g); QS_ROW(real, vel, rs, p, T, g); QS_ROW(real, rot, rs, p, T, g); QS_ROW(real, omega, rs, p, T, g);
    QS_ROW(real, rot_damp, rs, p, T, g); QS_ROW(real, cmds_damp, rs, p, T, g); QS_ROW(real, ou, rs, p, T, g);
    QS_ROW(real, goal, rs, p, T, g);
    QS_ROW(real, ring, rs, p, T, g); QS_ROW(real, sums, rs, p, T, g); QS_ROW(uint32_t, flags, rs, p, T, g);
    QS_ROW(uint64_t, pair, rs, p, T, g);

    QS_STAMP(0);
    // ================= loads (coalesced: component-major SoA) =================
    Drone<real> d;
    real goal[3], act[4], ring[4], sums[3];
    int32_t cnt[QS_CNT_COUNT];
#pragma unroll
    for (int q = 0; q < 3; ++q) { d.pos[q] = b_pos.ld(q); d.vel[q] = b_vel.ld(q); d.omega[q] = b_omega.ld(q); }
#pragma unroll
    for (int q = 0; q < 9; ++q) d.rot[q] = b_rot.ld(q);
#pragma unroll
    for (int q = 0; q < 4; ++q) { d.rot_damp[q] = b_rot_damp.ld(q); d.cmds_damp[q] = b_cmds_damp.ld(q); d.ou[q] = b_ou.ld(q); }
    d.flags = b_flags.ld();
    QS_POISON_DRONE(d);
#if !QS_LATE
#pragma unroll
    for (int q = 0; q < 3; ++q) { goal[q] = b_goal.ld(q); sums[q] = b_sums.ld(q); }
#pragma unroll
    for (int q = 0; q < 4; ++q) ring[q] = b_ring.ld(q);
    uint64_t prev_pair = b_pair.ld();
    QS_POISON_ARR(goal, 3, 16); QS_POISON_ARR(sums, 3, 16); QS_POISON_ARR(ring, 4, 16); QS_POISON_U64(prev_pair);
    if (active && i == 0) {
#pragma unroll
        for (int q = 0; q < QS_CNT_COUNT; ++q) cnt[q] = p.counters[q * E + ee];
    }
#endif
    int tick_before = p.tick[ee];
    uint32_t step_no = p.step_ctr[ee] + 1;
    int svs_period = (c.scenario == QS_SCENARIO_SWARM_VS_SWARM) ? p.scen_int[ee] : 0;
    if (c.use_obstacles && active) {   // stage the env's obstacle positions in LDS
        for (int k = i; k < M_; k += N) {
            s_obst[(le * 2 + 0) * M_ + k] = p.obst_pos[(size_t)e * M_ + k];
            s_obst[(le * 2 + 1) * M_ + k] = p.obst_pos[(size_t)E * M_ + (size_t)e * M_ + k];
        }
    }
#if QS_SCEN_FULL
    if (active) scen_lds_load<real>(p, L, smem, E, e, le, i, N);   // first read after the barrier that follows the self obs
    real *s_sr = (real *)(smem + L.off_sr) + le * SR_COUNT;
    int *s_si = (int *)(smem + L.off_si) + le * SI_COUNT;
#endif
    uint64_t out_curr_pair = 0;
    bool nan_any = false;
#if QS_MULTI
    bool goal_dirty = true;    // (the multi-step kernels write the state once, at the end of the launch)
#else
    bool goal_dirty = false;
#endif
#if QS_MULTI
    const int g_state = g, e_state = e;
    for (int t = 0; t < ksteps; ++t) {
    // Opaque copies of the drone / env index: keeps the ~60 output addresses of the loop body from being hoisted out
    // of the loop as live 64-bit pointers (they are recomputed from g / e in each step instead).
    int g = g_state, e = e_state;
    asm volatile("" : "+v"(g), "+v"(e));
#endif
    {   // actions are row-major [T,4]: one 16/32-byte vector load per lane
        const real *a = actions + ((size_t)t * T + g) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) act[q] = a[q];
        QS_POISON_ARR(act, 4, 8);
    }
#if !QS_LATE
    // this kernel writes new_pair_mask on every step: the word is "possibly non-zero" for the kernels that skip zero stores
    d.flags |= F_NEWPAIR_NZ;
#endif
#ifdef QS_TAPE
    RngKey key = {c.seed_lo, c.seed_hi, (uint32_t)(c.env_id_offset + ee), step_no, tape_env, &cursor};
#else
    RngKey key = {c.seed_lo, c.seed_hi, (uint32_t)(c.env_id_offset + ee), step_no};
#endif
    real zou[4];
    SensNoise<real> sn;
#if !QS_LATE
    // The random draws of the per-drone phase do not depend on the state: generating them here overlaps the
    // Philox / Box-Muller arithmetic with the HBM latency of the loads above.  (step_no is uniform per env and
    // the first value the wave waits for.)
    step_noise_draw<real>(c, key, i, zou, sn);
#endif

    QS_STAMP(1);
    // ================= A. per-drone step =================
    // RawControl quadrotor_control.py:53-57, OU noise quad_utils.py:275-279, 2 sub-steps (qs_device.h),
    // reward quadrotor_single.py:34-92, tick/done :352-353, self obs get_state.py + sensor_noise.py
    real rew = 0, ri[QS_RI_COUNT];
    auto phase_a = [&]() __attribute__((always_inline)) {
#if QS_LATE
        rng_normal<real, 4>(key, QS_SITE_OU, 0, i, 0, zou);   // the sensor noise is drawn where it is used (same sites / slots / values)
#endif
        real cmds[4], acc[3];
        control_and_thrust_noise<real>(c, act, zou, d, cmds);
        QS_STAMP(2);
        for (int s = 0; s < c.sim_steps; ++s) substep<real>(c, key, i, s, d, cmds, acc);
        QS_STAMP(3);
#if QS_LATE
        if (active) {   // final for this step (an auto-reset rewrites the two filters below): their registers are free from here on
#pragma unroll
            for (int q = 0; q < 4; ++q) { b_rot_damp.st(d.rot_damp[q], q); b_cmds_damp.st(d.cmds_damp[q], q); b_ou.st(d.ou[q], q); }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) goal[q] = b_goal.ld(q);
        QS_POISON_ARR(goal, 3, 16);
        if (c.sense_noise) sensor_noise_draw<real>(c, key, i, 0, sn);
#endif
        main_reward<real>(c, rewc, d, goal, act, rew, ri);
        QS_STAMP(4);
        self_obs<real>(c, sn, d, goal, myobs);
    };
#ifdef QS_TAPE
    // the reference steps the drones of an env one after the other (OU draw, floor-contact yaw draws, 27 sensor draws): take turns
    if (QS_ON_TAPE(key)) {
        __syncthreads();
        for (int turn = 0; turn < N; ++turn) {
            if (active && i == turn) { cursor = s_cur[le]; phase_a(); s_cur[le] = cursor; }
            __syncthreads();
        }
    } else
#endif
    phase_a();
    const bool nan_rew = not_finite(rew);
    const int tick = tick_before + 1;
    const bool done = tick > c.ep_len;
    QS_STAMP(5);
#pragma unroll
    for (int q = 0; q < 3; ++q) s_pos[q * B + tid] = d.pos[q];
    s_zax[0 * B + tid] = d.rot[2]; s_zax[1 * B + tid] = d.rot[5]; s_zax[2 * B + tid] = d.rot[8];
    __syncthreads();
    // Bookkeeping rows that only matter on some steps (qs_step_sem.h / qs_device.h F_RING_LIVE, F_NEWPAIR_NZ): wave-uniform decisions,
    // so that a wave whose 64 drones all do not need a row issues neither its loads nor its stores (36 + 44 bytes per drone-step in
    // the steady state of a random-action rollout: profiles/r04*_bytes*).
#if QS_SCEN_FULL
    const real goal_metric = active ? s_sr[SR_METRIC] : (real)0;
#else
    const real goal_metric = c.approach_goal_metric;
#endif
    const int tick_now = tick_before + 1;
    const bool ring_io = __ballot(active && ring_needed<real>(c, goal_metric, d.flags, ri)) != 0;
    const bool sums_io = __ballot(active && sums_window_open<real>(c, tick_now)) != 0;
    // someone was in a colliding pair last step: its mask is non-zero
    const bool pair_early = __ballot(active && (d.flags & F_IN_COL)) != 0;
#if QS_LATE
    uint64_t prev_pair = 0;
    if (pair_early) prev_pair = b_pair.ld();   // bookkeeping inputs: in flight during the pair scan
    if (sums_io) {
#pragma unroll
        for (int q = 0; q < 3; ++q) sums[q] = b_sums.ld(q);
    } else { sums[0] = sums[1] = sums[2] = 0; }
    if (ring_io) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ring[q] = b_ring.ld(q);
    } else { ring[0] = ring[1] = ring[2] = ring[3] = 0; }
    QS_POISON_ARR(sums, 3, 16); QS_POISON_ARR(ring, 4, 16); QS_POISON_U64(prev_pair);
#endif

    // ================= B. pair scan, obstacle first hit, room lists =================
    uint64_t curr_pair = 0, dw_mask = 0;
    bool in_curr = false;
    real prox = 0;
    uint32_t bits = 0;
    int obst_idx = -1;
    if (active) {
        // calculate_collision_matrix collisions/quadrotors.py:63-91, proximity penalties :95-103 and the downwash
        // cylinder test of aerodynamics/downwash.py:30-45 share the relative position; 8 partners per iteration so the
        // LDS reads are issued together
        const real pr = rewc[QS_REW_COUNT];
        for (int j0 = 0; j0 < N; j0 += QS_PCHUNK) {
            real dist_[QS_PCHUNK], rz_[QS_PCHUNK], rxy2_[QS_PCHUNK];   // |rel|, rel . z_j, |rel|^2 - rz^2 of the chunk's partners
            // float32, more than 8 drones: two partners per packed instruction, the multiply-add chains of the scalar form written out
            // (8 drones: no gain, 16 B of scratch per lane - profiles/r06s2_ab_keys_packed_scan.txt)
            if (sizeof(real) == 4 && N > 8) {
#pragma unroll
                for (int h = 0; h < QS_PCHUNK / 2; ++h) {
                    const int ja = (j0 + 2 * h < N) ? j0 + 2 * h : N - 1, jb = (j0 + 2 * h + 1 < N) ? j0 + 2 * h + 1 : N - 1;
                    qs_f32x2 rel[3], zx[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const qs_f32x2 pj = {(float)s_pos[a * B + base + ja], (float)s_pos[a * B + base + jb]};
                        rel[a] = (float)d.pos[a] - pj;
                        zx[a] = qs_f32x2{(float)s_zax[a * B + base + ja], (float)s_zax[a * B + base + jb]};
                    }
                    const qs_f32x2 d2 = __builtin_elementwise_fma(rel[2], rel[2], __builtin_elementwise_fma(rel[1], rel[1], rel[0] * rel[0]));
                    const qs_f32x2 dist = {__builtin_amdgcn_sqrtf(d2.x), __builtin_amdgcn_sqrtf(d2.y)};
                    const qs_f32x2 rz = __builtin_elementwise_fma(rel[2], zx[2], __builtin_elementwise_fma(rel[1], zx[1], rel[0] * zx[0]));
                    const qs_f32x2 r2 = __builtin_elementwise_fma(-rz, rz, dist * dist);
                    dist_[2 * h] = dist.x; dist_[2 * h + 1] = dist.y; rz_[2 * h] = rz.x; rz_[2 * h + 1] = rz.y;
                    rxy2_[2 * h] = r2.x; rxy2_[2 * h + 1] = r2.y;
                }
            } else {
                real rel[QS_PCHUNK][3], zx[QS_PCHUNK][3];
#pragma unroll
                for (int u = 0; u < QS_PCHUNK; ++u) {
                    const int j = (j0 + u < N) ? j0 + u : N - 1;
#pragma unroll
                    for (int a = 0; a < 3; ++a) { rel[u][a] = d.pos[a] - s_pos[a * B + base + j]; zx[u][a] = s_zax[a * B + base + j]; }
                }
#pragma unroll
                for (int u = 0; u < QS_PCHUNK; ++u) {
                    dist_[u] = M<real>::sqrt(rel[u][0] * rel[u][0] + rel[u][1] * rel[u][1] + rel[u][2] * rel[u][2]);
                    rz_[u] = dot3<real>(rel[u], zx[u]);
                    rxy2_[u] = dist_[u] * dist_[u] - rz_[u] * rz_[u];
                }
            }
            uint32_t hbits = 0, dbits = 0;   // this chunk's bits at literal positions: one 64-bit shift per chunk, not per partner
#pragma unroll
            for (int u = 0; u < QS_PCHUNK; ++u) {   // branch-free: `&&` on lane-varying conditions compiles to exec-mask branches
                const int j = j0 + u;
                const bool other = (j < N) & (j != i);
                const real dist = dist_[u], rz = rz_[u];
                const bool hit = other & (dist <= c.collision_threshold);
                in_curr |= hit;
                hbits |= (hit & (j > i)) ? (1u << u) : 0u;
                prox += (other & (dist <= c.collision_falloff_threshold)) ? pr * dist + rewc[QS_REW_QUADCOL_SMOOTH_MAX] : (real)0;
                const real rxy = M<real>::sqrt(rxy2_[u]);
                dbits |= (other & ((real)-0.7 < rz) & (rz < (real)0) & (rxy < (real)0.1)) ? (1u << u) : 0u;   // drone j is above me
            }
            curr_pair |= (uint64_t)hbits << j0; dw_mask |= (uint64_t)dbits << j0;
        }
        if (c.use_obstacles) {   // first hit in index order, obstacles/utils.py:31-43
            const real *ox = s_obst + (le * 2 + 0) * M_, *oy = s_obst + (le * 2 + 1) * M_;
            for (int k = M_ - 1; k >= 0; --k) {
                real dx = d.pos[0] - ox[k], dy = d.pos[1] - oy[k];
                obst_idx = (M<real>::sqrt(dx * dx + dy * dy) <= (c.dr_on ? c.arm_r + (real)0.5 * QS_OBST_SIZE : c.obst_hit_threshold))
                    ? k : obst_idx;
            }
            obstacle_hit_bits(obst_idx, d.flags, bits);
        }
        room_collision_bits(d.flags, bits);
    }
    QS_STAMP(6);
    // ---- env-level id sets, collision rewards, distance-to-goal log: qs_step_sem.h (quadrotor_multi.py:432-546, :649-661) ----
    const uint64_t new_pair = curr_pair & ~prev_pair;                                  // pair-level novelty (:437-438)
    const EnvEvents ev = env_events<real>(c, active, in_curr, new_pair, bits, d.flags, base, nmask, i, tick, tick_before, myobs);
    const uint64_t unique = ev.unique, m_obst_new = ev.obst_new, m_room = ev.room;
    collision_rewards<real>(c, rewc, ev, i, bits, prox, rew, ri);
    real eps_dist[3] = {0, 0, 0};
    goal_distance_log<real, (QS_LATE != 0)>(c, goal_metric, tick, done, d.flags, ring, sums, ri, eps_dist);
    // ---- episode snapshot of a finishing episode (:626-718): every input is final here (the flags it reads are not touched
    //      by the interactions below) ----
    if (active && done) {
        p.ep_stats[QS_EPS_DIST_1S * T + g] = eps_dist[0]; p.ep_stats[QS_EPS_DIST_3S * T + g] = eps_dist[1];
        p.ep_stats[QS_EPS_DIST_5S * T + g] = eps_dist[2];
        p.ep_stats[QS_EPS_REACHED_GOAL * T + g] = (d.flags & F_REACHED) ? (real)1 : (real)0;
        p.ep_stats[QS_EPS_COL_AGENT_OK * T + g] = (d.flags & F_COL_AGENT_OK) ? (real)1 : (real)0;
        p.ep_stats[QS_EPS_COL_OBST_OK * T + g] = (d.flags & F_COL_OBST_OK) ? (real)1 : (real)0;
#if QS_SCEN_FULL
        if (i == 0) p.ep_scenario[e] = s_si[SI_SCEN];
#else
        if (i == 0) p.ep_scenario[e] = c.scenario;
#endif
    }
#if QS_LATE
    if (active) {   // final for this step (an auto-reset clears F_RING_LIVE with the other flags: the ring row needs no store for it)
        if (sums_io) {
#pragma unroll
            for (int q = 0; q < 3; ++q) b_sums.st(sums[q], q);
        }
        if (ring_io) {
#pragma unroll
            for (int q = 0; q < 4; ++q) b_ring.st(ring[q], q);
        }
    }
#endif
    // ---- per-env counters (lane 0 of the env) ----
    if (active && i == 0) {
#if QS_LATE
#pragma unroll
        for (int q = 0; q < QS_CNT_COUNT; ++q) cnt[q] = p.counters[q * E + e];
#endif
        env_counters_add<real>(c, cnt, ev);
        if (done) {
#pragma unroll
            for (int q = 0; q < QS_CNT_COUNT; ++q) { p.ep_counters[q * E + e] = cnt[q]; cnt[q] = 0; }
        }
#if QS_LATE
#pragma unroll
        for (int q = 0; q < QS_CNT_COUNT; ++q) p.counters[q * E + e] = cnt[q];
#endif
    }

#if QS_LATE
    // ---- per-step outputs and the bookkeeping part of the state: all final here (an auto-reset zeroes the id sets) ----
    {
        const uint64_t np_out = done ? 0ull : new_pair;
        const bool np_store = __ballot(active && (np_out != 0 || (d.flags & F_NEWPAIR_NZ))) != 0;
        d.flags = np_out != 0 ? (d.flags | F_NEWPAIR_NZ) : (d.flags & ~F_NEWPAIR_NZ);
        QS_STORE_OUTPUTS(np_out, done ? -1 : obst_idx, done ? 0ull : unique, done ? 0ull : m_obst_new, done ? 0ull : m_room)
    }
    if (active) {
        // the pair-mask row: all zeros before (nobody carried F_IN_COL) and all zeros now (no hit in the wave) => nothing to write
        if (pair_early || __ballot(active && in_curr) != 0) b_pair.st(done ? 0ull : curr_pair);
        if (i == 0) { p.tick[e] = done ? 0 : tick; p.step_ctr[e] = step_no; }
    }
#endif
    QS_STAMP(7);
    // ================= C. physical interactions, in the reference's order (:548-587) =================
    // (qs_step_sem.h) 1) downwash, 2) drone-drone responses of the new pairs, 3) obstacle, 4) wall then ceiling
    downwash_phase<real>(c, key, d, s_pos, s_zax, B, base, nmask, N, i, active, dw_mask, bits, s_cur_env, tape_env_or_null, BlockSync());
    QS_STAMP(8);
    const bool any_dw = ((__ballot(active && (bits & B_DOWNWASH)) >> base) & nmask) != 0;
    pair_responses<real>(key, d, ev, new_pair, active, N, i, tid, base, B, s_pos, s_vel, s_om, s_mask, s_cur_env, BlockSync());
    room_obstacle_phase<real>(cp, key, d, active, N, i, bits, obst_idx, s_obst + (le * 2 + 0) * M_, s_obst + (le * 2 + 1) * M_,
        p.obst_size_env + ee, s_cur_env, BlockSync());
    const bool update_flag = any_dw || (ev.newpair_any != 0) || (ev.obst_new != 0) || (ev.wall != 0) || (ev.ceil != 0);

    // ================= D. scenario.step() (qs_step_sem.h; qs_scenarios.h) =================
    // goal rows in HBM: rewritten only by the steps that change a goal of the wave (the fast scenario set: a swarm_vs_swarm swap or an
    // auto-reset; the scenarios of the full set may move goals on any step)
#if QS_SCEN_FULL
    goal_dirty = true;
    {
        ScenCtx<real> x = {s_sr, s_si, (uint64_t *)(smem + L.off_omap) + le * 4, s_goal + le * L.goal_rows * 3, s_zax, B, base, N};
        scenario_phase_full<real>(c, key, x, active, N, i, tick, goal, (int *)s_mask + base, s_cur_env, BlockSync());
    }
#else
    goal_dirty |= svs_phase<real>(c, p, key, active, N, E, e, i, tick, svs_period, s_goal + le * L.goal_rows * 3, (int *)s_mask + base,
        goal, s_cur_env, BlockSync());
#endif

    QS_STAMP(9);
    // ================= E. final observations (:592-607) =================
#pragma unroll
    for (int q = 0; q < 3; ++q) s_vel[q * B + tid] = d.vel[q];
    QS_STAMP(14);
#ifdef QS_TAPE
    if (QS_ON_TAPE(key)) __syncthreads();   // the env's cursor as the last interaction left it
#endif
    if (__builtin_expect(update_flag && active, 0)) {   // fresh sensor noise, new goal (:598-599)
#ifdef QS_TAPE
        if (QS_ON_TAPE(key)) cursor = s_cur[le] + 27 * i;   // 27 draws per drone, in drone order
#endif
        if (c.sense_noise) sensor_noise_draw<real>(c, key, i, 1, sn);
        self_obs<real>(c, sn, d, goal, myobs);
    }
#ifdef QS_TAPE
    if (QS_ON_TAPE(key)) {
        __syncthreads();
        if (update_flag && active && i == 0 && c.sense_noise) s_cur[le] += 27 * N;
    }
#endif
    QS_STAMP(15);
    __syncthreads();
    QS_STAMP(16);
    // the observation rows leave: neighbour / SDF values in registers, a row group at a time through the rows stage together with
    // the self columns (which stayed in LDS for the noisy relative position above and the refresh just now)
    stream_rows<real>(c, L, obs_block, (const real *)(smem + L.off_self), (real *)(smem + L.off_rows), N, i, le, base, tid, s_pos, s_vel,
        s_metric, s_obst,
                      d.pos, d.vel, active, nrows, ~0ull, c.dr_on ? (real)0.5 * QS_OBST_SIZE : c.obst_radius);

    QS_STAMP(10);
    // ================= F. done: episode snapshot + auto-reset (:626-722) =================
    uint64_t out_unique = unique, out_obst_new = m_obst_new, out_room = m_room, out_new_pair = new_pair;
    out_curr_pair = curr_pair;
    int out_tick = tick, out_obst_idx = obst_idx;
    const bool do_reset = active && done;
    if (__builtin_expect(__ballot(do_reset) != 0, 0)) {
        goal_dirty = true;
        real stale_vel[3] = {d.vel[0], d.vel[1], d.vel[2]};
        __syncthreads();   // the last row group has left the stage
        // rewrites the rows of these envs
        reset_body<real, (QS_SCEN_FULL != 0), false, true>(cp, &p, &L, smem, epb, key, do_reset, &d, goal, stale_vel, (int)blockIdx.x);
        if (do_reset) {
            out_unique = 0; out_obst_new = 0; out_room = 0; out_curr_pair = 0; out_new_pair = 0; out_tick = 0; out_obst_idx = -1;
            ring[0] = ring[1] = ring[2] = ring[3] = 0;
            if (c.scenario == QS_SCENARIO_SWARM_VS_SWARM) svs_period = (int)s_envflag[epb + le];   // new U(4,6) s period
#if QS_LATE
#pragma unroll
            // after the stores that followed the sub-steps
            for (int q = 0; q < 4; ++q) { b_rot_damp.st((real)0, q); b_cmds_damp.st((real)0, q); }
#endif
        }
    }

    QS_STAMP(11);
    // ================= G. per-step outputs (the observation rows have left through the stage already) =================
    QS_STAMP(12);
#if !QS_LATE
    {
        // (rollout kernels: the state lives in registers, the output rows are written every step; F_NEWPAIR_NZ raised at the top of the
        // step)
        const bool np_store = true;
        QS_STORE_OUTPUTS(out_new_pair, out_obst_idx, out_unique, out_obst_new, out_room)
    }
#endif
    nan_any |= nan_rew;
    // loop-carried values of the next control step
#if !QS_LATE
    prev_pair = out_curr_pair;
#endif
    tick_before = out_tick;
    step_no += 1;
#if QS_MULTI
    if (t + 1 < ksteps) __syncthreads();   // the next step rewrites the stage / exchange rows this one has been reading
    }   // for t
#endif

#ifdef QS_TAPE
    if (tape_env) {
        __syncthreads();
        if (active && i == 0) p.tape_pos[e] = s_cur[le];
    }
#endif
    // ================= H. state stores (nothing waits on them: they are the last instructions of the wave) =================
#if QS_SCEN_FULL
    __syncthreads();
    if (active) scen_lds_store<real>(p, L, smem, E, e_state_or_e, le, i, N);
#endif
    if (active) {
#if QS_MULTI
        const int g = g_state, e = e_state;
#endif
        // fresh views for the stores: their ~45 scalar offsets are recomputed here (one SALU add each) instead of being kept
        // alive in SGPRs from the load phase, which is what the compiler does when it can see that they are the same values
        uint32_t Ts = (uint32_t)__builtin_amdgcn_readfirstlane((int)T);
        asm volatile("" : "+s"(Ts));
        QS_ROW(real, pos, rs, p, Ts, g); QS_ROW(real, vel, rs, p, Ts, g); QS_ROW(real, rot, rs, p, Ts, g);
        QS_ROW(real, omega, rs, p, Ts, g);
        QS_ROW(real, goal, rs, p, Ts, g); QS_ROW(uint32_t, flags, rs, p, Ts, g);
#pragma unroll
        for (int q = 0; q < 3; ++q) { b_pos.st(d.pos[q], q); b_vel.st(d.vel[q], q); b_omega.st(d.omega[q], q); }
        if (goal_dirty) {
#pragma unroll
            for (int q = 0; q < 3; ++q) b_goal.st(goal[q], q);
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) b_rot.st(d.rot[q], q);
#if !QS_LATE
        {
            QS_ROW(real, rot_damp, rs, p, Ts, g); QS_ROW(real, cmds_damp, rs, p, Ts, g); QS_ROW(real, ou, rs, p, Ts, g);
            QS_ROW(real, ring, rs, p, Ts, g); QS_ROW(real, sums, rs, p, Ts, g);
            QS_ROW(uint64_t, pair, rs, p, Ts, g);
            b_pair.st(out_curr_pair);
#pragma unroll
            for (int q = 0; q < 3; ++q) b_sums.st(sums[q], q);
#pragma unroll
            for (int q = 0; q < 4; ++q) { b_rot_damp.st(d.rot_damp[q], q); b_cmds_damp.st(d.cmds_damp[q], q); b_ou.st(d.ou[q], q);
                b_ring.st(ring[q], q); }
        }
#endif
        b_flags.st(d.flags);
        if (nan_any) atomicOr(p.error_flag, 1u);
#if !QS_LATE
        if (i == 0) {
#pragma unroll
            for (int q = 0; q < QS_CNT_COUNT; ++q) p.counters[q * E + e] = cnt[q];
            p.tick[e] = tick_before;
            p.step_ctr[e] = step_no - 1;
        }
#endif
    }
    QS_STAMP(13);
}


// qs_step_team.inc - "team of waves" variant of the step kernel (see qs_step_kernel.inc for the single-wave one), included
// by qs_step_team_modes.inc once per launch mode (step / rollout / gated), for each QS_SCEN_FULL that qs_step_flavours.inc sets.
//
// One workgroup = 4 wavefronts = the same floor(64/N) environments as the single-wave kernel: lane l of EVERY wave is
// drone l.  Wave 0 owns the drone state in registers and runs the serial physics (sub-steps, reward, collision
// responses, scenario, reset); waves 1-3 take the work that is independent per (drone, partner) or per drone:
//   wave 1      sensor-noise draws (concurrent with wave 0's sub-steps), then the self observation
//   waves 0,2,3 the pair scan (collision / proximity / downwash test), partners striped over the three waves
//   wave 3      obstacle first-hit
//   wave 2      logging outputs: the infos['rewards'] matrix (write_rew_info) and the per-episode sums of the reward-shaping wrapper
//               (episode_sums, reward_shaping.py:78-110) - 25 read-modify-write rows per drone that would otherwise sit at the end of
//               wave 0's critical path (measured: 7.8 -> 11.0 us per C2 step with them there); their loads go out at kernel entry
//   all four    neighbour metrics, rank-by-counting + neighbour-obs rows (partners striped), SDF cells, obs copy-out
// More than 8 drones per environment (BASELINE config 4: 32) - pair once: every UNORDERED pair is evaluated once, by one lane of
// any of the waves (round-robin tournament numbering: pair p -> round p / (N/2), slot p % (N/2); no table, no square root):
// distance, collision / proximity / downwash tests for both directions and the neighbour metric (symmetric in the pair), scattered
// with LDS atomic ORs / two stores into the metric matrix [N][lanes].  Waves 1.. then rank their stripe of every drone's row
// (rank-by-counting in registers, top 8 compacted by local rank) WHILE wave 0 does the bookkeeping and the rare responses; the
// metrics were computed with the velocities before those responses, so an environment in which a velocity changed (rare) redoes
// its rows after barrier 3.  N = 32: 992 pair evaluations per workgroup instead of 2 x 1984 + 2 x 1984 partner evaluations (C4 shard
// 14.66 -> 13.85 us per step: profiles/r03d_bench_lines.txt).
// At BASELINE config 2 (8192 drones = 128 workgroups) the chip is latency-bound on a lone wave per SIMD; spreading a
// drone's independent work over 4 SIMDs of the CU shortens that critical path.  Six LDS-only workgroup barriers per
// control step (QS_TEAM_BARRIER: s_waitcnt lgkmcnt(0) + s_barrier; global memory is not involved in any exchange).
// (Round 6 tried the neighbour / SDF columns of N <= 8 on the helper waves WHILE wave 0 does its bookkeeping between barriers 2 and 3, with a
// redo behind barrier 3 for the rare velocity change: C2 7.43 -> 7.84 us per step, C3 unchanged, with 7 / 6 / 4 / 3 helper waves alike - the
// helpers' LDS traffic and issue slots slow wave 0 down by more than the two barriers save: profiles/r06h_ab_early_rows.txt.  Not kept.)
// ------------------------------------------------------------------------------------------------
#undef e_state_or_e
#if QS_MULTI
#define e_state_or_e e_state
#else
#define e_state_or_e e
#endif
#ifndef QS_GATED
// 1 (with QS_MULTI): the resident-state kernel of qs_step_gated - its own instantiation, so that the open-loop multi-step kernel pays
// nothing for the gate
#define QS_GATED 0
#endif
#ifndef QS_XCHG
#error "QS_XCHG (0 / 1: the one-step body with the fused exchange epilogue) comes from qs_step_team_modes.inc"
#endif
#ifdef QS_SPEC
#if QS_MULTI && QS_GATED
extern "C" __global__ void __launch_bounds__(64 * QS_TW) qs_spec_gated(QS_KARGS, int QS_EPB_ARG, int ksteps) {
#elif QS_MULTI
extern "C" __global__ void __launch_bounds__(64 * QS_TW) qs_spec_rollout(QS_KARGS, int QS_EPB_ARG, int ksteps) {
#else
extern "C" __global__ void __launch_bounds__(64 * QS_TW) qs_spec_step(QS_KARGS, int QS_EPB_ARG) {
    const int t = 0;
#endif
#else
template <typename real>
#if QS_MULTI && QS_GATED && QS_SCEN_FULL
__global__ void __launch_bounds__(64 * QS_TW) qs_gated_team_full(QS_KARGS, int QS_EPB_ARG, int ksteps) {
#elif QS_MULTI && QS_GATED
__global__ void __launch_bounds__(64 * QS_TW) qs_gated_team(QS_KARGS, int QS_EPB_ARG, int ksteps) {
#elif QS_MULTI && QS_SCEN_FULL
__global__ void __launch_bounds__(64 * QS_TW) qs_rollout_team_full(QS_KARGS, int QS_EPB_ARG, int ksteps) {
#elif QS_MULTI
__global__ void __launch_bounds__(64 * QS_TW) qs_rollout_team(QS_KARGS, int QS_EPB_ARG, int ksteps) {
#elif QS_SCEN_FULL
__global__ void __launch_bounds__(64 * QS_TW) qs_step_team_full(QS_KARGS, int QS_EPB_ARG) {
    const int t = 0;
#else
__global__ void __launch_bounds__(64 * QS_TW) qs_step_team(QS_KARGS, int QS_EPB_ARG) {
    const int t = 0;
#endif
#endif
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int W = QS_TW, WS = QS_TW - 1;   // waves per workgroup; waves that take part in the pair scan (all but wave 1)
    QS_SPEC_PROLOGUE
    const Consts<real> *cp = &c;
    // reward coefficients + proximity slope: read from device memory on every launch, so that the reward-shaping wrapper's
    // updates (qs_set_reward_coeffs) also reach launches that were captured into a HIP graph
    real rewc[QS_REW_COUNT + 1];
#pragma unroll
    for (int q = 0; q <= QS_REW_COUNT; ++q) rewc[q] = p.rew_rt[q];
#define QS_OBST_SIZE (c.dr_on ? p.obst_size_env[ee] : c.obst_size)   /* --quads_domain_random: the running episode's obstacle size */
    const int B = QS_WAVE, N = c.num_agents, E = c.num_envs, T = E * N, M_ = c.num_obstacles, K = c.num_neighbors;
    uint64_t *s_mask = (uint64_t *)(smem + L.off_mask);
    uint32_t *s_envflag = (uint32_t *)(smem + L.off_envflag);
    real *s_pos = (real *)(smem + L.off_pos), *s_vel = (real *)(smem + L.off_vel), *s_zax = (real *)(smem + L.off_zax);
    real *s_om = (real *)(smem + L.off_om), *s_goal = (real *)(smem + L.off_goal), *s_obs = (real *)(smem + L.off_obs);
    real *s_obst = (real *)(smem + L.off_obst), *s_metric = (real *)(smem + L.off_metric);
    // team exchange rows: rotation rows 0,1 (row 2 = s_zax... see publish), goal, pair-scan partials, obstacle hit
    real *s_rot6 = (real *)(smem + L.off_t_rot), *s_gpub = (real *)(smem + L.off_t_goal), *s_prox = (real *)(smem + L.off_t_prox);
    uint64_t *s_colm = (uint64_t *)(smem + L.off_t_col), *s_dwm = (uint64_t *)(smem + L.off_t_dw),
        *s_nearm = (uint64_t *)(smem + L.off_t_near);
    int *s_ohit = (int *)(smem + L.off_t_ohit);
    real *s_ri = (real *)(smem + L.off_t_ri);                         // [QS_RI_COUNT + 1][B]: reward terms of this step, then the done flag
    int *s_redo = (int *)(smem + L.off_t_redo);                       // [epb] pair-once: a velocity of this env changed after the pair scan
    unsigned char *s_topk = smem + L.off_topk;                        // [(W-1)*8][B] keys: the ranking waves' compacted top-8 lists
    const bool pair_once = N > 8;                                     // (N is a literal in the config-specialised objects)
#ifndef QS_SN_STASH      // 1: the sensor noise of a step's SECOND observation pass (drawn only when something interacted, by wave 0, on the
#ifdef QS_SPEC           // critical path) is drawn ahead by wave 2 while it waits for barrier 1 and parked in the row's neighbour columns
#define QS_SN_STASH 1    // (config-specialised objects; 0: the generic kernels, A/B and identity switch)
#else
#define QS_SN_STASH 0
#endif
#endif
#ifndef QS_REDO_ROWS     // 1: a changed velocity redoes only the rows / columns of the changed drones (config-specialised objects); 0: the whole
#ifdef QS_SPEC           // environment's metrics (the generic kernels; -DQS_REDO_ROWS=0: A/B and identity switch)
#define QS_REDO_ROWS 1
#else
#define QS_REDO_ROWS 0
#endif
#endif

    QS_POISON_LDS(L.total, 64 * QS_TW);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave id: uniform => scalar branches
    const int tid = threadIdx.x & 63, le = tid / N, i = tid - le * N, e = blockIdx.x * epb + le, base = le * N;
    const bool active = (le < epb) && (e < E);
    const int g = active ? e * N + i : 0, ee = active ? e : 0;
    const uint64_t nmask = (N >= 64) ? ~0ull : ((1ull << N) - 1);
    real *myobs = s_obs + tid * c.obs_dim;
    const __amdgpu_buffer_rsrc_t rs = QS_BUF_RSRC(p);
    QS_ROW(real, pos, rs, p, T, g); QS_ROW(real, vel, rs, p, T, g); QS_ROW(real, rot, rs, p, T, g); QS_ROW(real, omega, rs, p, T, g);
    QS_ROW(real, rot_damp, rs, p, T, g); QS_ROW(real, cmds_damp, rs, p, T, g); QS_ROW(real, ou, rs, p, T, g);
    QS_ROW(real, goal, rs, p, T, g);
    QS_ROW(real, ring, rs, p, T, g); QS_ROW(real, sums, rs, p, T, g); QS_ROW(uint32_t, flags, rs, p, T, g);
    QS_ROW(uint64_t, pair, rs, p, T, g);
    // The per-environment rows (11 counters, tick, noise-stream position, the three collision id sets) through a resource of their own: one scalar
    // row offset + the lane's env offset per access where `p.counters[q * E + e]` costs a 64-bit address chain (v_ashrrev / v_add /
    // v_lshl_add_u64) per row - ~50 instructions in front of the kernel's last stores.  All 16 stores at the tail and the load of the
    // noise-stream position at the head.  One-step body only; -DQS_ENV_ROWS_FLAT=0: the typed pointers again (the same bytes: A/B and
    // identity switch).
#ifndef QS_ENV_ROWS_FLAT
#define QS_ENV_ROWS_FLAT 1
#endif
#undef QS_ENV_ROWS
#define QS_ENV_ROWS (QS_ENV_ROWS_FLAT && !QS_MULTI)
#if QS_ENV_ROWS
    const __amdgpu_buffer_rsrc_t rs_env = QS_ENV_RSRC(p, E);
    QS_ROWE(uint32_t, step_ctr, rs_env, E, ee);   // (the kernel's first load: its address chain sits in front of wave 0's state loads)
#endif

    QS_STAMP(0);
    QS_STAMPW(0);
    QS_STAMP_WG(0);
    // ================= loads (wave 0; coalesced: each array one contiguous span per wave) =================
    Drone<real> d;
    real goal[3], act[4], ring[4], sums[3];
    int32_t cnt[QS_CNT_COUNT];
    uint64_t prev_pair = 0;
    int tick_before = 0, svs_period = 0;
#if QS_SCEN_FULL && defined(QS_SPEC_N)
    ScenRegs<real> sreg;   // this lane's share of the env's scenario state between its load (here) and its LDS write (behind the sub-steps)
#endif
    uint32_t step_no = 0;
    // the noise stream's step counter first: loads return in order, so the two waves that draw noise wait for this one alone.  Only the
    // LOAD sits in front of the state loads; its `+ 1` comes behind their issue (with the add here the compiler closed the branch with
    // `s_waitcnt vmcnt(0)` before wave 0 had issued a single state load: profiles/r05b_oldctr_ab.txt, C2 - 0.20 us).  Loading the counter
    // inside each wave's own branch was measured slower (profiles/r05o_ab_prio.txt); docs/HISTORY.md has the ISA story.
    uint32_t step_raw = 0;
    if (wv <= 1 || (QS_SN_STASH && !QS_MULTI && wv == 2)) {   // (the waves that draw random numbers)
#if QS_ENV_ROWS
        step_raw = b_step_ctr.ld();
#else
        step_raw = p.step_ctr[ee];
#endif
    }
    if (wv == 0) {
        // lane-major blocks (the specialised 8-wave kernels): one 12- / 16-byte access per array and lane, 14 loads in float32
        if (b_pos.wide) {
            b_pos.template ldv<3>(d.pos); b_vel.template ldv<3>(d.vel); b_omega.template ldv<3>(d.omega); b_goal.template ldv<3>(goal);
            b_sums.template ldv<3>(sums);
            b_rot.template ldv<9>(d.rot);
            b_rot_damp.template ldv<4>(d.rot_damp); b_cmds_damp.template ldv<4>(d.cmds_damp); b_ou.template ldv<4>(d.ou);
            b_ring.template ldv<4>(ring);
        } else {            // component rows: one 4-byte access per component, 45 loads
#pragma unroll
            for (int q = 0; q < 3; ++q) { d.pos[q] = b_pos.ld(q); d.vel[q] = b_vel.ld(q); d.omega[q] = b_omega.ld(q);
                goal[q] = b_goal.ld(q); sums[q] = b_sums.ld(q); }
#pragma unroll
            for (int q = 0; q < 9; ++q) d.rot[q] = b_rot.ld(q);
#pragma unroll
            for (int q = 0; q < 4; ++q) { d.rot_damp[q] = b_rot_damp.ld(q); d.cmds_damp[q] = b_cmds_damp.ld(q); d.ou[q] = b_ou.ld(q);
                ring[q] = b_ring.ld(q); }
        }
        d.flags = b_flags.ld();
        prev_pair = b_pair.ld();
        QS_POISON_DRONE(d); QS_POISON_ARR(goal, 3, 16); QS_POISON_ARR(sums, 3, 16); QS_POISON_ARR(ring, 4, 16); QS_POISON_U64(prev_pair);
        tick_before = p.tick[ee];
        svs_period = (c.scenario == QS_SCENARIO_SWARM_VS_SWARM) ? p.scen_int[ee] : 0;
        if (active && i == 0) {
            // (these LOADS and the tick's keep the typed pointer: their address chains hide under the state loads' latency, and
            // tests/test_spec_resources.py pins the number of narrow buffer loads of the 8-wave kernel - one to spare; the stores do not)
#pragma unroll
            for (int q = 0; q < QS_CNT_COUNT; ++q) cnt[q] = p.counters[q * E + ee];
        }
#if QS_SCEN_FULL
#ifdef QS_SPEC_N
        if (active) scen_regs_load<real>(p, E, e, i, sreg);   // -> LDS behind the sub-steps
#else
        if (active) scen_lds_load<real>(p, L, smem, E, e, le, i, N);
#endif
#endif
        asm volatile("" : "+v"(step_raw));   // first use of the counter: HERE, behind the issue of the state loads (s_waitcnt vmcnt(~15))
        step_no = step_raw + 1;
    } else if (wv == 1 || (QS_SN_STASH && !QS_MULTI && wv == 2)) {
        step_no = step_raw + 1;
    }
    if (wv == W - 1 && c.use_obstacles && active) {   // stage the env's obstacle positions in LDS (first read after barrier 1)
        for (int k = i; k < M_; k += N) {
            s_obst[(le * 2 + 0) * M_ + k] = p.obst_pos[(size_t)e * M_ + k];
            s_obst[(le * 2 + 1) * M_ + k] = p.obst_pos[(size_t)E * M_ + (size_t)e * M_ + k];
        }
    }
#if QS_SCEN_FULL
    real *s_sr = (real *)(smem + L.off_sr) + le * SR_COUNT;
    int *s_si = (int *)(smem + L.off_si) + le * SI_COUNT;
#endif
    // wave 2 keeps the running per-episode sums in registers for the whole launch: loaded here (the latency hides under wave 0's
    // sub-steps), updated once per control step behind barrier 3, stored by the last instructions of the wave
    constexpr int WL = 2;
    const bool logw = (wv == WL) && active;
    real rsum[QS_SUM_COUNT];
    if (logw && c.episode_sums) {
#pragma unroll
        for (int q = 0; q < QS_SUM_COUNT; ++q) rsum[q] = p.run_sums[q * T + g];
    }
#if !QS_MULTI && QS_XCHG   // (the `_x` instantiation of the one-step body: qs_step_team_modes.inc)
    // fused exchange: the sequence number and the peers' acknowledgements are fetched here, under the state loads (qs_xchg_fused.h)
    unsigned long long xq_seq = 0, xq_ack = ~0ull;
    if constexpr (sizeof(real) == 4) qsx::fused_prefetch(p.xchg, wv, tid, xq_seq, xq_ack);
#endif
    uint64_t out_curr_pair = 0;
    bool nan_any = false;
#if QS_MULTI
    const int g_state = g, e_state = e;
#if QS_GATED
    // Resident-state stepping (qs_step_gated; qs_xchg_dev.h "Gate", "GateStep"): in this instantiation of the multi-step kernel the exchange
    // slot of Ptrs carries the gate (the fused exchange epilogue exists in the one-step kernels only), and the action-pointer argument the
    // sequence base of the launch (control steps taken by earlier gated launches).  The hand-over area of the action prefetch: the
    // reward-term rows.
    qsx::GateStep<real> gate((qsx::Gate *)p.xchg, (unsigned long long)(uintptr_t)actions, s_ri);
#endif
    for (int t = 0; t < ksteps; ++t) {
    // Opaque copies of the drone / env index: keeps the ~60 output addresses of the loop body from being hoisted out
    // of the loop as live 64-bit pointers (they are recomputed from g / e in each step instead).
    int g = g_state, e = e_state;
    asm volatile("" : "+v"(g), "+v"(e));
#endif
    RngKey key = {c.seed_lo, c.seed_hi, (uint32_t)(c.env_id_offset + ee), step_no};
    SensNoise<real> sn;
    real rew = 0, ri[QS_RI_COUNT];
    bool nan_rew = false, done = false;
    int tick = 0;
    // ================= A. wave 0: per-drone step | wave 1: sensor noise =================
    if (wv == 0) {
#if QS_GATED
        gate.wait_actions(t, g, tid, act);
#else
        {   // actions are row-major [T,4]: one 16/32-byte vector load per lane
            const real *a = actions + ((size_t)t * T + g) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) act[q] = a[q];
        }
#endif
        QS_POISON_ARR(act, 4, 8);
        // new_pair_mask is written on every step by this kernel: mark the word "possibly non-zero" for the kernels that skip zero stores
        // (F_NEWPAIR_NZ, qs_device.h).  Here, under the load latency - the same update next to the store, as a select on the mask, cost the
        // C2 step 0.22 us (profiles/r04j_team_outputs_ab.txt); an auto-reset re-initialises the flags and its word is the zero stored
        // below.
        d.flags |= F_NEWPAIR_NZ;
        real zou[4];
        rng_normal<real, 4>(key, QS_SITE_OU, 0, i, 0, zou);
#if !QS_MULTI
        // the pair-mask word (the LAST state load) is needed after barrier 2; without this the scheduler lifts `~prev_pair` to the top of
        // the block and the wait for it (vmcnt(1): every state load) lands in front of the Philox rounds that are meant to run under the
        // loads
        asm volatile("" : "+v"(prev_pair) : "v"(zou[0]));
#endif
        QS_STAMP(1);
        // RawControl quadrotor_control.py:53-57, OU noise quad_utils.py:275-279, 2 sub-steps (qs_device.h),
        // reward quadrotor_single.py:34-92, tick/done :352-353
        {
            real cmds[4], acc[3];
            control_and_thrust_noise<real>(c, act, zou, d, cmds);
            QS_STAMP(2);
            for (int s = 0; s < c.sim_steps; ++s) substep<real>(c, key, i, s, d, cmds, acc);
            QS_STAMP(3); QS_STAMP_WGK(6);
            // publish what the other waves need: position, velocity, rotation, angular velocity, goal; clear the OR rows
#pragma unroll
            for (int q = 0; q < 3; ++q) { s_pos[q * B + tid] = d.pos[q]; s_vel[q * B + tid] = d.vel[q]; s_om[q * B + tid] = d.omega[q];
                s_gpub[q * B + tid] = goal[q]; }
#pragma unroll
            for (int q = 0; q < 6; ++q) s_rot6[q * B + tid] = d.rot[(q / 2) * 3 + (q & 1)];
            s_zax[0 * B + tid] = d.rot[2]; s_zax[1 * B + tid] = d.rot[5]; s_zax[2 * B + tid] = d.rot[8];
            s_colm[tid] = 0; s_dwm[tid] = 0; s_nearm[tid] = 0;
#if QS_SCEN_FULL && defined(QS_SPEC_N)
#if QS_MULTI
            if (active && t == 0)   // (later steps of the launch continue from the LDS copy)
#else
            if (active)
#endif
                scen_regs_to_lds<real>(L, smem, le, i, sreg);   // read by this wave only (bookkeeping, phase D), two barriers from here
#endif
            main_reward<real>(c, rewc, d, goal, act, rew, ri);
        }
        nan_rew = not_finite(rew);
        tick = tick_before + 1;
        done = tick > c.ep_len;
        QS_STAMP(4);
    } else if (wv == 1) {
#if QS_GATED
        gate.prefetch(t, ksteps, g);   // (the loads' values are used at this step's publish point)
#endif
        // sensor noise of the first observation pass (sensor_noise.py:172-218): state-independent, drawn while wave 0 integrates
        real zou_unused[4];
        if (c.sense_noise) step_noise_draw<real>(c, key, i, zou_unused, sn);
    }
    // state-independent like every draw (Philox keyed by env, step, site, pass, drone): same values whoever draws them, whenever
    // (one step per launch only: in the multi-step kernels another wave may still be copying the previous step's rows out of LDS)
    const bool stash_sn = QS_SN_STASH && !QS_MULTI && W >= 3 && c.sense_noise && c.obs_dim - c.self_dim >= 12;
    if (stash_sn && wv == 2 && active) {
        SensNoise<real> s1;
        sensor_noise_draw<real>(c, key, i, 1, s1);
        real *o = myobs + c.self_dim;   // (free until the neighbour rows are written behind barrier 4)
#pragma unroll
        for (int q = 0; q < 3; ++q) { o[q] = s1.p[q]; o[3 + q] = s1.v[q]; o[6 + q] = s1.w[q]; o[9 + q] = s1.th[q]; }
    }
    QS_STAMPW(1);
    QS_TEAM_BARRIER();   // (1) published state visible
    QS_STAMP(5); QS_STAMP_WGK(7);
    QS_STAMPW(2);

    // ================= B. self obs (wave 1) | pair scan | obstacle first hit (wave 3) =================
    // self observation of wave 1 (get_state.py + sensor_noise.py on the published state)
#define QS_SELF_OBS_W1() do { if (active) { \
            Drone<real> dh; real gh[3]; \
            _Pragma("unroll") for (int q = 0; q < 3; ++q) { dh.pos[q] = s_pos[q * B + tid]; dh.vel[q] = s_vel[q * B + tid]; dh.omega[q] = s_om[q * B + tid]; gh[q] = s_gpub[q * B + tid]; } \
            _Pragma("unroll") for (int q = 0; q < 6; ++q) dh.rot[(q / 2) * 3 + (q & 1)] = s_rot6[q * B + tid]; \
            dh.rot[2] = s_zax[0 * B + tid]; dh.rot[5] = s_zax[1 * B + tid]; dh.rot[8] = s_zax[2 * B + tid]; \
            self_obs<real>(c, sn, dh, gh, myobs); } } while (0)
    const bool ranked = K > 0 && K < N - 1;
    if (pair_once) {
        // ---- every unordered pair of the environment once: lane (wave wv, drone i) takes the pairs p = wv*N + i, + W*N, ... ----
        // Round-robin numbering over MOD = N - 1 + (N & 1) (odd) rounds of PPR = N / 2 pairs: round r, slot k -> {(r + k) % MOD,
        // (r - k) % MOD}, k = 1 .. (MOD - 1) / 2, and for even N slot 0 -> {r, N - 1}.
        if (wv == 1 && c.use_obstacles) QS_SELF_OBS_W1();   // with obstacles the bookkeeping behind barrier 2 reads the noisy self obs
        const int NP = N * (N - 1) / 2, PPR = N / 2, MOD = N - 1 + (N & 1), workers = W * N;
        for (int it = 0; it * 2 * workers < NP; ++it) {   // uniform trip count; two pairs per iteration (their LDS reads fly together)
            const int p0 = wv * N + i + it * 2 * workers;
            int pa[2], pb[2];
            bool valid[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int p = p0 + u * workers;
                valid[u] = active & (p < NP);
                const int pc = (p < NP) ? p : 0, r = pc / PPR, k = pc - r * PPR;
                const int kk = (N & 1) ? k + 1 : k;
                int a = r + kk; a = a >= MOD ? a - MOD : a;
                int b = r - kk; b = b < 0 ? b + MOD : b;
                if (!(N & 1) && kk == 0) { a = r; b = N - 1; }
                pa[u] = a; pb[u] = b;
            }
            real xa[2][3], xb[2][3], va[2][3], vb[2][3], za[2][3], zb[2][3];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    xa[u][q] = s_pos[q * B + base + pa[u]]; xb[u][q] = s_pos[q * B + base + pb[u]];
                    va[u][q] = s_vel[q * B + base + pa[u]]; vb[u][q] = s_vel[q * B + base + pb[u]];
                    za[u][q] = s_zax[q * B + base + pa[u]]; zb[u][q] = s_zax[q * B + base + pb[u]];
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int a = pa[u], b = pb[u];
                // calculate_collision_matrix collisions/quadrotors.py:63-91, proximity :95-103, downwash cylinder test downwash.py:30-45
                const real rel[3] = {xa[u][0] - xb[u][0], xa[u][1] - xb[u][1], xa[u][2] - xb[u][2]};   // a seen from b
                const real dist = M<real>::sqrt(rel[0] * rel[0] + rel[1] * rel[1] + rel[2] * rel[2]);
                const bool hit = valid[u] & (dist <= c.collision_threshold);
                const bool near = valid[u] & (dist <= c.collision_falloff_threshold);
                // b above a?  (a's offset along b's body z)
                const real rz_a = dot3<real>(rel, zb[u]);
                const real nrel[3] = {-rel[0], -rel[1], -rel[2]};
                const real rz_b = dot3<real>(nrel, za[u]);                                          // a above b?
                const bool dw_a = valid[u] & ((real)-0.7 < rz_a) & (rz_a < (real)0) & (M<real>::sqrt(dist * dist - rz_a * rz_a) < (real)0.1);
                const bool dw_b = valid[u] & ((real)-0.7 < rz_b) & (rz_b < (real)0) & (M<real>::sqrt(dist * dist - rz_b * rz_b) < (real)0.1);
                if (__builtin_expect(hit | near | dw_a | dw_b, 0)) {   // rare: OR the partner's bit into both rows
                    const unsigned long long ba = 1ull << a, bb = 1ull << b;
                    if (hit) { atomicOr((unsigned long long *)&s_colm[base + a], bb);
                        atomicOr((unsigned long long *)&s_colm[base + b], ba); }
                    if (near) { atomicOr((unsigned long long *)&s_nearm[base + a], bb);
                        atomicOr((unsigned long long *)&s_nearm[base + b], ba); }
                    if (dw_a) atomicOr((unsigned long long *)&s_dwm[base + a], bb);
                    if (dw_b) atomicOr((unsigned long long *)&s_dwm[base + b], ba);
                }
                if (ranked) {   // neighborhood_indices quadrotor_multi.py:247-274: the metric is the same seen from a and from b
                    const real rv[3] = {vb[u][0] - va[u][0], vb[u][1] - va[u][1], vb[u][2] - va[u][2]};
                    const real m = nbr_metric<real>(nrel, rv);
                    if (valid[u]) { s_metric[b * B + base + a] = m; s_metric[a * B + base + b] = m; }
                }
            }
        }
        // rank-by-counting over the whole row reads the diagonal
        if (ranked && K > 8 && wv == 1 && active) s_metric[i * B + tid] = (real)3.4e38;
        if (wv == W - 1 && active) {
            int obst_idx = -1;
            if (c.use_obstacles) {   // first hit in index order, obstacles/utils.py:31-43
                const real mp[2] = {s_pos[0 * B + tid], s_pos[1 * B + tid]};
                const real *ox = s_obst + (le * 2 + 0) * M_, *oy = s_obst + (le * 2 + 1) * M_;
                for (int k = M_ - 1; k >= 0; --k) {
                    real dx = mp[0] - ox[k], dy = mp[1] - oy[k];
                    obst_idx = (M<real>::sqrt(dx * dx + dy * dy) <= (c.dr_on
                        ? c.arm_r + (real)0.5 * QS_OBST_SIZE : c.obst_hit_threshold)) ? k : obst_idx;
                }
            }
            s_ohit[tid] = obst_idx;
        }
    } else
    if (wv == 1) {
        QS_SELF_OBS_W1();
    } else if (active) {
        // calculate_collision_matrix collisions/quadrotors.py:63-91, proximity penalties :95-103 and the downwash
        // cylinder test of aerodynamics/downwash.py:30-45 share the relative position.  Partners are striped over the
        // three scanning waves; two partners per iteration so their LDS reads are issued together.
        const int lane3 = (wv == 0) ? 0 : wv - 1;   // index among the WS scanning waves
        const real mp[3] = {s_pos[0 * B + tid], s_pos[1 * B + tid], s_pos[2 * B + tid]};
        const real pr = rewc[QS_REW_COUNT];
        uint32_t colm_lo = 0, colm_hi = 0, dwm_lo = 0, dwm_hi = 0;   // 32-bit halves: with N <= 32 a literal the high halves fold away
        real prox = 0;
        for (int j0 = lane3; j0 < N; j0 += 2 * WS) {
            real rel[2][3], zx[2][3];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = (j0 + WS * u < N) ? j0 + WS * u : N - 1;
#pragma unroll
                for (int a = 0; a < 3; ++a) { rel[u][a] = mp[a] - s_pos[a * B + base + j]; zx[u][a] = s_zax[a * B + base + j]; }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {   // branch-free: `&&` on lane-varying conditions compiles to exec-mask branches
                const int j = j0 + WS * u;
                const bool other = (j < N) & (j != i);
                real dist = M<real>::sqrt(rel[u][0] * rel[u][0] + rel[u][1] * rel[u][1] + rel[u][2] * rel[u][2]);
                const uint32_t hit = (uint32_t)(other & (dist <= c.collision_threshold));
                prox += (other & (dist <= c.collision_falloff_threshold)) ? pr * dist + rewc[QS_REW_QUADCOL_SMOOTH_MAX] : (real)0;
                real rz = dot3<real>(rel[u], zx[u]), rxy = M<real>::sqrt(dist * dist - rz * rz);
                const uint32_t dw = (uint32_t)(other & ((real)-0.7 < rz) & (rz < (real)0) & (rxy < (real)0.1));   // drone j is above me
                if (N <= 32 || j < 32) { colm_lo |= hit << (j & 31); dwm_lo |= dw << (j & 31); }
                else { colm_hi |= hit << (j & 31); dwm_hi |= dw << (j & 31); }
            }
        }
        const uint64_t colm = colm_lo | ((uint64_t)colm_hi << 32), dwm = dwm_lo | ((uint64_t)dwm_hi << 32);
        if (colm) atomicOr((unsigned long long *)&s_colm[tid], (unsigned long long)colm);
        if (dwm) atomicOr((unsigned long long *)&s_dwm[tid], (unsigned long long)dwm);
        s_prox[lane3 * B + tid] = prox;
        if (wv == W - 1) {
            int obst_idx = -1;
            if (c.use_obstacles) {   // first hit in index order, obstacles/utils.py:31-43
                const real *ox = s_obst + (le * 2 + 0) * M_, *oy = s_obst + (le * 2 + 1) * M_;
                for (int k = M_ - 1; k >= 0; --k) {
                    real dx = mp[0] - ox[k], dy = mp[1] - oy[k];
                    obst_idx = (M<real>::sqrt(dx * dx + dy * dy) <= (c.dr_on
                        ? c.arm_r + (real)0.5 * QS_OBST_SIZE : c.obst_hit_threshold)) ? k : obst_idx;
                }
            }
            s_ohit[tid] = obst_idx;
        }
    }
    QS_STAMPW(3);
    QS_TEAM_BARRIER();   // (2) pair-scan partials + self obs visible
    QS_STAMP(6); QS_STAMP_WGK(8);
    QS_STAMPW(4);

    uint64_t curr_pair = 0, unique = 0, m_obst_new = 0, m_room = 0, new_pair = 0;
    bool refresh_obs = false;
    int obst_idx = -1;
    real eps_dist[3] = {0, 0, 0};
    if (wv == 0) {
        uint64_t dw_mask = 0;
        bool in_curr = false;
        real prox = 0;
        uint32_t bits = 0;
        if (active) {
            const uint64_t colm = s_colm[tid];
            in_curr = colm != 0;
            curr_pair = (i >= 63) ? 0 : (colm & ~((2ull << i) - 1));   // pairs are stored at the lower id (i < j)
            dw_mask = s_dwm[tid];
            // proximity penalties collisions/quadrotors.py:95-103 over the (rare) partners within the falloff radius, ascending index
            if (pair_once) {
                uint64_t nm = s_nearm[tid];
                while (__builtin_expect(nm != 0, 0)) {
                    const int j = __ffsll((long long)nm) - 1;
                    nm &= nm - 1;
                    const real rel[3] = {d.pos[0] - s_pos[0 * B + base + j], d.pos[1] - s_pos[1 * B + base + j],
                        d.pos[2] - s_pos[2 * B + base + j]};
                    prox += rewc[QS_REW_COUNT] * M<real>::sqrt(rel[0] * rel[0] + rel[1] * rel[1] + rel[2] * rel[2]) + rewc[QS_REW_QUADCOL_SMOOTH_MAX];
                }
            } else {
                prox = s_prox[0 * B + tid];
#pragma unroll
                for (int q = 1; q < WS; ++q) prox += s_prox[q * B + tid];
            }
            if (c.use_obstacles) {
                obst_idx = s_ohit[tid];
                obstacle_hit_bits(obst_idx, d.flags, bits);
            }
            room_collision_bits(d.flags, bits);
        }
        // ---- env-level id sets, collision rewards: qs_step_sem.h (quadrotor_multi.py:432-546) ----
        new_pair = curr_pair & ~prev_pair;                                                 // pair-level novelty (:437-438)
        const EnvEvents ev = env_events<real>(c, active, in_curr, new_pair, bits, d.flags, base, nmask, i, tick, tick_before, myobs);
        unique = ev.unique; m_obst_new = ev.obst_new; m_room = ev.room;
        collision_rewards<real>(c, rewc, ev, i, bits, prox, rew, ri);
        if (c.write_rew_info || c.episode_sums) {   // all 17 terms are final: hand them (and the done flag) to the logging wave
#pragma unroll
            for (int q = 0; q < QS_RI_COUNT; ++q) s_ri[q * B + tid] = ri[q];
            s_ri[QS_RI_COUNT * B + tid] = done ? (real)1 : (real)0;
        }
        // ---- distance-to-goal log, reached_goal, windowed sums for the episode stats; per-env counters (lane 0 keeps them in registers)
        // ----
#if QS_SCEN_FULL
        goal_distance_log<real, false>(c, active ? s_sr[SR_METRIC] : (real)0, tick, done, d.flags, ring, sums, ri, eps_dist);
#else
        goal_distance_log<real, false>(c, c.approach_goal_metric, tick, done, d.flags, ring, sums, ri, eps_dist);
#endif
        if (active && i == 0) env_counters_add<real>(c, cnt, ev);

        QS_STAMP(7); QS_STAMP_WGK(9);
        const real vel_before[3] = {d.vel[0], d.vel[1], d.vel[2]};   // (pair-once: which drones' metric rows are stale behind barrier 3)
        // ================= C. physical interactions, in the reference's order (:548-587) =================
        // (qs_step_sem.h) 1) downwash, 2) drone-drone responses of the new pairs, 3) obstacle, 4) wall then ceiling
        downwash_phase<real>(c, key, d, s_pos, s_zax, B, base, nmask, N, i, active, dw_mask, bits, (int *)nullptr,
            (const double *)nullptr, WaveSync());
        QS_STAMP(8);
        const bool any_dw = ((__ballot(active && (bits & B_DOWNWASH)) >> base) & nmask) != 0;
        // (draw table: the proximity rows of the pair scan, (W - 1) * 64 reals >= QS_DD_CHUNK * QS_DD_DRAWS - read above, rewritten behind the next barrier 1)
        static_assert((W - 1) * QS_WAVE >= QS_DD_CHUNK * QS_DD_DRAWS, "the draw table fits the proximity rows");
#ifdef QS_SERIAL_PAIR_RESPONSES   // the serial form, for same-box A/Bs and tests/test_object_identity_gpu.py
        pair_responses<real>(key, d, ev, new_pair, active, N, i, tid, base, B, s_pos, s_vel, s_om, s_mask, (int *)nullptr, WaveSync());
#else
        pair_responses<real>(key, d, ev, new_pair, active, N, i, tid, base, B, s_pos, s_vel, s_om, s_mask, (int *)nullptr, WaveSync(), s_prox);
#endif
        room_obstacle_phase<real>(cp, key, d, active, N, i, bits, obst_idx, s_obst + (le * 2 + 0) * M_, s_obst + (le * 2 + 1) * M_,
            p.obst_size_env + ee, (int *)nullptr, WaveSync());
        const bool update_flag = any_dw || (ev.newpair_any != 0) || (ev.obst_new != 0) || (ev.wall != 0) || (ev.ceil != 0);

        // ================= D. scenario.step() (qs_step_sem.h; qs_scenarios.h) =================
#if QS_SCEN_FULL
        {
            ScenCtx<real> x = {s_sr, s_si, (uint64_t *)(smem + L.off_omap) + le * 4, s_goal + le * L.goal_rows * 3, s_zax, B, base, N};
            scenario_phase_full<real>(c, key, x, active, N, i, tick, goal, (int *)s_mask + base, (int *)nullptr, WaveSync());
        }
#else
        svs_phase<real>(c, p, key, active, N, E, e, i, tick, svs_period, s_goal + le * L.goal_rows * 3, (int *)s_mask + base, goal,
            (int *)nullptr, WaveSync());
#endif
        QS_STAMP(9); QS_STAMP_WGK(10);
        // ================= E. final observations (:592-607) =================
#pragma unroll
        for (int q = 0; q < 3; ++q) s_vel[q * B + tid] = d.vel[q];
        refresh_obs = update_flag && active;
        if (pair_once) {
            // a velocity of this env changed: its metric rows are redone behind barrier 3
            // ... N <= 32 (QS_REDO_ROWS): bit j = the velocity of drone j changed, only those rows / columns of the metric matrix are redone
            const bool vel_changed = active && (bits_differ(d.vel[0], vel_before[0]) | bits_differ(d.vel[1], vel_before[1]) |
                bits_differ(d.vel[2], vel_before[2]));
            const uint32_t changed = (uint32_t)((__ballot(vel_changed) >> base) & nmask);
            if (active && i == 0) s_redo[le] = QS_REDO_ROWS && N <= 32 ? (int)changed : (update_flag ? 1 : 0);
        } else if (__builtin_expect(refresh_obs, 0)) {   // fresh sensor noise, new goal (:598-599)
            if (c.sense_noise) {
                if (stash_sn) {
                    const real *o = myobs + c.self_dim;
#pragma unroll
                    for (int q = 0; q < 3; ++q) { sn.p[q] = o[q]; sn.v[q] = o[3 + q]; sn.w[q] = o[6 + q]; sn.th[q] = o[9 + q]; }
                } else sensor_noise_draw<real>(c, key, i, 1, sn);
            }
            self_obs<real>(c, sn, d, goal, myobs);
        }
    } else if (pair_once) {
        // ================= waves 1.. while wave 0 does the bookkeeping: self obs, then the local ranking of this wave's candidates
        // =================
        if (wv == 1 && !c.use_obstacles) QS_SELF_OBS_W1();
        if (ranked && K <= 8 && active) team_rank_local<real, W>(N, i, base, B, tid, wv, s_pos, s_vel, s_metric, s_topk, false);
    }
    QS_STAMPW(5);
    QS_TEAM_BARRIER();   // (3) final velocities (and the redo flags) visible
    QS_STAMP(14); QS_STAMP_WGK(11);
    QS_STAMPW(6);
    // neighbour metric of this wave's partners (neighborhood_indices quadrotor_multi.py:247-274)
    real mpos[3] = {0, 0, 0}, mvel[3] = {0, 0, 0};
    if (K > 0 && active) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { mpos[q] = s_pos[q * B + tid]; mvel[q] = s_vel[q * B + tid]; }
    }
    const bool po_big = pair_once && K > 0 && K < N - 1 && K <= 8;
    const bool redo = pair_once && active && s_redo[le] != 0;
    if (QS_REDO_ROWS && N <= 32 && po_big) {   // (before wave 0's fresh-noise self observation: that runs beside the ranking)
        // Only the metrics of pairs with a drone whose velocity changed are stale: changed drone a (bit a of the env's word) -> every other
        // drone i of the env re-evaluates m(i, a) and writes it to both places of the matrix (the changed drones round-robin over the
        // ranking waves; a pair of two changed drones is written twice with the same bits: the metric is symmetric to the bit), then - one more
        // barrier, taken by the whole workgroup only when one of its environments needs it - the ranking waves rank from the matrix again.
        bool wg_redo = false;
        for (int q = 0; q < epb; ++q) wg_redo |= s_redo[q] != 0;   // (uniform: every wave reads the same words)
        if (__builtin_expect(wg_redo, 0)) {
            if (wv >= 1) {
                uint32_t m = active ? (uint32_t)s_redo[le] : 0u;
                for (int idx = 0; __any(m != 0); ++idx) {
                    const int a = m ? __ffs((int)m) - 1 : -1;
                    m &= m - 1;
                    if (a >= 0 && a != i && idx % (W - 1) == wv - 1) {
                        const real rp[3] = {s_pos[0 * B + base + a] - mpos[0], s_pos[1 * B + base + a] - mpos[1], s_pos[2 * B + base + a] - mpos[2]};
                        const real rv[3] = {s_vel[0 * B + base + a] - mvel[0], s_vel[1 * B + base + a] - mvel[1], s_vel[2 * B + base + a] - mvel[2]};
                        const real mm = nbr_metric<real>(rp, rv);
                        s_metric[a * B + tid] = mm; s_metric[i * B + base + a] = mm;
                    }
                }
            }
            QS_TEAM_BARRIER();   // (3b) the stale rows / columns are rewritten
            if (wv >= 1 && redo) team_rank_local<real, W>(N, i, base, B, tid, wv, s_pos, s_vel, s_metric, s_topk, false);
        }
    }
    // fresh sensor noise, new goal (:598-599); wave 1 wrote the row before barrier 3
    if (pair_once && wv == 0 && __builtin_expect(refresh_obs, 0)) {
        if (c.sense_noise) {
            if (stash_sn) {
                const real *o = myobs + c.self_dim;
#pragma unroll
                for (int q = 0; q < 3; ++q) { sn.p[q] = o[q]; sn.v[q] = o[3 + q]; sn.w[q] = o[6 + q]; sn.th[q] = o[9 + q]; }
            } else sensor_noise_draw<real>(c, key, i, 1, sn);
        }
        self_obs<real>(c, sn, d, goal, myobs);
    }
    if (logw && (c.write_rew_info || c.episode_sums)) {
        // infos[i]['rewards'] of this step (quadrotor_single.py:68-85, quadrotor_multi.py:533-540) and, on the device, what the
        // reward-shaping wrapper accumulates from them per episode (reward_shaping.py:78-110): sums of the 17 terms, of the 4 raw actions
        // and of their squares
        real r[QS_RI_COUNT];
#pragma unroll
        for (int q = 0; q < QS_RI_COUNT; ++q) r[q] = s_ri[q * B + tid];
        // the sums of a finished episode include its last step, then restart from zero
        const bool fin = s_ri[QS_RI_COUNT * B + tid] != (real)0;
        if (c.write_rew_info) {
#pragma unroll
            for (int q = 0; q < QS_RI_COUNT; ++q) p.rew_info[q * T + g] = r[q];
        }
        if (c.episode_sums) {
            real a4[4];
#if QS_GATED
            gate.reload_actions(t, g, a4);
#else
            {
                const real *a = actions + ((size_t)t * T + g) * 4;
#pragma unroll
                for (int q = 0; q < 4; ++q) a4[q] = a[q];
            }
#endif
#pragma unroll
            for (int q = 0; q < QS_SUM_COUNT; ++q) {
                const real add = q < QS_RI_COUNT
                    ? r[q < QS_RI_COUNT ? q : 0] : (q < QS_SUM_ACT2
                    ? a4[(q - QS_SUM_ACT) & 3] : a4[(q - QS_SUM_ACT2) & 3] * a4[(q - QS_SUM_ACT2) & 3]);
                const real v = rsum[q] + add;
                if (fin) p.ep_sums[q * T + g] = v;
                rsum[q] = fin ? (real)0 : v;
            }
        }
    }
    // N <= 8: one metric row per drone in LDS, then rank-by-counting over all N (2 candidates per wave).
    // pair-once (N > 8): the metric matrix is already there (pair scan) and, for K <= 8, so are the ranking waves' lists (made while
    //         wave 0 did the bookkeeping); only the environments in which a velocity changed since (s_redo) redo theirs here.
    if (QS_REDO_ROWS && N <= 32 && po_big) {   // (done right behind barrier 3, above)
    } else
    if (po_big && wv >= 1 && __builtin_expect(redo, 0)) team_rank_local<real,
        W>(N, i, base, B, tid, wv, s_pos, s_vel, s_metric, s_topk, true);
    if (ranked && active && !po_big && (!pair_once || redo)) {
        for (int j0 = wv; j0 < N; j0 += 2 * W) {
            real rp[2][3], rv[2][3];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = (j0 + W * u < N) ? j0 + W * u : N - 1;
#pragma unroll
                for (int a = 0; a < 3; ++a) { rp[u][a] = s_pos[a * B + base + j] - mpos[a]; rv[u][a] = s_vel[a * B + base + j] - mvel[a]; }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = j0 + W * u;
                real rd = M<real>::fmax(norm3<real>(rp[u]), (real)0.01);
                real m = rd + (rp[u][0] * rv[u][0] + rp[u][1] * rv[u][1] + rp[u][2] * rv[u][2]) * M<real>::rcp(rd);
                if (j < N) s_metric[j * B + tid] = (j != i) ? m : (real)3.4e38;
            }
        }
    }
    QS_STAMPW(7);
    QS_TEAM_BARRIER();   // (4) metrics visible
    QS_STAMP(15); QS_STAMP_WGK(12);
    QS_STAMPW(8);
    if (po_big && active && wv >= 1) {
        // global rank of this wave's r-th nearest = r + the number of smaller entries in the other ranking waves' lists (their first K
        // entries suffice: an entry that has K smaller ones in one list is not among the K nearest anyway); K <= 8
        constexpr int SL = (W - 1) * 8;
        NbrKey<real> own[8];
        int grank[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { if (r < K) own[r] = NbrKey<real>::ld(s_topk, SL, (wv - 1) * 8 + r, B, tid); grank[r] = r; }
        for (int w2 = 1; w2 < W; ++w2) {
            if (w2 == wv) continue;
            NbrKey<real> ok[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) if (q < K) ok[q] = NbrKey<real>::ld(s_topk, SL, (w2 - 1) * 8 + q, B, tid);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                if (r < K) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) if (q < K) grank[r] += (int)ok[q].less(own[r]);
                }
            }
        }
        real *o = myobs + c.self_dim;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r < K) {
                const int j = own[r].idx();
                if (j < N && grank[r] < K) {   // invalid entries (fewer candidates than slots) carry an index >= 0x7fffff00
                    real *oo = o + grank[r] * 6;
                    real vals[6];
#pragma unroll
                    for (int a = 0; a < 3; ++a) { vals[a] = s_pos[a * B + base + j]; vals[3 + a] = s_vel[a * B + base + j]; }
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        oo[a] = clipr<real>(vals[a] - mpos[a], -c.nbr_clip_pos[a], c.nbr_clip_pos[a]);
                        oo[3 + a] = clipr<real>(vals[3 + a] - mvel[a], -c.nbr_clip_vel[a], c.nbr_clip_vel[a]);
                    }
                }
            }
        }
    }
    if (K > 0 && active && !(ranked && po_big)) {
        // rank by counting = position in the stable ascending argsort; the K lowest go to obs slot `rank` (extend_obs_space :233-245)
        real *o = myobs + c.self_dim;
        for (int j = wv; j < N; j += W) {
            if (j == i) continue;
            int rank = (j < i) ? j : j - 1;   // K == N-1: all others in index order (:253-254)
            if (ranked) {
                const real mj = s_metric[j * B + tid];
                rank = 0;
                for (int k0 = 0; k0 < N; k0 += 8) {
                    real mk[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) mk[u] = s_metric[((k0 + u < N) ? k0 + u : N - 1) * B + tid];
#pragma unroll
                    for (int u = 0; u < 8; ++u) rank += (int)((k0 + u < N) & ((mk[u] < mj) | ((mk[u] == mj) & (k0 + u < j))));
                }
            }
            if (rank < K) {
                real *oo = o + rank * 6;
                real vals[6];   // all six LDS reads before the first LDS write (the compiler must assume they alias)
#pragma unroll
                for (int a = 0; a < 3; ++a) { vals[a] = s_pos[a * B + base + j]; vals[3 + a] = s_vel[a * B + base + j]; }
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    oo[a] = clipr<real>(vals[a] - mpos[a], -c.nbr_clip_pos[a], c.nbr_clip_pos[a]);
                    oo[3 + a] = clipr<real>(vals[3 + a] - mvel[a], -c.nbr_clip_vel[a], c.nbr_clip_vel[a]);
                }
            }
        }
    }
    if (c.use_obstacles && active) {   // get_surround_sdfs obstacles/utils.py:5-27: the 9 cells striped over the waves
        const real *ox = s_obst + (le * 2 + 0) * M_, *oy = s_obst + (le * 2 + 1) * M_;
        const real px = s_pos[0 * B + tid], py = s_pos[1 * B + tid];
        real *o = myobs + c.self_dim + 6 * K;
        for (int q = wv; q < 9; q += W) {
            const int a = q / 3, b = q - a * 3;
            const real gx = px + (real)0.1 * (real)(a - 1), gy = py + (real)0.1 * (real)(b - 1);
            real mind2 = (real)10000;   // min of the squared distances, one square root per cell (sdf_obs, qs_obs_rows.h)
            for (int k = 0; k < M_; ++k) {
                real dx = gx - ox[k], dy = gy - oy[k], d2 = dx * dx + dy * dy;
                mind2 = d2 < mind2 ? d2 : mind2;
            }
            o[q] = M<real>::sqrt(mind2) - (c.dr_on ? (real)0.5 * QS_OBST_SIZE : c.obst_radius);
        }
    }
    QS_STAMPW(9);
    QS_TEAM_BARRIER();   // (5) observation rows complete
    QS_STAMP(10); QS_STAMP_WGK(13);
    QS_STAMPW(10);

    // ================= F. done: episode snapshot + auto-reset (:626-722), wave 0 =================
    uint64_t out_unique = unique, out_obst_new = m_obst_new, out_room = m_room, out_new_pair = new_pair;
    out_curr_pair = curr_pair;
    int out_tick = tick, out_obst_idx = obst_idx;
    if (wv == 0) {
        const bool do_reset = active && done;
        if (__builtin_expect(__ballot(do_reset) != 0, 0)) {
            if (do_reset) {
                p.ep_stats[QS_EPS_DIST_1S * T + g] = eps_dist[0]; p.ep_stats[QS_EPS_DIST_3S * T + g] = eps_dist[1];
                p.ep_stats[QS_EPS_DIST_5S * T + g] = eps_dist[2];
                p.ep_stats[QS_EPS_REACHED_GOAL * T + g] = (d.flags & F_REACHED) ? (real)1 : (real)0;
                p.ep_stats[QS_EPS_COL_AGENT_OK * T + g] = (d.flags & F_COL_AGENT_OK) ? (real)1 : (real)0;
                p.ep_stats[QS_EPS_COL_OBST_OK * T + g] = (d.flags & F_COL_OBST_OK) ? (real)1 : (real)0;
                if (i == 0) {
#pragma unroll
                    for (int q = 0; q < QS_CNT_COUNT; ++q) { p.ep_counters[q * E + e] = cnt[q]; cnt[q] = 0; }
                }
            }
            real stale_vel[3] = {d.vel[0], d.vel[1], d.vel[2]};
            QS_WAVE_SYNC();
            if (do_reset && i == 0) p.ep_scenario[e] = QS_SCEN_FULL ? ((int *)(smem + L.off_si))[le * SI_COUNT + SI_SCEN] : c.scenario;
            reset_body<real, (QS_SCEN_FULL != 0), true>(cp, &p, &L, smem, epb, key, do_reset, &d, goal, stale_vel);
            if (do_reset) {
                out_unique = 0; out_obst_new = 0; out_room = 0; out_curr_pair = 0; out_new_pair = 0; out_tick = 0; out_obst_idx = -1;
                ring[0] = ring[1] = ring[2] = ring[3] = 0;
                if (c.scenario == QS_SCENARIO_SWARM_VS_SWARM) svs_period = (int)s_envflag[epb + le];   // new U(4,6) s period
            }
        }
    }
    QS_STAMP(11); QS_STAMP_WGK(14);
    QS_STAMPW(11);
    QS_TEAM_BARRIER();   // (6) rows of re-initialised envs rewritten
    QS_STAMPW(12);
    // ================= G. per-step outputs =================
    {   // obs copy-out by all four waves: the workgroup's rows form one contiguous [rows*obs_dim] block in LDS and in HBM
        const int D = c.obs_dim, first_env = blockIdx.x * epb;
        int nenv = E - first_env; nenv = nenv < epb ? nenv : epb;
        const int total = nenv * N * D;
        real *dst = p.obs + (size_t)first_env * N * D;
#if QS_GATED
        qsx::obs_copy_out_sc1<real, W>(dst, s_obs, total, (size_t)first_env * N * D);
#else
        if ((total & 3) == 0 && ((((size_t)first_env * N * D) * sizeof(real)) & 15) == 0 && sizeof(real) == 4) {
            const qs_f32x4 *src4 = (const qs_f32x4 *)s_obs;
            for (int idx = threadIdx.x; idx < total / 4; idx += 64 * W) obs_st4((float *)dst + 4 * idx, src4[idx]);
        } else {
            for (int idx = threadIdx.x; idx < total; idx += 64 * W) obs_st1<real>(dst + idx, s_obs[idx]);
        }
#endif
#if !QS_MULTI && QS_XCHG
        // the same rows, in the wire type, into every rank's receive window; the q8 wire stages in the (by now dead) reward-term rows
        if constexpr (sizeof(real) == 4) qsx::fused_push<W>(p.xchg, xq_seq, xq_ack, wv, tid, first_env, nenv, N, D, K, c.self_dim,
            (const float *)s_obs, (unsigned int *)s_ri, (int)(sizeof(real) * (QS_RI_COUNT + 1) * B));
#endif
    }
    QS_STAMP(12); QS_STAMP_WGK(15);
    QS_STAMPW(13);
#if QS_GATED
    // the same outputs, written through the L2, then published: done_flag[workgroup] = sequence number
    gate.publish(t, wv, tid, active, i == 0, p.new_pair_mask + g, out_new_pair, p.obst_hit_idx + g, c.use_obstacles, out_obst_idx,
        p.reward + g, rew, p.done + g, done, p.unique_col + e, out_unique, p.obst_new + e, out_obst_new, p.room_new + e, out_room);
#else
    if (wv == 0 && active) {
        {   // lane offsets from this step's (opaque) g: see the note at the top of the loop
            QS_ROWF(uint64_t, newpair, rs, p, T, g); QS_ROWF(int32_t, ohit, rs, p, T, g); QS_ROWF(real, reward, rs, p, T, g);
            QS_ROWF(uint8_t, done, rs, p, T, g);
            // obst_hit_idx keeps the reset's -1 without obstacles
            b_newpair.st(out_new_pair);   // always stored here (F_NEWPAIR_NZ is raised at the top of the step: see there)
            if (c.use_obstacles) b_ohit.st(out_obst_idx);
            b_reward.st(rew); b_done.st(done ? 1 : 0);
        }
#if !QS_ENV_ROWS   // (else: with the other per-environment rows, behind the state stores)
        if (i == 0) { p.unique_col[e] = out_unique; p.obst_new[e] = out_obst_new; p.room_new[e] = out_room; }
#endif
    }
#endif
    nan_any |= nan_rew;
    // loop-carried values of the next control step
    prev_pair = out_curr_pair;
    tick_before = out_tick;
    step_no += 1;
#if QS_MULTI
    }   // for t  (no extra barrier: every wave finishes its copy-out before it reaches barrier (1) of the next step)
#endif

    if (logw && c.episode_sums) {
#if QS_MULTI
        const int g = g_state;
#endif
#pragma unroll
        for (int q = 0; q < QS_SUM_COUNT; ++q) p.run_sums[q * T + g] = rsum[q];
    }
    // ================= H. state stores (nothing waits on them: they are the last instructions of the wave) =================
    if (wv == 0) {
#if QS_SCEN_FULL
        QS_WAVE_SYNC();
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
            QS_ROW(real, rot_damp, rs, p, Ts, g); QS_ROW(real, cmds_damp, rs, p, Ts, g); QS_ROW(real, ou, rs, p, Ts, g);
            QS_ROW(real, goal, rs, p, Ts, g);
            QS_ROW(real, ring, rs, p, Ts, g); QS_ROW(real, sums, rs, p, Ts, g); QS_ROW(uint32_t, flags, rs, p, Ts, g);
            QS_ROW(uint64_t, pair, rs, p, Ts, g);
            if (b_pos.wide) {   // lane-major: 12- / 16-byte pieces (ldv / stv, qs_state_rows.h)
                b_vel.template stv<3>(d.vel); b_omega.template stv<3>(d.omega);
                b_pos.template stv<3>(d.pos); b_rot.template stv<9>(d.rot);
                b_rot_damp.template stv<4>(d.rot_damp); b_cmds_damp.template stv<4>(d.cmds_damp); b_ou.template stv<4>(d.ou);
            } else {
#pragma unroll
                for (int q = 0; q < 3; ++q) { b_vel.st(d.vel[q], q); b_omega.st(d.omega[q], q); }
#pragma unroll
                for (int q = 0; q < 3; ++q) b_pos.st(d.pos[q], q);
#pragma unroll
                for (int q = 0; q < 9; ++q) b_rot.st(d.rot[q], q);
#pragma unroll
                for (int q = 0; q < 4; ++q) { b_rot_damp.st(d.rot_damp[q], q); b_cmds_damp.st(d.cmds_damp[q], q); b_ou.st(d.ou[q], q); }
            }
            b_flags.st(d.flags);
            b_goal.template stv<3>(goal);
            b_sums.template stv<3>(sums);
            b_ring.template stv<4>(ring);
            b_pair.st(out_curr_pair);
            if (nan_any) atomicOr(p.error_flag, 1u);
            if (i == 0) {
#if QS_ENV_ROWS
                // every per-environment row of the step in ONE lane-0 branch behind the state stores, row offsets recomputed like theirs
                uint32_t Es = (uint32_t)__builtin_amdgcn_readfirstlane((int)E);
                asm volatile("" : "+s"(Es));
                QS_ROWE(uint64_t, unique, rs_env, Es, e); QS_ROWE(uint64_t, obst_new, rs_env, Es, e); QS_ROWE(uint64_t, room_new, rs_env, Es, e);
                QS_ROWE(int32_t, counters, rs_env, Es, e); QS_ROWE(int32_t, tick, rs_env, Es, e); QS_ROWE(uint32_t, step_ctr, rs_env, Es, e);
                b_unique.st(out_unique); b_obst_new.st(out_obst_new); b_room_new.st(out_room);
#pragma unroll
                for (int q = 0; q < QS_CNT_COUNT; ++q) b_counters.st(cnt[q], q);
                b_tick.st(tick_before);
                b_step_ctr.st(step_no - 1);
#else
#pragma unroll
                for (int q = 0; q < QS_CNT_COUNT; ++q) p.counters[q * E + e] = cnt[q];
                p.tick[e] = tick_before;
                p.step_ctr[e] = step_no - 1;
#endif
            }
        }
    }
    QS_STAMP(13);
    QS_STAMP_WG(1);
}


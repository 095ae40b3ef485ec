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
// More than 8 drones per environment (BASELINE config 4: 32) - QS_PAIR_ONCE: every UNORDERED pair is evaluated once, by one lane of
// any of the waves (round-robin tournament numbering: pair p -> round p / (N/2), slot p % (N/2); no table, no square root):
// distance, collision / proximity / downwash tests for both directions and the neighbour metric (symmetric in the pair), scattered
// with LDS atomic ORs / two stores into the metric matrix [N][lanes].  Waves 1.. then rank their stripe of every drone's row
// (rank-by-counting in registers, top 8 compacted by local rank) WHILE wave 0 does the bookkeeping and the rare responses; the
// metrics were computed with the velocities before those responses, so an environment in which a velocity changed (rare) redoes
// its rows after barrier 3.  N = 32: 992 pair evaluations per workgroup instead of 2 x 1984 + 2 x 1984 partner evaluations.
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
#ifndef QS_PAIR_ONCE
#define QS_PAIR_ONCE 1   // C4 shard 14.66 -> 13.85 us per step (profiles/r03d_bench_lines.txt); 0 = the round-2 striped scan
#endif
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
    const bool pair_once = QS_PAIR_ONCE && N > 8;                     // (N is a literal in the config-specialised objects)
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
    // fused exchange: the sequence number and the peers' acknowledgements are fetched here, under the state loads (both are uncached
    // system-scope loads: ~2 us each if they sat in front of the epilogue)
    unsigned long long xq_seq = 0, xq_ack = ~0ull;
    if constexpr (sizeof(real) == 4) {
        if (p.xchg != nullptr) {
            // (+ 1 at its use in the epilogue: an add in this branch would close it with s_waitcnt vmcnt(0), behind the 45 state loads)
            xq_seq = p.xchg->loc->push_seq;
            if (wv == 0 && tid < p.xchg->world) xq_ack = qsx::ld_sys(&p.xchg->mine->ack[tid]);
        }
    }
#endif
    uint64_t out_curr_pair = 0;
    bool nan_any = false;
#if QS_MULTI
    const int g_state = g, e_state = e;
#if QS_GATED
    // Resident-state stepping (qs_step_gated; qs_xchg_dev.h "Gate"): in this instantiation of the multi-step kernel the exchange slot of
    // Ptrs carries the gate (the fused exchange epilogue exists in the one-step kernels only), and the action-pointer argument the sequence
    // base of the launch (control steps taken by earlier gated launches).
    qsx::Gate *const G = (qsx::Gate *)p.xchg;
    const unsigned long long gseq0 = (unsigned long long)(uintptr_t)actions;
    bool gate_dead = false;
    // Action prefetch (wave 1, idle after its noise draws): when the producer is seen to be at least two steps ahead, the NEXT step's
    // action rows are fetched during the current step and handed to wave 0 through LDS, so that a producer that runs ahead costs the
    // stepper no uncached round trip in front of its sub-steps.  Ordering: the flag is read in step t - 1, its value is consumed in step t,
    // and only then is the load of step t + 1's rows issued - a dependent load, never ahead of the flag that vouches for it.  A closed-loop
    // producer is never two steps ahead: nothing is prefetched and wave 0 takes the polling path.
    // [1] sequence number of the rows staged below (0 = none)
    unsigned long long *s_pre_seq = (unsigned long long *)s_ri;
    // [B][4 or 8] words: action rows of that step (the reward-term
    unsigned int *s_actpre = (unsigned int *)((char *)s_ri + 16);
                                                                                   // rows are dead between wave 2's read and wave 0's next
                                                                                   // write)
    unsigned long long pf_flag = 0, pf_flag_next = 0;
    if (threadIdx.x == 0) *s_pre_seq = 0;
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
#if QS_GATED
    bool pf_hold_issue = false;
    unsigned int pf_hold[sizeof(real)] = {};   // 4 (f32) / 8 (f64) words of the next step's action row, wave 1 only
#endif
    // ================= A. wave 0: per-drone step | wave 1: sensor noise =================
    if (wv == 0) {
#if QS_GATED
        {   // wait (bounded) until this workgroup's actions of sequence number gseq0 + t + 1 are in the ring, then read them past the L2
            const unsigned long long seq = gseq0 + (unsigned long long)t + 1;
            if (*s_pre_seq == seq) {   // staged by wave 1 during the previous step (behind that step's publish barrier)
                if constexpr (sizeof(real) == 4) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) act[q] = __uint_as_float(s_actpre[tid * 4 + q]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) act[q] = __longlong_as_double(((long long)s_actpre[tid * 8 + 2 * q + 1] << 32) | s_actpre[tid * 8 + 2 * q]);
                }
            } else {
            if (!gate_dead && !qsx::poll_ge_agent(&G->act_flag[blockIdx.x / G->wg_per_group], seq, G->timeout_ticks)) {
                gate_dead = true;   // a missing producer is reported once; the launch then runs on without waiting (no hung GPU)
                if (tid == 0) atomicOr(&G->status, 1u);
            }
            const char *a = G->act_ring + ((seq - 1) % G->ring_len) * G->act_stride + (size_t)g * 4 * sizeof(real);
            if constexpr (sizeof(real) == 4) {
                const qsx::u32x4_t v = qsx::ld16_sc1(a);
                act[0] = __uint_as_float(v.x); act[1] = __uint_as_float(v.y); act[2] = __uint_as_float(v.z); act[3] = __uint_as_float(v.w);
            } else {
                const qsx::u32x4_t v0 = qsx::ld16_sc1(a), v1 = qsx::ld16_sc1(a + 16);
                act[0] = __longlong_as_double(((long long)v0.y << 32) | v0.x);
                act[1] = __longlong_as_double(((long long)v0.w << 32) | v0.z);
                act[2] = __longlong_as_double(((long long)v1.y << 32) | v1.x);
                act[3] = __longlong_as_double(((long long)v1.w << 32) | v1.z);
            }
            }
        }
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
        // (relaxed system-scope atomic loads: compiler-tracked, asynchronous - their values are used at this step's publish point)
        const unsigned long long seq_w1 = gseq0 + (unsigned long long)t + 1;
        // the producer was seen two steps ahead: rows of step seq + 1 are in the ring
        const bool pf_issue = (t + 1 < ksteps) && (pf_flag >= seq_w1 + 1);
        unsigned int pf_w[2 * sizeof(real)] = {};
        if (pf_issue) {
            const unsigned int *a = (const unsigned int *)(G->act_ring + (seq_w1 % G->ring_len) * G->act_stride + (size_t)g * 4 * sizeof(real));
#pragma unroll
            for (int q = 0; q < (int)(2 * sizeof(real)) / 2; ++q) pf_w[q] = __hip_atomic_load(a + q, __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_SYSTEM);
        }
        pf_flag_next = __hip_atomic_load(&G->act_flag[blockIdx.x / G->wg_per_group], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
        // sensor noise of the first observation pass (sensor_noise.py:172-218): state-independent, drawn while wave 0 integrates
        real zou_unused[4];
        if (c.sense_noise) step_noise_draw<real>(c, key, i, zou_unused, sn);
#if QS_GATED
        // hand-over words (consumed behind this step's publish barrier by wave 0 at the top of the next step; the region is written here at
        // once? no - it is the reward-term area, live until wave 2 has read it behind barrier 3: the values wait in registers until the
        // publish point)
        pf_hold_issue = pf_issue;
#pragma unroll
        for (int q = 0; q < (int)(2 * sizeof(real)) / 2; ++q) pf_hold[q] = pf_w[q];
#endif
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
            {   // (in the ring since wave 0 passed its gate, two barriers ago)
                const char *a = G->act_ring + ((gseq0 + (unsigned long long)t) % G->ring_len) * G->act_stride + (size_t)g * 4 * sizeof(real);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if constexpr (sizeof(real) == 4) a4[q] = __uint_as_float(qsx::ld4_sc1(a + 4 * q));
                    else a4[q] = __longlong_as_double(((long long)qsx::ld4_sc1(a + 8 * q + 4) << 32) | qsx::ld4_sc1(a + 8 * q));
                }
            }
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
    // N  > 8: every wave keeps the sorted top-8 (metric, index) of its own candidates (insertion network in registers),
    //         publishes that list, and the global rank of an entry is its local rank plus the number of smaller entries in
    //         the other three lists - N-independent after the streaming pass (rank-by-counting would cost N*N/4 per wave).
    //         Only valid while K <= 8 (one wave may own more than 8 of the K nearest otherwise): K > 8 ranks by counting.
    // pair-once (N > 8): the metric matrix is already there (pair scan) and, for K <= 8, so are the ranking waves' lists (made while
    //         wave 0 did the bookkeeping); only the environments in which a velocity changed since (s_redo) redo theirs here.
#ifdef QS_EXP_NOBIG   // experiment: rank by counting over all N also for N > 8 (pays off when a wave owns few candidates)
    const bool big = false;
#else
    const bool big = !pair_once && N > 8 && K <= 8;
#endif
    real bm[8];
    int bi[8];
    int *s_mlist_i = (int *)(s_metric + W * 8 * B);   // [W waves][8 slots][B] metrics, then the same shape of indices
    if (QS_REDO_ROWS && N <= 32 && po_big) {   // (done right behind barrier 3, above)
    } else
    if (po_big && wv >= 1 && __builtin_expect(redo, 0)) team_rank_local<real,
        W>(N, i, base, B, tid, wv, s_pos, s_vel, s_metric, s_topk, true);
    if (ranked && active && !big && !po_big && (!pair_once || redo)) {
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
    if (ranked && active && big) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { bm[k] = (real)3.4e38; bi[k] = 0x7fffffff; }
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
                const bool valid = (j < N) & (j != i);
                m = valid ? m : (real)3.4e38;
                int mi = valid ? j : 0x7fffffff;
                // candidates arrive in ascending index order, so inserting behind equal metrics keeps the lower index first
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
        if constexpr (sizeof(real) == 4) {
            // fp32: (metric, index) packed into one order-preserving 64-bit key, so "smaller metric, lower index first" is a single
            // unsigned compare in the merge below
            unsigned long long *s_keys = (unsigned long long *)s_metric;
#pragma unroll
            for (int k = 0; k < 8; ++k) s_keys[(wv * 8 + k) * B + tid] = nbr_key((float)bm[k], bi[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) { s_metric[(wv * 8 + k) * B + tid] = bm[k]; s_mlist_i[(wv * 8 + k) * B + tid] = bi[k]; }
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
    if (K > 0 && active && !(ranked && (big || po_big))) {
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
    if (ranked && big && active) {
        real *o = myobs + c.self_dim;
        int grank[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) grank[k] = k;
        if constexpr (sizeof(real) == 4) {
            const unsigned long long *s_keys = (const unsigned long long *)s_metric;
            unsigned long long mk[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) mk[k] = nbr_key((float)bm[k], bi[k]);
            for (int w2 = 0; w2 < W; ++w2) {   // the other waves' lists, one LDS round trip each
                if (w2 == wv) continue;
                unsigned long long ok[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) ok[q] = s_keys[(w2 * 8 + q) * B + tid];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (k < K) {   // an entry below local rank K cannot be among the K nearest
#pragma unroll
                        for (int q = 0; q < 8; ++q) grank[k] += (int)(ok[q] < mk[k]);
                    }
                }
            }
        } else {
            for (int w2 = 0; w2 < W; ++w2) {   // the other waves' lists, one LDS round trip each
                if (w2 == wv) continue;
                real om[8];
                int oi[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) { om[q] = s_metric[(w2 * 8 + q) * B + tid]; oi[q] = s_mlist_i[(w2 * 8 + q) * B + tid]; }
#pragma unroll
                for (int k = 0; k < 8; ++k)
#pragma unroll
                    for (int q = 0; q < 8; ++q) grank[k] += (int)((om[q] < bm[k]) | ((om[q] == bm[k]) & (oi[q] < bi[k])));
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < K && bi[k] < N && grank[k] < K) {   // slots beyond this wave's candidates hold index 0x7fffffff
                const int j = bi[k];
                real *oo = o + grank[k] * 6;
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
        {   // resident-state stepping: the rows are read by kernels that run concurrently (other XCDs): written through the L2
            if ((total & 3) == 0 && ((((size_t)first_env * N * D) * sizeof(real)) & 15) == 0 && sizeof(real) == 4) {
                const qsx::u32x4_t *src4 = (const qsx::u32x4_t *)s_obs;
                for (int idx = threadIdx.x; idx < total / 4; idx += 64 * W) qsx::st16_sc1((float *)dst + 4 * idx, src4[idx]);
            } else if constexpr (sizeof(real) == 4) {
                for (int idx = threadIdx.x; idx < total; idx += 64 * W) qsx::st4_sc1(dst + idx, __float_as_uint((float)s_obs[idx]));
            } else {
                for (int idx = threadIdx.x; idx < total; idx += 64 * W) qsx::st8_sc1(dst + idx,
                    (unsigned long long)__double_as_longlong((double)s_obs[idx]));
            }
        }
#else
        if ((total & 3) == 0 && ((((size_t)first_env * N * D) * sizeof(real)) & 15) == 0 && sizeof(real) == 4) {
            const qs_f32x4 *src4 = (const qs_f32x4 *)s_obs;
            for (int idx = threadIdx.x; idx < total / 4; idx += 64 * W) obs_st4((float *)dst + 4 * idx, src4[idx]);
        } else {
            for (int idx = threadIdx.x; idx < total; idx += 64 * W) obs_st1<real>(dst + idx, s_obs[idx]);
        }
#endif
#if !QS_MULTI && QS_XCHG
        // ---- fused observation exchange (qs_set_obs_exchange, include/quadswarm_exchange.h): the same rows, in the wire type, into slot
        // [seq & 1][rank] of EVERY rank's receive window - peer stores over the point-to-point links straight from this workgroup's LDS
        // stage, no extra launch.  Flow control and completion flags as in qs_xchg_push_kernel (qs_exchange.hip). ----
        if constexpr (sizeof(real) == 4) {
            if (p.xchg != nullptr) {
                const qsx::XchgDev &X = *p.xchg;
                const unsigned long long seq = xq_seq + 1;            // (push_seq is advanced by the last workgroup of a launch only)
                const int slot = (int)(seq & 1);
                if (wv == 0) {   // every destination must have released what this slot held before (seq - 2)
                    bool ok = true;
                    if (tid < X.world && seq > 2 && xq_ack < seq - 2) ok = qsx::poll_ge(&X.mine->ack[tid], seq - 2, X.timeout_ticks);
                    if (__any(!ok) && tid == 0) atomicOr(&X.loc->status, (unsigned int)QS_XCHG_ERR_ACK_TIMEOUT);
                }
                __syncthreads();
                const size_t row0 = (size_t)first_env * N * D, wsz = X.wire == QS_WIRE_BF16 ? 2 : 4;
                const size_t off = X.wire == QS_WIRE_Q8 ? (size_t)slot * (size_t)X.slot_bytes + ((size_t)X.rank * (size_t)(X.n / D) + (size_t)first_env * N) * (size_t)X.q8.row_words * 4
                                                        : (size_t)slot * (size_t)X.slot_bytes + ((size_t)X.rank * (size_t)X.n + row0) * wsz;
                const float *src = (const float *)s_obs;
                const bool vec = ((total & 7) == 0) && ((off & 15) == 0);   // (the windows themselves are 256-byte aligned)
#ifndef QS_NO_Q8_FUSED   // (A/B switch: the step kernel without the q8 branch of its exchange epilogue)
                // the narrow row: bf16 self / SDF columns + 8-bit fixed-point neighbour block (quadswarm_exchange.h)
                if (X.wire == QS_WIRE_Q8) {
                    // The layout is rebuilt from the kernel's own constants (literals in a config-specialised object: the row / word index
                    // arithmetic folds into multiplications by constants; qs_set_obs_exchange checks that the endpoint was created with
                    // this layout) and the six scales are copied into registers: the stores below are `asm volatile` with a memory clobber,
                    // so every field read through the descriptor pointer inside the loop would be a fresh load from device memory (a first
                    // version did that and divided by a run-time row length: + 14.6 us per C4 step at world size 1 where bf16 costs + 3.8).
                    const int q0 = c.self_dim, q1 = c.self_dim + 6 * K, w16 = (D - 6 * K + 1) >> 1;
                    const float s0 = X.q8.s0, s1 = X.q8.s1, s2 = X.q8.s2, s3 = X.q8.s3, s4 = X.q8.s4, s5 = X.q8.s5;
                    const int rw = w16 + ((6 * K + 3) >> 2), words = nenv * N * rw;
                    // Two phases where the wire block fits the (by now dead) reward-term rows of LDS: every lane converts consecutive words
                    // into a staged copy of the block - no volatile store in that loop, so its LDS reads and the arithmetic of several
                    // words overlap - then the block leaves like the bf16 rows do, one 16-byte LDS read + one 16-byte store per lane and
                    // destination.
                    unsigned int *s_wire = (unsigned int *)s_ri;
                    if ((off & 15) == 0 && (words & 3) == 0 && words * 4 <= (int)(sizeof(real) * (QS_RI_COUNT + 1) * B)) {
                        // (two uniform loops - the bf16 words of every row, then the int8 words - instead of one over all words: in a mixed
                        // loop the lanes of a wave diverge between the two word kinds and every iteration pays for both)
                        const int rows_here = nenv * N, n8w = rw - w16;
                        for (int k = threadIdx.x; k < rows_here * w16; k += 64 * W) {
                            const int r = k / w16, j = k - r * w16;
                            s_wire[r * rw + j] = qsx::q8_row_word_v(src + r * D, D, q0, q1, w16, s0, s1, s2, s3, s4, s5, j);
                        }
                        for (int k = threadIdx.x; k < rows_here * n8w; k += 64 * W) {
                            const int r = k / n8w, j = w16 + (k - r * n8w);
                            s_wire[r * rw + j] = qsx::q8_row_word_v(src + r * D, D, q0, q1, w16, s0, s1, s2, s3, s4, s5, j);
                        }
                        QS_TEAM_BARRIER();
                        for (int idx = threadIdx.x; idx < (words >> 2); idx += 64 * W) {
                            const qsx::u32x4_t ov = *(const qsx::u32x4_t *)(s_wire + 4 * idx);
                            for (int dd = 0; dd < X.world; ++dd) qsx::st16_wt(X.data_win[dd] + off + (size_t)idx * 16, ov);
                        }
                    // 16 bytes per lane and iteration: the volatile stores serialise the iterations, so few, fat ones
                    } else if ((off & 15) == 0 && (words & 3) == 0) {
                        for (int idx = threadIdx.x; idx < (words >> 2); idx += 64 * W) {
                            const int w0 = 4 * idx, r0 = w0 / rw;
                            int r = r0, j = w0 - r0 * rw;
                            unsigned int o[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                o[u] = qsx::q8_row_word_v(src + r * D, D, q0, q1, w16, s0, s1, s2, s3, s4, s5, j);
                                if (++j == rw) { j = 0; ++r; }
                            }
                            const qsx::u32x4_t ov = {o[0], o[1], o[2], o[3]};
                            for (int dd = 0; dd < X.world; ++dd) qsx::st16_wt(X.data_win[dd] + off + (size_t)idx * 16, ov);
                        }
                    } else {
#pragma unroll 1
                        for (int w = threadIdx.x; w < words; w += 64 * W) {   // consecutive lanes = consecutive words of the wire block
                            const int r = w / rw;
                            const unsigned int o = qsx::q8_row_word_v(src + r * D, D, q0, q1, w16, s0, s1, s2, s3, s4, s5, w - r * rw);
                            for (int dd = 0; dd < X.world; ++dd) qsx::st4_wt(X.data_win[dd] + off + (size_t)w * 4, o);
                        }
                    }
                } else
#endif
                if (X.wire == QS_WIRE_BF16) {
                    if (vec) {
                        for (int idx = threadIdx.x; idx < (total >> 3); idx += 64 * W) {
                            const qs_f32x4 a = *(const qs_f32x4 *)(src + 8 * idx), b = *(const qs_f32x4 *)(src + 8 * idx + 4);
                            qsx::u32x4_t o;
                            o.x = qsx::f32_to_bf16_rne(a[0]) | (qsx::f32_to_bf16_rne(a[1]) << 16);
                            o.y = qsx::f32_to_bf16_rne(a[2]) | (qsx::f32_to_bf16_rne(a[3]) << 16);
                            o.z = qsx::f32_to_bf16_rne(b[0]) | (qsx::f32_to_bf16_rne(b[1]) << 16);
                            o.w = qsx::f32_to_bf16_rne(b[2]) | (qsx::f32_to_bf16_rne(b[3]) << 16);
                            for (int dd = 0; dd < X.world; ++dd) qsx::st16_wt(X.data_win[dd] + off + (size_t)idx * 16, o);
                        }
                    } else {
                        for (int idx = threadIdx.x; idx < total; idx += 64 * W) {
                            const unsigned int o = qsx::f32_to_bf16_rne(src[idx]);
                            for (int dd = 0; dd < X.world; ++dd) qsx::st2_wt(X.data_win[dd] + off + (size_t)idx * 2, o);
                        }
                    }
                } else {
                    if (vec) {
                        for (int idx = threadIdx.x; idx < (total >> 2); idx += 64 * W) {
                            const qs_f32x4 a = *(const qs_f32x4 *)(src + 4 * idx);
                            const qsx::u32x4_t o = {__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]),
                                __float_as_uint(a[3])};
                            for (int dd = 0; dd < X.world; ++dd) qsx::st16_wt(X.data_win[dd] + off + (size_t)idx * 16, o);
                        }
                    } else {
                        for (int idx = threadIdx.x; idx < total; idx += 64 * W)
                            for (int dd = 0; dd < X.world; ++dd) qsx::st4_wt(X.data_win[dd] + off + (size_t)idx * 4,
                                __float_as_uint(src[idx]));
                    }
                }
                qsx::wt_drain();          // this thread's (write-through) rows have reached their windows ...
                __syncthreads();
                if (threadIdx.x == 0) {
                    // fenced protocol: EVERY workgroup writes its XCD's L2 back before it takes its ticket
                    qsx::fence_release_sys(X.fenced);
                    const unsigned int tk = atomicAdd(&X.loc->ticket_all, 1u);
                    if (tk == X.blocks - 1) {   // ... and this is the last workgroup of the launch: raise the flags
                        X.loc->ticket_all = 0;
                        for (int dd = 0; dd < X.world; ++dd) qsx::st_sys(&X.flag_win[dd]->arrive[slot][X.rank], seq);
                        X.loc->push_seq = seq;
                        if (X.auto_ack) {   // no in-place reader: wait for the rows of every OTHER rank, then hand the slot back
                            bool ok = true;
                            for (int r = 0; r < X.world; ++r) if (r != X.rank) ok &= qsx::poll_ge(&X.mine->arrive[slot][r], seq,
                                X.timeout_ticks);
                            if (!ok) atomicOr(&X.loc->status, (unsigned int)QS_XCHG_ERR_ARRIVE_TIMEOUT);
                            qsx::fence_acquire_sys(X.fenced);
                            for (int dd = 0; dd < X.world; ++dd) qsx::st_sys(&X.flag_win[dd]->ack[X.rank], seq);
                            X.loc->wait_seq = seq; X.loc->release_seq = seq;
                        }
                    }
                }
            }
        }
#endif
    }
    QS_STAMP(12); QS_STAMP_WGK(15);
    QS_STAMPW(13);
#if QS_GATED
    {   // the same outputs, written through the L2 (agent scope), then published: done_flag[workgroup] = sequence number
        if (wv == 0 && active) {
            qsx::st8_sc1(p.new_pair_mask + g, out_new_pair);
            if (c.use_obstacles) qsx::st4_sc1(p.obst_hit_idx + g, (unsigned int)out_obst_idx);
            if constexpr (sizeof(real) == 4) qsx::st4_sc1(p.reward + g, __float_as_uint((float)rew));
            else qsx::st8_sc1(p.reward + g, (unsigned long long)__double_as_longlong((double)rew));
            qsx::st1_sc1(p.done + g, done ? 1u : 0u);
            if (i == 0) { qsx::st8_sc1(p.unique_col + e, out_unique); qsx::st8_sc1(p.obst_new + e, out_obst_new);
                qsx::st8_sc1(p.room_new + e, out_room); }
        }
        if (wv == 1) {   // stage the prefetched rows of the next step (or say that there are none)
            if (pf_hold_issue) {
#pragma unroll
                for (int q = 0; q < (int)sizeof(real); ++q) s_actpre[tid * (int)sizeof(real) + q] = pf_hold[q];
            }
            if (tid == 0) *s_pre_seq = pf_hold_issue ? gseq0 + (unsigned long long)t + 2 : 0ull;
            pf_flag = pf_flag_next;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's rows and outputs have left the L2 ...
        QS_TEAM_BARRIER();                                   // ... and so have those of the other waves
        if (threadIdx.x == 0) qsx::st_agent(&G->done_flag[blockIdx.x], gseq0 + (unsigned long long)t + 1);
    }
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


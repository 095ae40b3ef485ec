// qs_snapshot_replay.inc - part of quadswarm_hip.hip (one translation unit; needs its handle, dalloc, fail / HIP_TRY and the gate's join).
extern "C" {

// ---- environment snapshots: device-side deep copies of single environments (replay wrapper, SURVEY 8f rank 3) ----
int qs_snapshot_pool(qs_handle *h, int32_t slots) {
    if (!h || slots < 0) return fail(QS_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    if (h->snap_pool) { (void)hipFree(h->snap_pool); h->snap_pool = nullptr; h->snap_slots = 0; }
    if (slots == 0) return QS_OK;
    HIP_TRY(hipMalloc((void **)&h->snap_pool, h->snap_bytes * (size_t)slots));
    h->snap_slots = slots;
    return QS_OK;
}

static int snapshot_io(qs_handle *h, int32_t env, int32_t slot, bool save, hipStream_t s) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    if (env < 0 || env >= h->cfg.num_envs) return fail(QS_ERR_INVALID, "env out of range");
    if (slot < 0 || slot >= h->snap_slots) return fail(QS_ERR_INVALID, "snapshot slot out of range (qs_snapshot_pool first)");
    HIP_TRY(hipSetDevice(h->device));
    if (h->gate_pending) { if (int jr = gate_join_stream(h, s)) return jr; }
    char *dst = h->snap_pool + h->snap_bytes * (size_t)slot;
    for (const auto &a : h->snap_arrays) {
        const size_t gb = a.group ? (size_t)env / a.group : 0, ge = a.group ? (size_t)env - gb * a.group : (size_t)env;
        char *src = a.base + gb * a.group_stride + a.elem * a.per_env * ge;
        const size_t width = a.elem * a.per_env, spitch = a.elem * a.comp_stride;
        if (save) HIP_TRY(hipMemcpy2DAsync(dst, width, src, spitch, width, a.comps, hipMemcpyDeviceToDevice, s));
        else HIP_TRY(hipMemcpy2DAsync(src, spitch, dst, width, width, a.comps, hipMemcpyDeviceToDevice, s));
        dst += (a.elem * a.comps * a.per_env + 15) & ~(size_t)15;
    }
    return QS_OK;
}
int qs_snapshot_save(qs_handle *h, int32_t env, int32_t slot, void *stream) { return snapshot_io(h, env, slot, true, (hipStream_t)stream); }
int qs_snapshot_load(qs_handle *h, int32_t slot, int32_t env, void *stream) { return snapshot_io(h, env, slot, false, (hipStream_t)stream); }
int qs_snapshot_copy(qs_handle *h, int32_t src_slot, int32_t dst_slot, void *stream) {
    if (!h || src_slot < 0 || dst_slot < 0 || src_slot >= h->snap_slots || dst_slot >= h->snap_slots)
        return fail(QS_ERR_INVALID, "snapshot slot out of range");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(h->snap_pool + h->snap_bytes * (size_t)dst_slot, h->snap_pool + h->snap_bytes * (size_t)src_slot, h->snap_bytes,
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return QS_OK;
}

/* Batched experience replay on the device: see include/quadswarm.h. */
int qs_replay_enable(qs_handle *h, double sample_prob) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    if (h->replay_on) return fail(QS_ERR_INVALID, "replay is already enabled on this handle");
    if (h->obs_target)
        return fail(QS_ERR_UNSUPPORTED, "qs_replay_enable: the replay wrapper restores observations into qs_buffers.obs (reset qs_set_obs_target first)");
    if (!h->cfg.episode_sums)
        return fail(QS_ERR_INVALID, "qs_replay_enable needs a handle created with episode_sums = 1 (per-episode crash reward)");
    if (!(sample_prob >= 0.0 && sample_prob <= 1.0)) return fail(QS_ERR_INVALID, "sample_prob must be in [0, 1]");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    ReplayParams &P = h->rp;
    memset(&P, 0, sizeof P);
    const size_t E = h->cfg.num_envs;
    uint32_t off = 0;
    for (const auto &a : h->snap_arrays) {
        if (a.kind == 2) continue;   // the reward-shaping wrapper sits outside the replay wrapper: its sums restart with the episode
        if (P.narr == QS_REPLAY_MAX_ARR) return fail(QS_ERR_UNSUPPORTED, "too many snapshot arrays");
        if (a.kind == 1) P.obs_arr = P.narr;
        if (a.base == (char *)h->pf.tick) P.tick_arr = P.narr;
        P.arr[P.narr++] = {a.base, (uint32_t)a.elem, (uint32_t)a.comps, (uint32_t)a.per_env, off, (uint64_t)a.comp_stride,
                           (uint32_t)a.group, (uint32_t)a.group_stride};
        off += (uint32_t)((a.elem * a.comps * a.per_env + 15) & ~(size_t)15);
    }
    P.snap_bytes = off;
    const double control_freq = 1.0 / (h->cfg.dt * h->cfg.sim_steps);
    P.N = h->cfg.num_agents; P.E = h->cfg.num_envs; P.use_obstacles = h->cfg.use_obstacles;
    P.ep_len = h->cfg.ep_len;
    P.cp_every = (int)(0.5 * control_freq + 0.5);        // cp_step_size_freq (:18-19)
    P.grace_ticks = (int)(1.5 * control_freq + 0.5);     // collisions_grace_period_seconds * control_freq (:150)
    P.min_gap = (int)(5.0 * control_freq + 0.5);         // :152
    P.seed_lo = (uint32_t)(h->cfg.seed & 0xffffffffu); P.seed_hi = (uint32_t)(h->cfg.seed >> 32);
    P.env_id_offset = h->cfg.env_id_offset;
    P.sample_prob = (float)sample_prob;
    P.done = h->pf.done; P.tick = h->pf.tick; P.step_ctr = h->pf.step_ctr; P.unique_col = h->pf.unique_col; P.obst_new = h->pf.obst_new;
    P.counters = h->pf.counters; P.ep_sums = h->pf.ep_sums; P.run_sums = h->pf.run_sums; P.real_size = h->real_size;
    P.T = (int32_t)(E * h->cfg.num_agents);
    int rc;
    if ((rc = dalloc(h, &P.pool, (size_t)P.snap_bytes * (QS_REPLAY_RING + QS_REPLAY_EVENTS) * E)) != QS_OK) return rc;
    if ((rc = dalloc(h, &P.active, E)) != QS_OK || (rc = dalloc(h, &P.saved, E)) != QS_OK || (rc = dalloc(h, &P.ep_saved, E)) != QS_OK ||
        (rc = dalloc(h, &P.crash_hist, 100 * E)) != QS_OK || (rc = dalloc(h, &P.crash_n, E)) != QS_OK ||
        (rc = dalloc(h, &P.crash_pos, E)) != QS_OK || (rc = dalloc(h, &P.ck_count, E)) != QS_OK ||
        (rc = dalloc(h, &P.ck_head, E)) != QS_OK || (rc = dalloc(h, &P.last_added, E)) != QS_OK || (rc = dalloc(h, &P.ev_len, E)) != QS_OK ||
        (rc = dalloc(h, &P.ev_idx, E)) != QS_OK || (rc = dalloc(h, &P.ev_replayed, QS_REPLAY_EVENTS * E)) != QS_OK ||
        (rc = dalloc(h, &P.ev_slot, QS_REPLAY_EVENTS * E)) != QS_OK || (rc = dalloc(h, &P.episodes, E)) != QS_OK ||
        (rc = dalloc(h, &P.replayed, E)) != QS_OK || (rc = dalloc(h, &P.errors, E)) != QS_OK || (rc = dalloc(h, &P.start_tick, E)) != QS_OK ||
        (rc = dalloc(h, &P.last_steps, E)) != QS_OK) return rc;
    {   // the reset() that starts the first episode records crashes_last_episode = 0 (quadrotor_multi.py:356-359); last_added = -1e9
        std::vector<int32_t> ones(E, 1), neg(E, -1000000000);
        HIP_TRY(hipMemcpy(P.crash_n, ones.data(), E * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(P.crash_pos, ones.data(), E * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(P.last_added, neg.data(), E * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    h->replay_on = true;
    return QS_OK;
}

int qs_replay_stats(qs_handle *h, int32_t *out) {
    if (!h || !out) return fail(QS_ERR_INVALID, "null argument");
    if (!h->replay_on) return fail(QS_ERR_INVALID, "replay is not enabled");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t E = h->cfg.num_envs;
    const ReplayParams &P = h->rp;
    std::vector<int32_t> len(E), rep(QS_REPLAY_EVENTS * E);
    std::vector<uint8_t> act(E), eps(E);
    HIP_TRY(hipMemcpy(eps.data(), P.ep_saved, E, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out + 0 * E, P.episodes, E * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out + 1 * E, P.replayed, E * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(len.data(), P.ev_len, E * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rep.data(), P.ev_replayed, QS_REPLAY_EVENTS * E * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(act.data(), P.active, E, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out + 5 * E, P.ck_count, E * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out + 6 * E, P.errors, E * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out + 8 * E, P.last_steps, E * 4, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < E; ++e) {
        int32_t sum = 0;
        for (int q = 0; q < len[e]; ++q) sum += rep[(size_t)q * E + e];
        out[2 * E + e] = len[e]; out[3 * E + e] = sum; out[4 * E + e] = act[e]; out[7 * E + e] = eps[e];
    }
    return QS_OK;
}

int qs_replay_set_active(qs_handle *h, const uint8_t *active_host) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    if (!h->replay_on) return fail(QS_ERR_INVALID, "replay is not enabled");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t E = h->cfg.num_envs;
    std::vector<uint8_t> v(E, 1);
    if (active_host) for (size_t e = 0; e < E; ++e) v[e] = active_host[e] ? 1 : 0;
    HIP_TRY(hipMemcpy(h->rp.active, v.data(), E, hipMemcpyHostToDevice));
    return QS_OK;
}

}  // extern "C"

// qs_env_debug.inc - part of quadswarm_hip.hip (one translation unit; needs its handle, handle_layout and fail / HIP_TRY): single-
// environment state I/O, array copies, the noise tape (test instrument), debug read-outs and per-launch profiling.
extern "C" {

static int state_io(qs_handle *h, int32_t env, double *host, int32_t *tick, int set) {
    if (!h || !host) return fail(QS_ERR_INVALID, "null argument");
    if (env < 0 || env >= h->cfg.num_envs) return fail(QS_ERR_INVALID, "env out of range");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const int N = h->cfg.num_agents;
    const size_t bytes = sizeof(double) * N * QS_STATE_STRIDE;
    int32_t t = tick ? *tick : -1;
    if (set) {
        HIP_TRY(hipMemcpy(h->d_state_buf, host, bytes, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->d_tick_io, &t, sizeof t, hipMemcpyHostToDevice));
    }
    if (h->real_size == 8) {
        Ptrs<double> p; memcpy(&p, &h->pf, sizeof p);
        hipLaunchKernelGGL(qs_state_kernel<double>, dim3(1), dim3(QS_WAVE), 0, 0, p, h->cfg.num_envs, N, env, h->d_state_buf,
                           h->d_tick_io, set);
    } else {
        hipLaunchKernelGGL(qs_state_kernel<float>, dim3(1), dim3(QS_WAVE), 0, 0, h->pf, h->cfg.num_envs, N, env, h->d_state_buf,
                           h->d_tick_io, set);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (!set) {
        HIP_TRY(hipMemcpy(host, h->d_state_buf, bytes, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&t, h->d_tick_io, sizeof t, hipMemcpyDeviceToHost));
        if (tick) *tick = t;
    }
    return QS_OK;
}

int qs_get_state(qs_handle *h, int32_t env, double *state_host, int32_t *tick) { return state_io(h, env, state_host, tick, 0); }
int qs_set_state(qs_handle *h, int32_t env, const double *state_host, int32_t tick) {
    int32_t t = tick;
    return state_io(h, env, (double *)state_host, &t, 1);
}

int qs_memcpy_d2h(qs_handle *h, void *host_dst, const void *dev_src, size_t bytes) {
    if (!h || !host_dst || !dev_src) return fail(QS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return QS_OK;
}

int qs_memcpy_h2d(qs_handle *h, void *dev_dst, const void *host_src, size_t bytes) {
    if (!h || !dev_dst || !host_src) return fail(QS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return QS_OK;
}

int qs_state_array_copy(qs_handle *h, void *host, void *dev_array, int32_t elem, int32_t comps, int32_t to_device) {
    if (!h || !host || !dev_array || elem < 1 || comps < 1) return fail(QS_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t E = h->cfg.num_envs, N = h->cfg.num_agents, T = E * N, epb = h->bufs.envs_per_block, pitch = h->bufs.state_block_bytes;
    if (!h->bufs.state_lane_major) {   // rows of 64 elements per component: one strided copy per component
        const size_t full = E / epb, rem = E - full * epb;   // whole blocks, environments of the last partial one
        for (int32_t c = 0; c < comps; ++c) {
            char *dev = (char *)dev_array + (size_t)c * 64 * elem, *hst = (char *)host + (size_t)c * T * elem;
            const size_t width = epb * N * elem;
            if (full) {
                if (to_device) HIP_TRY(hipMemcpy2D(dev, pitch, hst, width, width, full, hipMemcpyHostToDevice));
                else HIP_TRY(hipMemcpy2D(hst, width, dev, pitch, width, full, hipMemcpyDeviceToHost));
            }
            if (rem) {
                if (to_device) HIP_TRY(hipMemcpy(dev + full * pitch, hst + full * width, rem * N * elem, hipMemcpyHostToDevice));
                else HIP_TRY(hipMemcpy(hst + full * width, dev + full * pitch, rem * N * elem, hipMemcpyDeviceToHost));
            }
        }
        return QS_OK;
    }
    // lane-major: per block 64 lanes x comps adjacent components (lane = local env * N + drone); host: [comps][E * N].  Through a staging
    // copy of the blocks' pieces of this array (a debugging / test path: one strided copy and a transposition on the host)
    const size_t nblk = (E + epb - 1) / epb, lanes = epb * N, width = lanes * comps * elem;
    std::vector<char> stage(nblk * width);
    if (!to_device || E % epb)   // (a partial last block: keep what its idle lanes hold)
        HIP_TRY(hipMemcpy2D(stage.data(), width, dev_array, pitch, width, nblk, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < nblk; ++b)
        for (size_t l = 0; l < lanes && b * lanes + l < T; ++l)
            for (int32_t c = 0; c < comps; ++c) {
                char *st = stage.data() + b * width + (l * comps + c) * elem, *hs = (char *)host + ((size_t)c * T + b * lanes + l) * elem;
                if (to_device) memcpy(st, hs, elem); else memcpy(hs, st, elem);
            }
    if (to_device) HIP_TRY(hipMemcpy2D(dev_array, pitch, stage.data(), width, width, nblk, hipMemcpyHostToDevice));
    return QS_OK;
}

/* Noise tape (test instrument): see include/quadswarm.h. */
int qs_set_noise_tape(qs_handle *h, const double *tape_host, int64_t len_per_env) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    if (h->d_tape) { (void)hipFree(h->d_tape); h->d_tape = nullptr; }
    if (h->d_tape_pos) { (void)hipFree(h->d_tape_pos); h->d_tape_pos = nullptr; }
    h->tape_len = 0;
    h->pf.tape = nullptr; h->pf.tape_pos = nullptr; h->pf.tape_len = 0;
    if (!tape_host || len_per_env <= 0) return QS_OK;   // back to the counter-based stream
    if (len_per_env > 0x7fffff00ll) return fail(QS_ERR_INVALID, "tape too long");
    if (qs_tape_lds_bytes(&h->cfg, h->obs_dim, h->full ? 1 : 0, h->real_size) > 160 * 1024)
        return fail(QS_ERR_UNSUPPORTED, "noise tape: the single-wave layout does not fit the LDS");
    const size_t E = h->cfg.num_envs, bytes = E * (size_t)len_per_env * sizeof(double);
    HIP_TRY(hipMalloc((void **)&h->d_tape, bytes));
    HIP_TRY(hipMalloc((void **)&h->d_tape_pos, E * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(h->d_tape, tape_host, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(h->d_tape_pos, 0, E * sizeof(int32_t)));
    h->tape_len = len_per_env;
    h->pf.tape = h->d_tape; h->pf.tape_pos = h->d_tape_pos; h->pf.tape_len = len_per_env;
    return QS_OK;
}

int qs_set_tape_pos(qs_handle *h, const int32_t *pos_host) {
    if (!h || !pos_host) return fail(QS_ERR_INVALID, "null argument");
    if (!h->d_tape) return fail(QS_ERR_INVALID, "no noise tape set");
    for (int e = 0; e < h->cfg.num_envs; ++e)
        if (pos_host[e] < 0 || pos_host[e] > h->tape_len) return fail(QS_ERR_INVALID, "tape position out of range");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->d_tape_pos, pos_host, (size_t)h->cfg.num_envs * sizeof(int32_t), hipMemcpyHostToDevice));
    return QS_OK;
}

int qs_get_tape_pos(qs_handle *h, int32_t *pos_host) {
    if (!h || !pos_host) return fail(QS_ERR_INVALID, "null argument");
    if (!h->d_tape) return fail(QS_ERR_INVALID, "no noise tape set");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(pos_host, h->d_tape_pos, (size_t)h->cfg.num_envs * sizeof(int32_t), hipMemcpyDeviceToHost));
    return QS_OK;
}

/* debug / tools: dynamic LDS bytes per workgroup of the layout qs_create would use (team: waves per workgroup, 0 = single-wave;
 * spec: 1 = config-specialised kernels) */
int qs_debug_lds_bytes(const qs_config *cfg, int team, int spec) {
    if (!cfg) return -1;
    return handle_layout(cfg, team, spec != 0).total;
}

// QS_TIMING builds (all zero otherwise): [blocks][16]: start, end (s_memtime), HW_ID, XCC_ID, start, end (100 MHz wall clock), then
// s_memtime at 10 phase boundaries of wave 0 of every workgroup
int qs_debug_wg_times(qs_handle *h, unsigned long long *out, int32_t max_blocks) {
    if (!h || !out) return fail(QS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    const int n = h->blocks < max_blocks ? h->blocks : max_blocks;
    HIP_TRY(hipMemcpy(out, h->pf.timing + 128, (size_t)n * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return n;
}
int qs_debug_timing(qs_handle *h, unsigned long long *out128) {   // [4 waves][32 stamps] of workgroup 0 (QS_TIMING builds)
    if (!h || !out128) return fail(QS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out128, h->pf.timing, 128 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return QS_OK;
}

int qs_set_profiling(qs_handle *h, int32_t enable) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    h->profiling = enable != 0;
    h->events_used = 0;
    return QS_OK;
}

int qs_get_kernel_time(qs_handle *h, double *avg_ms, int64_t *launches) {
    if (!h || !avg_ms || !launches) return fail(QS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    double total = 0;
    for (size_t k = 0; k < h->events_used; ++k) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->events[k].first, h->events[k].second));
        total += ms;
    }
    *launches = (int64_t)h->events_used;
    *avg_ms = h->events_used ? total / (double)h->events_used : 0.0;
    h->events_used = 0;
    return QS_OK;
}

}  // extern "C"

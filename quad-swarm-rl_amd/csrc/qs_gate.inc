// qs_gate.inc - part of quadswarm_hip.hip (one translation unit; needs its handle, fail / HIP_TRY and launch_step).
// ------------------------------------------------------------------------------------------------
// Resident-state stepping (include/quadswarm.h)
// ------------------------------------------------------------------------------------------------
extern "C" {

// A gated launch (qs_step_gated) runs on the library's own stream and nothing waits for it by itself: every other entry point that touches
// the handle's device state first joins it - stream-ordered where the call takes a stream, on the host where it copies synchronously.
static int gate_join_stream(qs_handle *h, hipStream_t s) {
    if (h->gate_pending) { HIP_TRY(hipStreamWaitEvent(s, h->gate_ev_out, 0)); }
    return QS_OK;
}
static int gate_join_host(qs_handle *h) {
    if (h->gate_pending) { HIP_TRY(hipStreamSynchronize(h->gate_stream)); h->gate_pending = false; }
    return QS_OK;
}

// the benchmark's / the tests' producer: per control step it (closed_loop: waits until the outputs of the previous step of ITS workgroups
// are published, else: only until the ring slot is free), copies the group's share of the next action batch from a table resident in HBM
// into the ring - written through the L2 - and raises the group's sequence word
// `sums` (qs_gate_produce_verify, closed loop only): the kernel is also a CONSUMER of the stepper's outputs the way the protocol describes
// one - having seen done_flag >= s for its workgroups it executes an agent-scope acquire and reads the observation rows and rewards of step
// s with plain loads - and records a checksum (the sum of their 32-bit words) per step and group, WHILE the gated launch is resident and
// working on step s + 1.  tests/test_gated_gpu.py compares the sums with those of a one-launch-per-step twin.
__global__ void __launch_bounds__(256) qs_gate_producer_kernel(qsx::Gate *G, const char *src, unsigned int n_src,
                                                                unsigned long long seq0, int k, int closed_loop,
                                                                unsigned long long wg_bytes, unsigned long long batch_bytes,
                                                                unsigned long long *sums, const unsigned int *obs_words,
                                                                const unsigned int *rew_words,
                                                                unsigned long long obs_words_per_wg, unsigned long long rew_words_per_wg,
                                                                unsigned long long obs_words_total, unsigned long long rew_words_total) {
    const unsigned int grp = blockIdx.x, w0 = grp * G->wg_per_group,
                       w1 = (w0 + G->wg_per_group < G->blocks) ? w0 + G->wg_per_group : G->blocks;
    const unsigned long long lo = (unsigned long long)w0 * wg_bytes, hi0 = (unsigned long long)w1 * wg_bytes,
                             hi = hi0 < batch_bytes ? hi0 : batch_bytes;
    __shared__ int dead;
    __shared__ unsigned long long acc;
    if (threadIdx.x == 0) dead = 0;
    __syncthreads();
    for (int t = 0; t <= k; ++t) {
        const unsigned long long seq = seq0 + (unsigned long long)t + 1;
        if (t == k && sums == nullptr) break;   // (the extra round only reads the last step's outputs)
        const unsigned long long need = (closed_loop || t == k) ? seq - 1 : (seq > G->ring_len ? seq - G->ring_len : 0);
        if (need > 0 && !dead) {   // every workgroup of the group, 256 at a time (a group may hold all ~512 workgroups of a team handle)
            for (unsigned int w = w0 + threadIdx.x; w < w1; w += 256)
                if (!qsx::poll_ge_agent(&G->done_flag[w], need, G->timeout_ticks)) { dead = 1; atomicOr(&G->status, 2u); break; }
        }
        __syncthreads();
        // the outputs of sequence number seq - 1 (a step of THIS call), read the way a policy would read them
        if (sums != nullptr && t >= 1) {
            if (threadIdx.x == 0) acc = 0;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // buffer_inv sc1: this XCD's L2 may hold the rows of the step before
            __syncthreads();
            unsigned long long part = 0;
            const unsigned long long o0 = (unsigned long long)w0 * obs_words_per_wg, o1u = (unsigned long long)w1 * obs_words_per_wg,
                o1 = o1u < obs_words_total ? o1u : obs_words_total;
            for (unsigned long long j = o0 + threadIdx.x; j < o1; j += 256) part += obs_words[j];
            const unsigned long long r0 = (unsigned long long)w0 * rew_words_per_wg, r1u = (unsigned long long)w1 * rew_words_per_wg,
                r1 = r1u < rew_words_total ? r1u : rew_words_total;
            for (unsigned long long j = r0 + threadIdx.x; j < r1; j += 256) part += rew_words[j];
            atomicAdd(&acc, part);
            __syncthreads();
            if (threadIdx.x == 0) sums[(unsigned long long)(t - 1) * G->groups + grp] = acc;
            __syncthreads();
        }
        if (t == k) break;
        const char *from = src + ((seq - 1) % n_src) * batch_bytes;
        char *to = G->act_ring + ((seq - 1) % G->ring_len) * G->act_stride;
        // system-scope write-through: the flag below must not become visible before the batch (`sc1` alone was seen to let it: one run in
        // three of the run-ahead parity test read a stale batch)
        for (unsigned long long off = lo + 16ull * threadIdx.x; off < hi; off += 16ull * 256)
            qsx::st16_wt(to + off, *(const qsx::u32x4_t *)(from + off));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) qsx::st_agent(&G->act_flag[grp], seq);
    }
}

int qs_gate_create(qs_handle *h, int32_t ring_len, int32_t wg_per_group) {
    if (!h || ring_len < 1 || ring_len > 65536 || wg_per_group < 1) return fail(QS_ERR_INVALID, "qs_gate_create: bad argument");
    if (h->d_gate) return fail(QS_ERR_INVALID, "qs_gate_create: the handle has a gate already");
    if (!h->team) return fail(QS_ERR_UNSUPPORTED, kGatedNeedsTeam);
    if (h->replay_on || h->d_tape)
        return fail(QS_ERR_UNSUPPORTED, "resident-state stepping is not available with the device-side replay wrapper or a noise tape");
    HIP_TRY(hipSetDevice(h->device));
    const size_t T = (size_t)h->cfg.num_envs * h->cfg.num_agents, stride = (T * 4 * (size_t)h->real_size + 255) & ~(size_t)255;
    const unsigned int groups = (unsigned int)((h->blocks + wg_per_group - 1) / wg_per_group);
    const size_t o_ring = 256, o_act = o_ring + stride * (size_t)ring_len, o_done = o_act + (((size_t)groups * 8 + 255) & ~(size_t)255),
        total = o_done + (((size_t)h->blocks * 8 + 255) & ~(size_t)255);
    // Fine-grained (uncached) device memory: the ring and the sequence words are handed between kernels that run CONCURRENTLY, mostly on
    // different XCDs, whose L2s are not coherent with each other - an `sc1` load that hits a stale line of its own XCD's L2 is how a first
    // version of this took 7.8 ms per closed-loop step (profiles/r04c_bench_c2_default.json); uncached memory has no such line
    char *base = nullptr;
    if (hipExtMallocWithFlags((void **)&base, total, hipDeviceMallocUncached) != hipSuccess) {
        (void)hipGetLastError();
        return fail(QS_ERR_HIP, "qs_gate_create: fine-grained (uncached) device memory is not available: resident-state stepping needs it for its action ring and sequence words");
    }
    HIP_TRY(hipMemset(base, 0, total));
    qsx::Gate g;
    memset(&g, 0, sizeof g);
    int khz = 100000;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) {
        (void)hipGetLastError();
        khz = 100000;
    }
    long ms = 500;
    if (const char *ev = getenv("QS_GATE_TIMEOUT_MS")) { const long v = atol(ev); if (v > 0) ms = v; }
    g.timeout_ticks = (unsigned long long)khz * (unsigned long long)ms;
    g.act_ring = base + o_ring; g.act_stride = stride; g.ring_len = (unsigned int)ring_len; g.groups = groups;
    g.wg_per_group = (unsigned int)wg_per_group; g.blocks = (unsigned int)h->blocks;
    g.act_flag = (unsigned long long *)(base + o_act); g.done_flag = (unsigned long long *)(base + o_done);
    HIP_TRY(hipMemcpy(base, &g, sizeof g, hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    {
        int least = 0, greatest = 0;
        hipError_t er = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (er == hipSuccess && !h->gate_stream) er = hipStreamCreateWithPriority(&h->gate_stream, hipStreamNonBlocking, greatest);
        if (er == hipSuccess && !h->gate_ev_in) er = hipEventCreateWithFlags(&h->gate_ev_in, hipEventDisableTiming);
        if (er == hipSuccess && !h->gate_ev_out) er = hipEventCreateWithFlags(&h->gate_ev_out, hipEventDisableTiming);
        if (er != hipSuccess) { (void)hipFree(base); return fail(QS_ERR_HIP, std::string("qs_gate_create: ") + hipGetErrorString(er)); }
    }
    h->d_gate = (qsx::Gate *)base; h->gate_host = g; h->gate_step_seq = 0; h->gate_prod_seq = 0;
    return QS_OK;
}

int qs_gate_info(qs_handle *h, qs_gate_info_t *out) {
    if (!h || !out) return fail(QS_ERR_INVALID, "null argument");
    if (!h->d_gate) return fail(QS_ERR_INVALID, "no gate: call qs_gate_create first");
    const qsx::Gate &g = h->gate_host;
    out->action_ring = g.act_ring; out->action_stride_bytes = (int64_t)g.act_stride; out->ring_len = (int32_t)g.ring_len;
    out->act_flag = g.act_flag; out->done_flag = g.done_flag; out->groups = (int32_t)g.groups;
    out->wg_per_group = (int32_t)g.wg_per_group; out->workgroups = (int32_t)g.blocks;
    out->envs_per_workgroup = h->epb; out->steps_launched = (int64_t)h->gate_step_seq; out->steps_fed = (int64_t)h->gate_prod_seq;
    return QS_OK;
}

int qs_step_gated(qs_handle *h, int32_t k, void *stream) {
    if (!h || k < 1) return fail(QS_ERR_INVALID, "bad argument");
    if (!h->d_gate) return fail(QS_ERR_INVALID, "no gate: call qs_gate_create first");
    if (h->profiling || h->replay_on || h->d_tape || h->pf.xchg)
        return fail(QS_ERR_UNSUPPORTED, "qs_step_gated: not available with per-launch profiling, the replay wrapper, a noise tape or the fused exchange");
    HIP_TRY(hipSetDevice(h->device));
    // stream-ordered behind everything on the caller's stream, and the caller's stream behind the launch - but the kernel itself sits in
    // the library's high-priority queue (see qs_handle::gate_stream)
    HIP_TRY(hipEventRecord(h->gate_ev_in, (hipStream_t)stream));
    HIP_TRY(hipStreamWaitEvent(h->gate_stream, h->gate_ev_in, 0));
    // the kernel's action-pointer argument carries the sequence base of this launch (qs_step_team.inc)
    int rc = launch_step(h, (const void *)(uintptr_t)h->gate_step_seq, h->gate_stream, k, true);
    if (rc != QS_OK) return rc;
    h->gate_step_seq += (unsigned long long)k;
    HIP_TRY(hipEventRecord(h->gate_ev_out, h->gate_stream));
    h->gate_pending = true;
    // NOT waited for on `stream` here: a wait packet in the caller's hardware queue would hold back whatever shares that queue - possibly
    // the producer this launch is waiting for.  qs_gate_wait orders a stream behind the launch when the caller asks for it.
    return QS_OK;
}

int qs_gate_wait(qs_handle *h, void *stream) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    if (!h->d_gate) return fail(QS_ERR_INVALID, "no gate: call qs_gate_create first");
    HIP_TRY(hipSetDevice(h->device));
    if (h->gate_step_seq > 0) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, h->gate_ev_out, 0));
    return QS_OK;
}

int qs_gate_produce(qs_handle *h, const void *src_actions_dev, int32_t n_src, int32_t k, int32_t closed_loop, void *stream) {
    if (!h || !src_actions_dev || n_src < 1 || k < 1) return fail(QS_ERR_INVALID, "bad argument");
    if (!h->d_gate) return fail(QS_ERR_INVALID, "no gate: call qs_gate_create first");
    if (((uintptr_t)src_actions_dev) & 15) return fail(QS_ERR_INVALID, "qs_gate_produce: the action table must be 16-byte aligned");
    HIP_TRY(hipSetDevice(h->device));
    const unsigned long long T = (unsigned long long)h->cfg.num_envs * h->cfg.num_agents;
    const unsigned long long wg_bytes = (unsigned long long)h->epb * h->cfg.num_agents * 4 * h->real_size,
        batch_bytes = T * 4 * h->real_size;
    hipLaunchKernelGGL(qs_gate_producer_kernel, dim3(h->gate_host.groups), dim3(256), 0, (hipStream_t)stream, h->d_gate,
                       (const char *)src_actions_dev, (unsigned int)n_src, h->gate_prod_seq, (int)k, (int)(closed_loop != 0), wg_bytes,
                       batch_bytes, (unsigned long long *)nullptr, (const unsigned int *)nullptr, (const unsigned int *)nullptr,
                       0ull, 0ull, 0ull, 0ull);
    HIP_TRY(hipGetLastError());
    h->gate_prod_seq += (unsigned long long)k;
    return QS_OK;
}

int qs_gate_produce_verify(qs_handle *h, const void *src_actions_dev, int32_t n_src, int32_t k, unsigned long long *sums_dev,
                           void *stream) {
    if (!h || !src_actions_dev || !sums_dev || n_src < 1 || k < 1) return fail(QS_ERR_INVALID, "bad argument");
    if (!h->d_gate) return fail(QS_ERR_INVALID, "no gate: call qs_gate_create first");
    if (((uintptr_t)src_actions_dev) & 15) return fail(QS_ERR_INVALID, "qs_gate_produce_verify: the action table must be 16-byte aligned");
    HIP_TRY(hipSetDevice(h->device));
    const unsigned long long T = (unsigned long long)h->cfg.num_envs * h->cfg.num_agents,
        rows_wg = (unsigned long long)h->epb * h->cfg.num_agents, wpr = h->real_size / 4;
    const unsigned long long wg_bytes = rows_wg * 4 * h->real_size, batch_bytes = T * 4 * h->real_size;
    hipLaunchKernelGGL(qs_gate_producer_kernel, dim3(h->gate_host.groups), dim3(256), 0, (hipStream_t)stream, h->d_gate,
                       (const char *)src_actions_dev, (unsigned int)n_src, h->gate_prod_seq, (int)k, 1, wg_bytes, batch_bytes, sums_dev,
                       (const unsigned int *)h->pf.obs, (const unsigned int *)h->pf.reward,
                       rows_wg * h->obs_dim * wpr, rows_wg * wpr, T * h->obs_dim * wpr, T * wpr);
    HIP_TRY(hipGetLastError());
    h->gate_prod_seq += (unsigned long long)k;
    return QS_OK;
}

int qs_gate_status(qs_handle *h, int64_t out[4]) {
    if (!h || !out) return fail(QS_ERR_INVALID, "null argument");
    if (!h->d_gate) return fail(QS_ERR_INVALID, "no gate: call qs_gate_create first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    qsx::Gate g;
    HIP_TRY(hipMemcpy(&g, h->d_gate, sizeof g, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> a(g.groups), d(g.blocks);
    HIP_TRY(hipMemcpy(a.data(), g.act_flag, a.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(d.data(), g.done_flag, d.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long amin = ~0ull, dmin = ~0ull;
    for (auto v : a) amin = v < amin ? v : amin;
    for (auto v : d) dmin = v < dmin ? v : dmin;
    out[0] = g.status; out[1] = (int64_t)h->gate_step_seq; out[2] = (int64_t)amin; out[3] = (int64_t)dmin;
    return QS_OK;
}

}  // extern "C"

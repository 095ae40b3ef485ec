// qs_rollout_targets.inc - what a PPO learner needs from a recorded rollout segment, in ONE launch behind it
// (include/quadswarm_encoder.h: qs_rollout_targets; part of qs_policy_encoder.hip's translation unit, behind its C ABI).
//
//   r_t   = clip(rewards_t * reward_scale, -reward_clip, +reward_clip)           nd_t = 1 - dones_t
//   d_t   = r_t + gamma * V_{t+1} * nd_t - V_t
//   adv_t = d_t + gamma * gae_lambda * nd_t * adv_{t+1},  adv_T = 0              ret_t = adv_t + V_t
//   logp_t = sum_k ( -0.5 * z_k^2 - log_std_k - 0.5 * log(2 pi) ),  z_k = (a_k - mean_k) * exp(-log_std_k)
// (tools/ppo_c5.py: Learner.advantages / gaussian_logp - Sample Factory's GAE with --value_bootstrap=False - which run as a Python loop
// of T iterations with ~ten elementwise kernels each.)
//
// Lane = agent: for a fixed step the 64 lanes of a wave read 64 consecutive rewards / values (256 B), done flags (64 B) and action rows
// (16 B each, one dwordx4 load per lane: 1 KiB per wave instruction).  The advantage is an affine recurrence in adv, so the time axis is
// cut into C chunks that C waves of a workgroup take in parallel:
//   pass 1  every wave folds its chunk [t0, t1) into adv_{t0} = P + Q * adv_{t1} (and writes the chunk's log-probabilities),
//   LDS     (P, Q) of all chunks of the 64 agents; the wave of chunk c composes the later chunks' maps from adv_T = 0 into its adv_{t1},
//   pass 2  the plain recurrence over the chunk from that value (rewards / done flags / values a second time, from L2), adv and ret stored.
// C = 1 is the plain form: one lane per agent runs all T steps, pass 2 only.  One thread owns each output element and every sum has a
// fixed order: same inputs, same bits, no atomics.  A/B of the forms on MI355X: DESIGN.md 8b (C = 16 and the plain form are built).

// the kernels' parameter block: qs_rollout_targets_params under the name their symbols carry
struct RolloutTargetsParams : qs_rollout_targets_params {};

#define RT_MAX_ACT 8
#define RT_HALF_LOG_2PI 0.9189385332046727f

template <int C>
__global__ void __launch_bounds__(64 * C) qs_rollout_targets_kernel(const RolloutTargetsParams p) {
    const int T = p.T, A = p.A;
    const int c = threadIdx.y;
    const int agent = blockIdx.x * 64 + threadIdx.x;
    const bool live = agent < A;
    const size_t a = live ? agent : A - 1;            // lanes behind the last agent read its rows and store nothing
    const int L = (T + C - 1) / C;
    const int t0 = c * L < T ? c * L : T, t1 = t0 + L < T ? t0 + L : T;   // this wave's steps (none when T < c * L)
    const float gamma = p.gamma, gl = p.gamma * p.gae_lambda, scale = p.reward_scale, clip = p.reward_clip;
    const float *__restrict__ rew = p.rewards + a;
    const uint8_t *__restrict__ done = p.dones + a;
    const float *__restrict__ val = p.values + a;

    if (p.logp != nullptr && p.means != nullptr) {
        // the chunk's log-probabilities: elementwise, no dependence between steps
        const int K = p.act_dim;
        float inv_std[RT_MAX_ACT], c0 = 0.0f;
#pragma unroll
        for (int k = 0; k < RT_MAX_ACT; ++k) {
            const float ls = k < K ? p.log_std[k] : 0.0f;
            inv_std[k] = expf(-ls);
            c0 -= k < K ? ls + RT_HALF_LOG_2PI : 0.0f;
        }
        if (K == 4 && ((((size_t)p.means | (size_t)p.actions)) & 15) == 0) {   // the action rows of the environments: one 16-byte load each
            const f32x4 *__restrict__ m4 = (const f32x4 *)p.means + a, *__restrict__ a4 = (const f32x4 *)p.actions + a;
#pragma unroll 4
            for (int t = t0; t < t1; ++t) {
                const f32x4 m = m4[(size_t)t * A], x = a4[(size_t)t * A];
                const float z0 = (x[0] - m[0]) * inv_std[0], z1 = (x[1] - m[1]) * inv_std[1];
                const float z2 = (x[2] - m[2]) * inv_std[2], z3 = (x[3] - m[3]) * inv_std[3];
                const float lp = c0 - 0.5f * ((z0 * z0 + z1 * z1) + (z2 * z2 + z3 * z3));
                if (live) p.logp[(size_t)t * A + a] = lp;
            }
        } else {
            for (int t = t0; t < t1; ++t) {
                const float *__restrict__ m = p.means + ((size_t)t * A + a) * K, *__restrict__ x = p.actions + ((size_t)t * A + a) * K;
                float s = 0.0f;
#pragma unroll
                for (int k = 0; k < RT_MAX_ACT; ++k)
                    if (k < K) { const float z = (x[k] - m[k]) * inv_std[k]; s += z * z; }
                if (live) p.logp[(size_t)t * A + a] = c0 - 0.5f * s;
            }
        }
    }

    float adv = 0.0f;                                  // adv_{t1}: 0 behind the last step
    if constexpr (C > 1) {
        __shared__ float sP[C][64], sQ[C][64];
        float P = 0.0f, Q = 1.0f, vn = val[(size_t)t1 * A];
#pragma unroll 4
        for (int t = t1 - 1; t >= t0; --t) {
            const float r = fminf(fmaxf(rew[(size_t)t * A] * scale, -clip), clip), nd = 1.0f - (float)done[(size_t)t * A], v = val[(size_t)t * A];
            const float d = r + gamma * vn * nd - v, k = gl * nd;
            P = d + k * P;
            Q = k * Q;
            vn = v;
        }
        sP[c][threadIdx.x] = P;
        sQ[c][threadIdx.x] = Q;
        __syncthreads();
        for (int j = C - 1; j > c; --j) adv = sP[j][threadIdx.x] + sQ[j][threadIdx.x] * adv;
    }
    float vn = val[(size_t)t1 * A];
#pragma unroll 4
    for (int t = t1 - 1; t >= t0; --t) {
        const float r = fminf(fmaxf(rew[(size_t)t * A] * scale, -clip), clip), nd = 1.0f - (float)done[(size_t)t * A], v = val[(size_t)t * A];
        const float d = r + gamma * vn * nd - v;
        adv = d + gl * nd * adv;
        if (live) {
            p.advantages[(size_t)t * A + a] = adv;
            p.returns[(size_t)t * A + a] = adv + v;
        }
        vn = v;
    }
}

// waves per workgroup = chunks of the time axis.  Measured at T = 128, A = 8192 on MI355X (profiles/r08_bench_rollout_targets.jsonl, DESIGN.md
// 8b; us per launch, inputs not cache-resident): plain 119, 2 chunks 55.8, 4: 33.0, 8: 20.9, 16: 15.5 - the more chunks the faster, up to the
// 1024 threads of a workgroup.  Kept: the winner and the plain form.  16 chunks from T = 32 on (chunks of at least two steps; only T = 128 is
// measured), the plain form below.  qs_rollout_set_targets_chunks is a switch for tools/bench_rollout_targets.py and the test of both forms,
// NOT part of include/quadswarm_encoder.h: process-global, not synchronised, and a launch recorded into a HIP graph keeps the form that was
// set when it was captured.  Accepted: 0 (the rule above), 1, 16; anything else only reads; returns the previous value.  The forms differ in
// the last bits of the advantages (another association of the same sums).
#define RT_CHUNKS 16
static int g_targets_chunks = 0;
static int rollout_targets_chunks(int T) {
    if (g_targets_chunks > 0) return g_targets_chunks;
    return T >= 32 ? RT_CHUNKS : 1;
}

extern "C" {

size_t qs_rollout_sizeof_targets(void) { return sizeof(qs_rollout_targets_params); }

int32_t qs_rollout_set_targets_chunks(int32_t chunks) {
    const int prev = g_targets_chunks;
    if (chunks == 0 || chunks == 1 || chunks == RT_CHUNKS) g_targets_chunks = chunks;
    return prev;
}

int qs_rollout_targets(const qs_rollout_targets_params *p, void *stream) {
    if (!p) { g_enc_error = "qs_rollout_targets: NULL parameter struct"; return -1; }
    if (!p->rewards || !p->dones || !p->values || !p->advantages || !p->returns) {
        g_enc_error = "qs_rollout_targets: rewards, dones, values, advantages and returns must not be NULL"; return -1; }
    if (p->T < 1 || p->A < 1) { g_enc_error = "qs_rollout_targets: T and A must be at least 1"; return -1; }
    if ((p->means == nullptr) != (p->actions == nullptr)) {
        g_enc_error = "qs_rollout_targets: means and actions go together (both, or both NULL for no log-probabilities)"; return -1; }
    if (p->means) {
        if (p->act_dim < 1 || p->act_dim > RT_MAX_ACT) { g_enc_error = "qs_rollout_targets: act_dim must be 1..8"; return -1; }
        if (!p->log_std) { g_enc_error = "qs_rollout_targets: log_std must not be NULL when means / actions are given"; return -1; }
    }
    if (!(p->gamma >= 0.0f && p->gamma <= 1.0f) || !(p->gae_lambda >= 0.0f && p->gae_lambda <= 1.0f)) {
        g_enc_error = "qs_rollout_targets: gamma and gae_lambda must be in [0, 1]"; return -1; }
    if (!(p->reward_clip > 0.0f)) { g_enc_error = "qs_rollout_targets: reward_clip must be positive"; return -1; }
    const dim3 grid((p->A + 63) / 64);
    const RolloutTargetsParams kp{*p};
    if (rollout_targets_chunks(p->T) == 1) hipLaunchKernelGGL(qs_rollout_targets_kernel<1>, grid, dim3(64, 1), 0, (hipStream_t)stream, kp);
    else hipLaunchKernelGGL(qs_rollout_targets_kernel<RT_CHUNKS>, grid, dim3(64, RT_CHUNKS), 0, (hipStream_t)stream, kp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_enc_error = hipGetErrorString(e); return -2; }
    return 0;
}

}

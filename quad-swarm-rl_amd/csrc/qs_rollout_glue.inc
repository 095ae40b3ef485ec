// qs_rollout_glue.inc - qs_rollout_pre / qs_rollout_post (include/quadswarm_encoder.h), kernels and entry points; part of
// qs_policy_encoder.hip's translation unit (glue_philox: qs_enc_device.h, g_enc_error: the unit).
//
// Closed-loop glue (quad-swarm-rl_amd/rollout.py): what sits between the encoder and the environment step in a rollout segment,
// as ONE launch before the step (trajectory copy of the observations + Gaussian sampling of the actions from the head's mean)
// and ONE after it (trajectory copies of rewards / dones) instead of eight small framework kernels (copy, randn, exp, mul, add,
// copy, copy, copy) at 1.5 - 2 us each inside a HIP graph.  The noise is Philox4x32-10 keyed (seed, launch counter, agent); the
// counter lives in device memory and is advanced by the second launch, so a captured graph draws fresh noise on every replay.
extern "C" __global__ void __launch_bounds__(256) qs_rollout_pre_kernel(const float *__restrict__ obs, float *__restrict__ obs_out,
    int n_obs, const float *__restrict__ mean,
                                                                        const float *__restrict__ log_std, float *__restrict__ act_out,
                                                                            int A, uint32_t seed_lo,
                                                                        uint32_t seed_hi, const uint32_t *__restrict__ counter) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
    // 16-byte copies when both rows are 16-byte aligned (a trajectory slot obs[t] of A * D floats is only when A * D % 4 == 0)
    const int n4 = (((size_t)obs | (size_t)obs_out) & 15) == 0 ? n_obs >> 2 : 0;
    for (int i = tid; i < n4; i += nthreads) ((f32x4 *)obs_out)[i] = ((const f32x4 *)obs)[i];
    for (int i = (n4 << 2) + tid; i < n_obs; i += nthreads) obs_out[i] = obs[i];
    const bool act16 = ((((size_t)mean | (size_t)act_out)) & 15) == 0;
    for (int a = tid; a < A; a += nthreads) {
        f32x4 m;
        if (act16) m = *(const f32x4 *)(mean + (size_t)a * 4);
        else { m[0] = mean[(size_t)a * 4]; m[1] = mean[(size_t)a * 4 + 1]; m[2] = mean[(size_t)a * 4 + 2]; m[3] = mean[(size_t)a * 4 + 3]; }
        if (log_std) {   // action = mean + exp(log_std) * N(0, 1): two Box-Muller pairs from one Philox group
            uint32_t w[4];
            glue_philox((uint32_t)a, *counter, 0x51u, 0u, seed_lo, seed_hi, w);
            const float u0 = ((float)(w[0] >> 9) + 0.5f) * (1.0f / 8388608.0f), u1 = ((float)(w[1] >> 9) + 0.5f) * (1.0f / 8388608.0f);
            const float u2 = ((float)(w[2] >> 9) + 0.5f) * (1.0f / 8388608.0f), u3 = ((float)(w[3] >> 9) + 0.5f) * (1.0f / 8388608.0f);
            const float r0 = sqrtf(-2.0f * __logf(u0)), r1 = sqrtf(-2.0f * __logf(u2));
            float s0, c0, s1, c1;
            __sincosf(6.283185307179586f * u1, &s0, &c0);
            __sincosf(6.283185307179586f * u3, &s1, &c1);
            m[0] += __expf(log_std[0]) * r0 * c0; m[1] += __expf(log_std[1]) * r0 * s0;
            m[2] += __expf(log_std[2]) * r1 * c1; m[3] += __expf(log_std[3]) * r1 * s1;
        }
        if (act16) *(f32x4 *)(act_out + (size_t)a * 4) = m;
        else { act_out[(size_t)a * 4] = m[0]; act_out[(size_t)a * 4 + 1] = m[1]; act_out[(size_t)a * 4 + 2] = m[2];
            act_out[(size_t)a * 4 + 3] = m[3]; }
    }
}
extern "C" __global__ void __launch_bounds__(256) qs_rollout_post_kernel(const float *__restrict__ rew, float *__restrict__ rew_out,
    const uint8_t *__restrict__ done,
                                                                         uint8_t *__restrict__ done_out, int A,
                                                                             uint32_t *__restrict__ counter) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
    for (int a = tid; a < A; a += nthreads) { rew_out[a] = rew[a]; done_out[a] = done[a]; }
    if (tid == 0) *counter += 1u;
}
extern "C" {

// obs[n_obs] -> obs_out, act_out[A, 4] = mean[A, 4] (+ exp(log_std[4]) * N(0, 1) if log_std != NULL)
int qs_rollout_pre(const float *obs, float *obs_out, int32_t n_obs, const float *mean, const float *log_std, float *act_out, int32_t A,
    uint64_t seed,
                   const uint32_t *counter, void *stream) {
    if ((n_obs > 0 && (!obs || !obs_out)) || !mean || !act_out || !counter || n_obs < 0 || A < 0) { g_enc_error = "bad argument";
        return -1; }
    if (A == 0 && n_obs == 0) return 0;
    const int work = (n_obs >> 2) > A ? (n_obs >> 2) : A, blocks = (work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048;
    hipLaunchKernelGGL(qs_rollout_pre_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, (hipStream_t)stream, obs, obs_out, n_obs,
        mean, log_std, act_out, A,
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), counter);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_enc_error = hipGetErrorString(e); return -2; }
    return 0;
}
// rew[A] -> rew_out, done[A] -> done_out, *counter += 1 (the next qs_rollout_pre draws new noise)
int qs_rollout_post(const float *rew, float *rew_out, const uint8_t *done, uint8_t *done_out, int32_t A, uint32_t *counter, void *stream) {
    if (!rew || !rew_out || !done || !done_out || !counter || A < 0) { g_enc_error = "bad argument"; return -1; }
    hipLaunchKernelGGL(qs_rollout_post_kernel, dim3((A + 255) / 256 > 0 ? ((A + 255) / 256 < 2048 ? (A + 255) / 256 : 2048) : 1),
        dim3(256), 0, (hipStream_t)stream, rew, rew_out, done, done_out, A, counter);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_enc_error = hipGetErrorString(e); return -2; }
    return 0;
}

}

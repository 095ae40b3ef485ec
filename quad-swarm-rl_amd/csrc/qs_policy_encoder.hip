// qs_policy_encoder.hip - fused forward pass of the quad-swarm policy encoder on gfx950 matrix cores.
//
// Reference: swarm_rl/models/quad_multi_model.py:250-350 (QuadMultiEncoder: self encoder, neighbour encoder, optional obstacle
// encoder, feed-forward) with the `mean_embed` neighbour encoder (:22-43, QuadNeighborhoodEncoderDeepsets); tanh non-linearity,
// hidden size 256.  It reads the observation rows straight from the stepper's buffer.
// The `attention` neighbour encoder (:46-101) takes two kernels: its `self_obs.repeat(K, 1)` (:84) and `mean.repeat(K, 1)` (:92)
// tile the WHOLE batch, so row (agent a, neighbour k) is paired with the self observation and the mean embedding of agent
// (a*K + k) mod batch - an inter-agent dependence on an intermediate result.  qs_encoder_embed_kernel computes e_i for every row
// (with that self observation) and g = W_m e_mean per agent; qs_encoder_kernel then runs value MLP, score MLP (W_e e_i + g[(a*K+k)
// mod B] + b), softmax over the neighbours and the weighted sum, all lane-local across accumulator tiles.
//
// One workgroup = 8 waves = 16 agents.  Every layer is a transposed GEMM on v_mfma_f32_16x16x32_bf16:
//     C[feature][row] = sum_k W[feature][k] * X[row][k]
//   A operand = weights, packed on the host in fragment order ([M/16][K/32][64 lanes][8 bf16]) and streamed from L2 with one
//               16-byte load per lane;
//   B operand = activations, row-major bf16 in LDS with K contiguous (one ds_read_b128 per lane);
//   C         = 4 consecutive features of one row per lane  ->  bias, tanh, bf16, one 8-byte LDS store.
// Wave w owns features [32w, 32w+32) of a 256-wide layer.  Neighbour rows are ordered neighbour-major (row = k*16 + agent), so
// the row tile index IS the neighbour index and the mean over neighbours is a lane-local sum across accumulator tiles.
// Operand layout verified on hardware by tools/mfma_layout_probe.hip.
//
// ONE translation unit, cut along its seams; this file keeps the C ABI and includes, in the order of the kernels in the code object:
//   qs_enc_plan.h (plain C++: constants, LDS layouts, the kernel list, enc_select), qs_enc_device.h (shared device pieces),
//   qs_enc_attn16.inc (attention, 16 agents: embed + attn), qs_enc_mha.inc (multi-head / Sim2Real), qs_enc_main16.inc (mean_embed / mlp /
//   no_encoder, 16 agents), qs_enc_wide.inc (32 agents: weight ring, wide, ping-pong, attention), qs_enc_narrow.inc (Sim2Real at rnn_size 16 / 32 /
//   64: one wave per 16 agents, static LDS, outside the kernel list; its host side is qs_enc_narrow_plan.h), qs_rollout_glue.inc,
//   qs_rollout_targets.inc, qs_value_map.inc, qs_attn_weights.inc (the attention weights as an output: kernels and a table of their own).
#include <hip/hip_runtime.h>
#include <mutex>
#include <stdlib.h>
#include <stdint.h>

#include <string>

#include "../../include/quadswarm_encoder.h"
#include "qs_enc_plan.h"
#include "qs_enc_narrow_plan.h"
#include "qs_enc_device.h"
#include "qs_enc_attn16.inc"
#include "qs_enc_mha.inc"
#include "qs_enc_main16.inc"
#include "qs_enc_wide.inc"
#include "qs_enc_narrow.inc"

static thread_local std::string g_enc_error;
#include "qs_rollout_glue.inc"

// ------------------------------------------------------------------------------------------------
// C ABI (include/quadswarm_encoder.h)
// ------------------------------------------------------------------------------------------------
#define ENC_KERNEL_ROW(sym, lds, agents, has_out) {(const void *)sym, #sym, lds, agents, has_out},
static const EncKernel enc_kernels[ENC_NUM_KERNELS] = {ENC_KERNELS(ENC_KERNEL_ROW)};
#undef ENC_KERNEL_ROW

extern "C" {

const char *qs_enc_last_error(void) { return g_enc_error.c_str(); }
size_t qs_enc_sizeof_params(void) { return sizeof(qs_enc_params); }

// Batches from this many agents on take the 32-agent workgroups (mean_embed, attention).  Default (-1): more agents than one
// 16-agent workgroup per CU can hold - up to there every 16-agent workgroup has a CU to itself and its shorter chain wins (measured
// 8192 / 4096 agents, us: mean_embed 28.4 / 18.9 narrow vs 25.0 / 22.3 wide, attention 76.5 / 51.0 vs 70.1 / 68.2;
// tools/enc_threshold.sh).  0 = never; QS_ENC_WIDE_MIN / qs_enc_set_wide_min override.
static int g_wide_min = [] { const char *e = getenv("QS_ENC_WIDE_MIN"); return e ? atoi(e) : -1; }();
static int wide_min_agents(int dev) {
    if (g_wide_min >= 0) return g_wide_min;
    static int cus[64] = {0};
    if (dev < 0 || dev >= 64) return 4097;
    if (!cus[dev]) { int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError();
        n = 256; } cus[dev] = n; }
    return ENC_TA * cus[dev] + 1;
}
// mean_embed on 32-agent workgroups: the ping-pong schedule (pp_body) or, QS_ENC_PP=0 / qs_enc_set_pingpong(0), the lock-step one (wide_body)
static int g_pp = [] { const char *e = getenv("QS_ENC_PP"); return e ? atoi(e) : 1; }();
int32_t qs_enc_set_pingpong(int32_t on) { const int prev = g_pp; if (on >= 0) g_pp = on != 0; return prev; }
// -1: the default rule; < -1: read only
int32_t qs_enc_set_wide_min(int32_t agents) { const int prev = g_wide_min; if (agents >= -1) g_wide_min = agents; return prev; }
size_t qs_enc_lds_bytes(void) { return EncLdsMain::bytes; }
// LDS request of the kernel that serves `model` (QS_ENC_NBR_* / QS_ENC_MODEL_*): the multi-head and Sim2Real kernels ask for more than
// half of a CU's 160 KiB ON PURPOSE - one workgroup per CU by construction (an experiment with two co-resident
// workgroups of this body was not run-to-run deterministic and was never shipped); tests/test_c_abi.py pins that.
size_t qs_enc_lds_bytes_of(int32_t model) {
    if (model == QS_ENC_MODEL_MHA || model == QS_ENC_MODEL_S2R) return EncLdsMha::bytes;
    if (model == QS_ENC_NBR_ATTENTION) return EncLdsEmbed::bytes > EncLdsMain::bytes ? EncLdsEmbed::bytes : EncLdsMain::bytes;
    return EncLdsMain::bytes;
}
size_t qs_enc_lds_bytes_split(int32_t attention) { return attention ? EncLdsSplit::bytes_scores : EncLdsSplit::bytes; }

// the Sim2Real encoder at rnn_size 16 / 32 / 64 (qs_enc_narrow.inc)
static const void *narrow_kernel(int H) {
    return H == 16 ? (const void *)qs_encoder_narrow16_kernel : H == 32 ? (const void *)qs_encoder_narrow32_kernel : (const void *)qs_encoder_narrow64_kernel;
}

// out[B, 512] (QS_ENC_MODEL_S2R: [B, 256]) = encoder(obs[B, obs_dim]); all pointers (obs, out, the weights / biases inside `params`) are
// device pointers
int qs_enc_forward(const float *obs, int32_t B, const qs_enc_params *params, float *out, void *stream) {
    if (!obs || !params || B < 0) { g_enc_error = "bad argument"; return -1; }
    const EncParams &P = *params;
    if (P.head_dim < 0 || P.head_dim > 8 || (P.head_dim > 0 && (!P.head_w || !P.head_b || !P.head_out)) || (!out && P.head_dim == 0) ||
        (P.sample_log_std && (P.head_dim == 0 || !P.act_out || !P.sample_counter))) {
        g_enc_error = "bad argument";   // neither the features nor a head output requested, or an incomplete head
        return -1;
    }
    const bool att = P.nbr_encoder == QS_ENC_NBR_ATTENTION && P.num_nbr > 0, s2r = P.nbr_encoder == QS_ENC_MODEL_S2R,
        mha = P.nbr_encoder == QS_ENC_MODEL_MHA || s2r, sp = P.precision == 1;
    if (P.precision != 0 && P.precision != 1) { g_enc_error = "precision: 0 (bf16) or 1 (reference precision, fp16 pairs)"; return -1; }
    if (P.num_nbr > ENC_MAX_NBR || P.self_dim > 32 || P.obst_dim > 32 || P.nbr_dim > 32 || P.nbr_encoder < 0
        || P.nbr_encoder > QS_ENC_MODEL_S2R ||
        (att && P.self_dim + P.nbr_dim > 32) || ((P.nbr_encoder == QS_ENC_NBR_MLP || mha) && P.nbr_dim * P.num_nbr > 64) ||
        (mha && (P.num_nbr < 1 || P.obst_dim < 1 || !P.ln_w || !P.ln_b))) {
        g_enc_error = "unsupported encoder shape (inputs wider than 32 - 64 for the mlp neighbour encoder - or more than 8 neighbours)";
        return -4;
    }
    if (att && !P.a3w) { g_enc_error = "the attention neighbour encoder needs the last score layer's weight row (a3w)"; return -1; }
    if (att && (!P.ebuf || !P.gbuf)) { g_enc_error = "the attention neighbour encoder needs the ebuf / gbuf scratch buffers"; return -1; }
    if (att && (int64_t)B * P.num_nbr * (ENC_H * 2) * (sp ? 2 : 1) > 0x7fffffffll) { g_enc_error = "attention: batch x neighbours too large for 32-bit scratch offsets"; return -4; }
    if ((int64_t)B * P.obs_dim * 4 > 0xffffffffll) { g_enc_error = "batch x obs_dim too large for 32-bit observation offsets"; return -4; }
    if (B == 0) return 0;
    // the Sim2Real encoder below 256 features: kernels of their own (qs_enc_narrow.inc), refused here - before any device is touched - where they are not built
    const bool narrow = enc_narrow_route(P.nbr_encoder, P.s1.M);
    if (narrow) {
        if (!enc_narrow_width(P.s1.M)) { g_enc_error = "the Sim2Real encoder is built for rnn_size 16, 32, 64 and 256"; return -4; }
        if (!enc_narrow_consistent(P)) { g_enc_error = "narrow Sim2Real encoder: every layer has M = rnn_size, the attention block K = ceil32(rnn_size), the feed-forward layer K = ceil32(3 rnn_size)"; return -4; }
        if (!sp) { g_enc_error = "narrow widths run in reference precision"; return -4; }
    }
    // launch on the device that owns `obs` (a process may drive several GPUs); the > 64 KB dynamic-LDS attribute is per device
    int dev = 0;
    {
        hipPointerAttribute_t pa;
        if (hipPointerGetAttributes(&pa, obs) == hipSuccess) dev = pa.device; else { (void)hipGetLastError(); (void)hipGetDevice(&dev); }
        if (hipSetDevice(dev) != hipSuccess) { g_enc_error = "hipSetDevice failed"; return -2; }
    }
    if (narrow) {   // static LDS, far below 64 KiB: no attribute to raise
        void *args[] = {&obs, &B, (void *)params, &out};
        (void)hipLaunchKernel(narrow_kernel(P.s1.M), dim3(enc_narrow_grid(B, ENC_NW_WAVES)), dim3(64 * ENC_NW_WAVES), args, 0, (hipStream_t)stream);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { g_enc_error = hipGetErrorString(e); return -2; }
        return 0;
    }
    {
        static std::mutex attr_mutex;
        static uint64_t attr_set = 0;   // bit d: attributes set on device d
        std::lock_guard<std::mutex> lock(attr_mutex);
        if (dev < 0 || dev >= 64) { g_enc_error = "device index out of range"; return -2; }
        if (!(attr_set >> dev & 1)) {
            for (const EncKernel &k : enc_kernels)
                if (hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes) != hipSuccess) {
                    g_enc_error = "cannot raise the dynamic LDS limit";
                    return -2;
                }
            attr_set |= 1ull << dev;
        }
    }
    const EncPlan plan = enc_select(P.nbr_encoder, P.num_nbr, P.obst_dim, P.precision, B, wide_min_agents(dev), g_pp);
    for (int i = 0; i < plan.n; ++i) {
        const EncKernel &k = enc_kernels[plan.kernel[i]];
        void *args[] = {&obs, &B, (void *)params, k.has_out ? &out : nullptr};
        (void)hipLaunchKernel(k.fn, dim3((B + k.agents - 1) / k.agents), dim3(64 * ENC_WAVES), args, k.lds_bytes, (hipStream_t)stream);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_enc_error = hipGetErrorString(e); return -2; }
    return 0;
}

#ifdef ENC_TIMING
int qs_enc_stamps(unsigned long long *out16) { return hipMemcpyFromSymbol(out16, HIP_SYMBOL(enc_stamps),
    sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -2; }
int qs_enc_wg_times(unsigned long long *out,
    int n) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(enc_wg_times), sizeof(unsigned long long) * 2 * n) == hipSuccess ? 0 : -2; }
#endif
// `iters` back-to-back forward passes timed with HIP events on `stream` (no host work in between): average ms per pass
int qs_enc_benchmark(const float *obs, int32_t B, const EncParams *params, float *out, void *stream, int32_t iters, double *avg_ms) {
    if (iters < 1 || !avg_ms) { g_enc_error = "bad argument"; return -1; }
    int rc = qs_enc_forward(obs, B, params, out, stream);   // warm-up (+ sets the LDS attribute)
    if (rc != 0) return rc;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { g_enc_error = "hipEventCreate failed"; return -2; }
    (void)hipEventRecord(e0, (hipStream_t)stream);
    for (int i = 0; i < iters && rc == 0; ++i) rc = qs_enc_forward(obs, B, params, out, stream);
    (void)hipEventRecord(e1, (hipStream_t)stream);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *avg_ms = (double)ms / iters;
    return rc;
}
}

#include "qs_rollout_targets.inc"   // qs_rollout_targets: values -> log-probabilities, advantages, returns of a recorded segment
#include "qs_value_map.inc"         // qs_value_map: observation rows -> hypothetical rows over an offset grid -> the critic -> per-agent extrema
#include "qs_attn_weights.inc"      // qs_attn_weights: observation rows -> the softmax the attention encoders compute, stored instead of applied

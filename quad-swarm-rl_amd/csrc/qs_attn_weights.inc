// qs_attn_weights.inc - the attention weights of the policy encoders as an output (include/quadswarm_attention.h: the semantics are stated
// THERE, once; part of qs_policy_encoder.hip's translation unit because its kernels are built from the forward kernels' device pieces).
//
// The forward kernels compute these softmaxes and keep them in registers (attn_pass folds its scores into an online softmax, mha_body_split and
// narrow_body hold pr[2][2]).  The kernels here run the part of the same bodies that the weights depend on - reference precision only, the same
// fp16-pair GEMMs, fp32 scores and softmax - and store the softmax instead of applying it:
//
//   attention   launch 1 is qs_encoder_embed_split_kernel itself (e_i -> ebuf, W_m e_mean -> gbuf).  Launch 2, qs_attn_scores_kernel, is the
//               score half of attn_pass - a1e on e_i plus the gbuf row of agent (a*K + k) mod B, a2, the 256 -> 1 row from the accumulators -
//               over the K slots of 16 agents in groups of ENC_ANH row tiles, without the value MLP, the self / obstacle encoders and the
//               feed-forward layer.  The scores of all slots meet in LDS; one thread per agent takes a plain softmax over them and stores [K].
//   MHA / S2R   qs_attn_mha_kernel / qs_attn_s2r_kernel: mha_body_split up to pr[2][2] - neighbour and obstacle embeddings, the mq / mk
//               projections, the 2 x 2 scores per head with 1 / sqrt(256) - without the self encoder, the value projection, fc, LayerNorm and
//               the feed-forward layer.  The even wave of a head (wave 0 for the one head of S2R) stores its [2][2].
//   narrow S2R  qs_attn_narrow{16,32,64}_kernel: narrow_body up to pr[2][2], one wave per 16 agents; lane group 0 stores.
//
// They are outside ENC_KERNELS (the list enc_select indexes): a table of their own below.

// LDS of qs_attn_scores_kernel: the two group buffers of EncLdsAttn inside each plane, behind both planes the float scratch
struct EncLdsAttnW {
    static constexpr int buf_a = EncLdsAttn::buf_a;                        // [ANH*16][YS]  e_i of the group
    static constexpr int buf_h = EncLdsAttn::buf_h;                        // [ANH*16][YS]  first score layer
    static constexpr int s_alpha = EncLdsSplit::s_alpha;                   // float [8 waves][ANH][16]  partial scores of the group
    static constexpr int s_score = s_alpha + 2 * ENC_WAVES * ENC_ANH * 16; // float [MAX_NBR][16]  scores of every slot
    static constexpr int end = s_score + 2 * ENC_MAX_NBR * 16, bytes = 2 * end;
};
static_assert(EncLdsAttnW::buf_h + ENC_ANH * ENC_TA * ENC_YS <= ENC_SPLANE && EncLdsAttnW::bytes <= 160 * 1024, "the score kernel's LDS fits a CU");

// ------------------------------------------------------------------------------------------------
// attention, launch 2: scores of one group of NTH neighbour row tiles (attn_pass's first half), summed over the waves into s_score
// ------------------------------------------------------------------------------------------------
template <int NTH>
__device__ __forceinline__ void attnw_score_pass(const EncParams &P, int B, int a0, int t0, uint16_t *buf_a, uint16_t *buf_h, float *s_alpha,
    float *s_score) {
    const int wave = wave_id(), lane = threadIdx.x & 63, mt0 = wave * ENC_MT;
    const int ga = a0 + (lane & 15);
    attn_load_e<NTH, true>(P, B, a0, t0, buf_a);   // (every wave is behind the last barrier of the previous group: nobody reads buf_a)
    f32x4 acc[ENC_MT][NTH];
    // first layer on [e_i | e_mean.repeat(K, 1)]: W_e e_i + b + g[(a*K + k) mod B]   (:92-94)
    init_bias<ENC_MT, NTH>(P.a1e, mt0, acc);
    {
        const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void *)P.gbuf, 0, (uint32_t)B * (ENC_H * 4), 0x00020000);
#pragma unroll
        for (int nt = 0; nt < NTH; ++nt) {
            const uint32_t j = mod_batch((uint32_t)ga * (uint32_t)P.num_nbr + (uint32_t)(t0 + nt), (uint32_t)B, 1.0f / (float)B);
            const uint32_t off = ga < B ? j * (ENC_H * 4) + (lane >> 4) * 16 : 0xffffffffu;   // padding rows: out of range, reads zero
#pragma unroll
            for (int mt = 0; mt < ENC_MT; ++mt) {
                const f32x4 gv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(grs, off, (mt0 + mt) * 64, 0));
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[mt][nt][r] += gv[r];
            }
        }
    }
    __syncthreads();   // e_i is in buf_a
    gemm_tiles<ENC_MT, NTH, true>(P.a1e, mt0, buf_a, ENC_YS, acc);
    store_tanh<ENC_MT, NTH, true>(acc, mt0, buf_h, ENC_YS);
    __syncthreads();
    init_bias<ENC_MT, NTH>(P.a2, mt0, acc);
    gemm_tiles<ENC_MT, NTH, true>(P.a2, mt0, buf_h, ENC_YS, acc);
    // last score layer 256 -> 1 from the accumulators: per-lane partial dot product, two shuffles over the lane groups, the waves through LDS
#pragma unroll
    for (int nt = 0; nt < NTH; ++nt) {
        float sp = 0.0f;
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) {
            const f32x4 w = *(const f32x4 *)(P.a3w + (mt0 + mt) * 16 + (lane >> 4) * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) sp += fast_tanh(acc[mt][nt][r]) * w[r];
        }
        sp = lane_groups_sum(sp);
        if (lane < 16) s_alpha[(wave * ENC_ANH + nt) * 16 + lane] = sp;
    }
    __syncthreads();   // partial scores visible; every wave is done reading buf_h
    if ((int)threadIdx.x < NTH * 16) {   // one thread per (slot, agent): bias + the eight partials in wave order, as attn_pass adds them
        const int nt = threadIdx.x >> 4, a = threadIdx.x & 15;
        float s = P.a3b;
#pragma unroll
        for (int w = 0; w < ENC_WAVES; ++w) s += s_alpha[(w * ENC_ANH + nt) * 16 + a];
        s_score[(t0 + nt) * 16 + a] = s;   // (the next group writes s_alpha behind two more barriers)
    }
}

extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_attn_scores_kernel(const float *__restrict__ obs, int B, EncParams P,
    float *__restrict__ weights) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsAttnW Lds;
    uint16_t *const lds = (uint16_t *)smem, *buf_a = lds + Lds::buf_a, *buf_h = lds + Lds::buf_h;
    float *s_alpha = (float *)(lds + Lds::s_alpha), *s_score = (float *)(lds + Lds::s_score);
    const int a0 = blockIdx.x * ENC_TA, NB = P.num_nbr;
    (void)obs;   // (the rows were read by launch 1; the argument keeps the encoder kernels' signature)
    for (int t0 = 0; t0 < NB; t0 += ENC_ANH) {
#define ENC_CALL(n) attnw_score_pass<n>(P, B, a0, t0, buf_a, buf_h, s_alpha, s_score)
        ENC_DISPATCH_NT(NB - t0, ENC_ANH, ENC_CALL)
#undef ENC_CALL
    }
    __syncthreads();
    // softmax over the neighbours (:95-96), plain: thread a owns the K weights of agent a0 + a
    const int a = threadIdx.x, ga = a0 + a;
    if (a < ENC_TA && ga < B) {
        float mx = -3.0e38f, den = 0.0f;
        for (int k = 0; k < NB; ++k) mx = fmaxf(mx, s_score[k * 16 + a]);
        for (int k = 0; k < NB; ++k) den += __expf(s_score[k * 16 + a] - mx);
        for (int k = 0; k < NB; ++k) weights[(size_t)ga * NB + k] = __expf(s_score[k * 16 + a] - mx) / den;
    }
}

// ------------------------------------------------------------------------------------------------
// QuadMultiHeadAttentionEncoder / its Sim2Real subclass at width 256: mha_body_split up to the softmax over the keys
// ------------------------------------------------------------------------------------------------
template <bool S2R>
__device__ __forceinline__ void attnw_mha_body(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ weights) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsMhaSplit Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_obst = lds + Lds::x_obst, *x_nbr = lds + Lds::x_nbr;
    uint16_t *hid = lds + Lds::hid, *tok = lds + Lds::tok;
    float *red_s = (float *)(lds + Lds::red_s);
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, a0 = blockIdx.x * ENC_TA;
    const int NB = P.num_nbr, D = P.obs_dim, mt0 = wave * ENC_MT, nbw = P.nbr_dim * NB;
    // columns as fp16 pairs, zero padded: [obstacle 32 | neighbours 64]
    for (int idx = tid; idx < ENC_TA * 96; idx += 64 * ENC_WAVES) {
        const int a = idx / 96, c = idx - a * 96, ga = a0 + a;
        int col = -1;
        uint16_t *dst;
        if (c < 32) { dst = x_obst + a * ENC_XS + c; if (c < P.obst_dim) col = P.self_dim + nbw + c; }
        else { dst = x_nbr + a * ENC_XW + (c - 32); if (c - 32 < nbw) col = P.self_dim + (c - 32); }
        put1<true>(dst, obs_at(obs_rsrc(obs, B, D), ga < B && col >= 0, (uint32_t)ga * (uint32_t)D + col));
    }
    __syncthreads();
    if constexpr (S2R) {   // one layer per embedding (:229-240).  (Spelled out, not mlp1_keep<false, true>: with a second user of that instance
                           // qs_encoder_s2r_split_kernel came out with another scalar register allocation - the forward kernels stay byte-identical)
        f32x4 acc[ENC_MT][1];
        init_bias<ENC_MT, 1>(P.n1, mt0, acc);
        gemm_tiles<ENC_MT, 1, true>(P.n1, mt0, x_nbr, ENC_XW, acc);
        store_tanh<ENC_MT, 1, true>(acc, mt0, tok, ENC_YS);
        init_bias<ENC_MT, 1>(P.o1, mt0, acc);
        gemm_tiles<ENC_MT, 1, true>(P.o1, mt0, x_obst, ENC_XS, acc);
        store_tanh<ENC_MT, 1, true>(acc, mt0, tok + ENC_TA * ENC_YS, ENC_YS);
    } else {
        mlp2_one_tile<true>(P.n1, P.n2, mt0, x_nbr, ENC_XW, hid, tok, ENC_YS, 0);
        __syncthreads();
        mlp2_one_tile<true>(P.o1, P.o2, mt0, x_obst, ENC_XS, hid, tok + ENC_TA * ENC_YS, ENC_YS, 0);
    }
    __syncthreads();
    // s[i][j] = q_i . k_j over the head's 256 features: wave w owns 128 features of head w / 2 (S2R: 32 of the one head), two tiles at a time
    constexpr int QT = 2, QC = S2R ? 1 : 4;
    float sc[2][2] = {{0, 0}, {0, 0}};
#pragma unroll 1
    for (int c = 0; c < QC; ++c) {
        f32x4 q[QT][2], k[QT][2];
        zero_acc<QT, 2>(q);
        gemm_tiles<QT, 2, true>(P.mq, (wave * QC + c) * QT, tok, ENC_YS, q);
        zero_acc<QT, 2>(k);
        gemm_tiles<QT, 2, true>(P.mk, (wave * QC + c) * QT, tok, ENC_YS, k);
#pragma unroll
        for (int mt = 0; mt < QT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) sc[i][j] += q[mt][i][r] * k[mt][j][r];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float t = lane_groups_sum(sc[i][j]);
            if (lane < 16) red_s[(wave * 4 + i * 2 + j) * 16 + lane] = t;
        }
    __syncthreads();
    // lanes 0..15 of a head's even wave (S2R: of wave 0) own that head's [2][2] of agent a0 + lane
    const int ga = a0 + lane;
    if (lane < 16 && ga < B && (S2R ? wave == 0 : (wave & 1) == 0)) {
        float *w = weights + (size_t)ga * (S2R ? 4 : 16) + (S2R ? 0 : (wave >> 1) * 4);
#pragma unroll
        for (int i = 0; i < 2; ++i) {   // softmax over the keys j of (q_i / sqrt(d_k)) . k_j   (attention_layer.py:118-125)
            float t[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float acc_s = 0.0f;
                if constexpr (S2R) {
#pragma unroll
                    for (int v = 0; v < ENC_WAVES; ++v) acc_s += red_s[(v * 4 + i * 2 + j) * 16 + lane];
                } else
                    acc_s = red_s[(wave * 4 + i * 2 + j) * 16 + lane] + red_s[((wave | 1) * 4 + i * 2 + j) * 16 + lane];
                t[j] = acc_s * (1.0f / 16.0f);
            }
            const float m = fmaxf(t[0], t[1]), e0 = __expf(t[0] - m), e1 = __expf(t[1] - m), den = e0 + e1;
            w[i * 2 + 0] = e0 / den;
            w[i * 2 + 1] = e1 / den;
        }
    }
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_attn_mha_kernel(const float *__restrict__ obs, int B, EncParams P,
    float *__restrict__ weights) {
    attnw_mha_body<false>(obs, B, P, weights);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_attn_s2r_kernel(const float *__restrict__ obs, int B, EncParams P,
    float *__restrict__ weights) {
    attnw_mha_body<true>(obs, B, P, weights);
}

// ------------------------------------------------------------------------------------------------
// the Sim2Real encoder at rnn_size 16 / 32 / 64: narrow_body up to the softmax, one wave per 16 agents
// ------------------------------------------------------------------------------------------------
template <int NH, int WAVES>
__device__ __forceinline__ void attnw_narrow_body(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ weights) {
    constexpr int KSH = (NH + 1) / 2;
    __shared__ __align__(16) uint16_t lds[WAVES * 2 * ENC_NW_PLANE];
    const int wave = wave_id(), lane = threadIdx.x & 63, g = lane >> 4;
    const int a0 = blockIdx.x * (ENC_NW_AGENTS * WAVES) + ENC_NW_AGENTS * wave, ga = a0 + (lane & 15);
    uint16_t *const slice = lds + wave * 2 * ENC_NW_PLANE;
    if (a0 >= B) return;   // a wave behind the batch: nobody waits for it
    const bool ok = ga < B;
    const int nbw = P.nbr_dim * P.num_nbr;
    const uint32_t row = (uint32_t)ga * (uint32_t)P.obs_dim;
    const __amdgpu_buffer_rsrc_t rs = obs_rsrc(obs, B, P.obs_dim);
    f32x4 tk[2][NH];   // tokens: all neighbour columns -> 0, obstacle columns -> 1   (:226-234)
    {
        const NwFrag xn[2] = {nw_obs_frag(rs, ok, row + P.self_dim, nbw, 8 * g), nw_obs_frag(rs, ok, row + P.self_dim, nbw, 32 + 8 * g)};
        const NwFrag xo[1] = {nw_obs_frag(rs, ok, row + P.self_dim + nbw, P.obst_dim, 8 * g)};
        nw_bias<NH>(P.n1, tk[0]);
        nw_gemm<NH, 2>(P.n1, xn, tk[0]);
        nw_bias<NH>(P.o1, tk[1]);
        nw_gemm<NH, 1>(P.o1, xo, tk[1]);
        nw_tanh<NH>(tk[0]);
        nw_tanh<NH>(tk[1]);
    }
    f32x4 q[2][NH], k[2][NH];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        NwFrag tb[KSH];
        nw_as_operand<NH>(slice, tk[i], tb);
        nw_zero<NH>(q[i]);
        nw_gemm<NH, KSH>(P.mq, tb, q[i]);
        nw_zero<NH>(k[i]);
        nw_gemm<NH, KSH>(P.mk, tb, k[i]);
    }
    constexpr float scale = NH == 1 ? 0.25f : NH == 2 ? 0.17677669529663687f : 0.125f;   // 1 / sqrt(H)   (attention_layer.py:82)
    float pr[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float t[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int mt = 0; mt < NH; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) s += q[i][mt][r] * k[j][mt][r];
            t[j] = lane_groups_sum(s) * scale;
        }
        const float m = fmaxf(t[0], t[1]), e0 = __expf(t[0] - m), e1 = __expf(t[1] - m), den = e0 + e1;
        pr[i][0] = e0 / den;
        pr[i][1] = e1 / den;
    }
    if (ok && g == 0) {   // (every lane group of the agent holds the same four numbers: group 0 stores them)
        float *w = weights + (size_t)ga * 4;
        w[0] = pr[0][0]; w[1] = pr[0][1]; w[2] = pr[1][0]; w[3] = pr[1][1];
    }
}
#define ATTNW_NARROW_KERNEL(NH, H)                                                                                                       \
    extern "C" __global__ void __launch_bounds__(64 * ENC_NW_WAVES) qs_attn_narrow##H##_kernel(const float *__restrict__ obs, int B,    \
        EncParams P, float *__restrict__ weights) {                                                                                      \
        attnw_narrow_body<NH, ENC_NW_WAVES>(obs, B, P, weights);                                                                         \
    }
ATTNW_NARROW_KERNEL(1, 16) ATTNW_NARROW_KERNEL(2, 32) ATTNW_NARROW_KERNEL(4, 64)
#undef ATTNW_NARROW_KERNEL

// ------------------------------------------------------------------------------------------------
// C ABI (include/quadswarm_attention.h)
// ------------------------------------------------------------------------------------------------
// the kernels with dynamic LDS above 64 KiB, once: what the attribute loop and the launches below index
struct AttnwKernel { const void *fn; int lds_bytes; };
enum { ATTNW_K_EMBED, ATTNW_K_SCORES, ATTNW_K_MHA, ATTNW_K_S2R, ATTNW_NUM_KERNELS };
static const AttnwKernel attnw_kernels[ATTNW_NUM_KERNELS] = {
    {(const void *)qs_encoder_embed_split_kernel, EncLdsSplit::bytes},   // launch 1 of the attention encoder's forward pass, as it is
    {(const void *)qs_attn_scores_kernel, EncLdsAttnW::bytes},
    {(const void *)qs_attn_mha_kernel, EncLdsSplit::bytes},
    {(const void *)qs_attn_s2r_kernel, EncLdsSplit::bytes},
};

static int attnw_fail(const char *fn, int code, const char *what) { g_enc_error = std::string(fn) + ": " + what; return code; }

// the model, the precision and the shape: elements of a row, or -4.  No pointer inside `P` is looked at.
static int attnw_check_shape(const char *fn, const qs_enc_params &P) {
    const int m = P.nbr_encoder;
    if (m != QS_ENC_NBR_ATTENTION && m != QS_ENC_MODEL_MHA && m != QS_ENC_MODEL_S2R)
        return attnw_fail(fn, -4, "this encoder has no attention (mean_embed, mlp, no_encoder); the attention neighbour encoder and the two multi-head classes have");
    if (m == QS_ENC_NBR_ATTENTION && P.num_nbr == 0) return attnw_fail(fn, -4, "the attention neighbour encoder without neighbours computes no weights");
    if (P.precision != 1) return attnw_fail(fn, -4, "attention weights are computed in reference precision only (precision = 1, fp16-pair packing)");
    const bool mha = m != QS_ENC_NBR_ATTENTION;
    if (P.num_nbr < 1 || P.num_nbr > ENC_MAX_NBR || P.self_dim < 0 || P.self_dim > 32 || P.obst_dim < 0 || P.obst_dim > 32 || P.nbr_dim < 1 || P.nbr_dim > 32 ||
        (!mha && P.self_dim + P.nbr_dim > 32) || (mha && (P.nbr_dim * P.num_nbr > 64 || P.obst_dim < 1)))
        return attnw_fail(fn, -4, "unsupported encoder shape (inputs wider than 32 - 64 for the multi-head classes' neighbour columns -, more than 8 neighbours, "
                                  "or a multi-head class without neighbour or obstacle columns)");
    if (P.obs_dim < P.self_dim + P.nbr_dim * P.num_nbr + (mha ? P.obst_dim : 0)) return attnw_fail(fn, -4, "obs_dim is smaller than the columns the encoder reads");
    // the layers read have the packed sizes the kernels walk (a bias is read M floats long, an input row K columns wide)
    auto is = [](const qs_enc_layer &L, int M, int K) { return L.M == M && L.K == K; };
    const char *sizes = "a layer the weights depend on does not have the packed size of its place (M = width, K = ceil32 of its input)";
    if (!mha) {
        if (!is(P.n1, ENC_H, 32) || !is(P.n2, ENC_H, ENC_H) || !is(P.a1e, ENC_H, ENC_H) || !is(P.a1m, ENC_H, ENC_H) || !is(P.a2, ENC_H, ENC_H))
            return attnw_fail(fn, -4, sizes);
        return P.num_nbr;
    }
    const int kn = enc_narrow_ceil32(P.nbr_dim * P.num_nbr);
    if (m == QS_ENC_MODEL_MHA) {
        if (!is(P.n1, ENC_H, kn) || !is(P.n2, ENC_H, ENC_H) || !is(P.o1, ENC_H, 32) || !is(P.o2, ENC_H, ENC_H) || !is(P.mq, 4 * ENC_H, ENC_H) ||
            !is(P.mk, 4 * ENC_H, ENC_H))
            return attnw_fail(fn, -4, sizes);
        return 16;
    }
    const int H = P.n1.M;   // the width is the neighbour embedding's: the self encoder is not read here
    if (H != ENC_H && !enc_narrow_width(H)) return attnw_fail(fn, -4, "the Sim2Real encoder is built for rnn_size 16, 32, 64 and 256");
    if (!is(P.n1, H, kn) || !is(P.o1, H, 32) || !is(P.mq, H, enc_narrow_ceil32(H)) || !is(P.mk, H, enc_narrow_ceil32(H)))
        return attnw_fail(fn, -4, H == ENC_H ? sizes : "narrow Sim2Real encoder: n1, o1, mq, mk have M = rnn_size, mq and mk K = ceil32(rnn_size)");
    return 4;
}

extern "C" {

int32_t qs_attn_row_elems(const qs_enc_params *params) {
    const char *fn = "qs_attn_row_elems";
    if (!params) return attnw_fail(fn, -1, "NULL parameter struct");
    return attnw_check_shape(fn, *params);
}

int qs_attn_weights(const float *obs, int32_t B, const qs_enc_params *params, float *weights, void *stream) {
    const char *fn = "qs_attn_weights";
    if (!obs || !params || !weights) return attnw_fail(fn, -1, "obs, params and weights must not be NULL");
    if (B < 1) return attnw_fail(fn, -1, "B must be at least 1");
    const qs_enc_params &P = *params;
    const int elems = attnw_check_shape(fn, P);
    if (elems < 0) return elems;
    // a copy with the fields the weights depend on and nothing else: no head, no sampling, no trajectory copy reaches a kernel
    qs_enc_params Q = {};
    Q.self_dim = P.self_dim; Q.nbr_dim = P.nbr_dim; Q.num_nbr = P.num_nbr; Q.obst_dim = P.obst_dim; Q.obs_dim = P.obs_dim;
    Q.nbr_encoder = P.nbr_encoder; Q.precision = 1;
    const bool att = P.nbr_encoder == QS_ENC_NBR_ATTENTION, s2r = P.nbr_encoder == QS_ENC_MODEL_S2R;
    bool missing;
    if (att) {
        Q.n1 = P.n1; Q.n2 = P.n2; Q.a1e = P.a1e; Q.a1m = P.a1m; Q.a2 = P.a2; Q.a3w = P.a3w; Q.a3b = P.a3b; Q.ebuf = P.ebuf; Q.gbuf = P.gbuf;
        missing = !P.n1.w || !P.n1.b || !P.n2.w || !P.n2.b || !P.a1e.w || !P.a1e.b || !P.a1m.w || !P.a2.w || !P.a2.b || !P.a3w;
        if (!missing && (!P.ebuf || !P.gbuf)) return attnw_fail(fn, -1, "the attention neighbour encoder needs the ebuf / gbuf scratch buffers");
    } else {
        Q.n1 = P.n1; Q.o1 = P.o1; Q.mq = P.mq; Q.mk = P.mk;
        missing = !P.n1.w || !P.n1.b || !P.o1.w || !P.o1.b || !P.mq.w || !P.mk.w;
        if (!s2r) { Q.n2 = P.n2; Q.o2 = P.o2; missing = missing || !P.n2.w || !P.n2.b || !P.o2.w || !P.o2.b; }
    }
    if (missing) return attnw_fail(fn, -1, "a weight or bias pointer of a layer the weights depend on is NULL");
    if (att && (int64_t)B * P.num_nbr * (ENC_H * 2) * 2 > 0x7fffffffll) return attnw_fail(fn, -4, "attention: batch x neighbours too large for 32-bit scratch offsets");
    if ((int64_t)B * P.obs_dim * 4 > 0xffffffffll) return attnw_fail(fn, -4, "batch x obs_dim too large for 32-bit observation offsets");

    int dev = 0;   // launch on the device that owns `obs`, as qs_enc_forward does
    {
        hipPointerAttribute_t pa;
        if (hipPointerGetAttributes(&pa, obs) == hipSuccess) dev = pa.device; else { (void)hipGetLastError(); (void)hipGetDevice(&dev); }
        if (hipSetDevice(dev) != hipSuccess) return attnw_fail(fn, -2, "hipSetDevice failed");
    }
    void *args[] = {&obs, &B, (void *)&Q, &weights};
    if (s2r && P.n1.M != ENC_H) {   // static LDS, far below 64 KiB: no attribute to raise
        const int H = P.n1.M;
        const void *k = H == 16 ? (const void *)qs_attn_narrow16_kernel : H == 32 ? (const void *)qs_attn_narrow32_kernel : (const void *)qs_attn_narrow64_kernel;
        (void)hipLaunchKernel(k, dim3(enc_narrow_grid(B, ENC_NW_WAVES)), dim3(64 * ENC_NW_WAVES), args, 0, (hipStream_t)stream);
    } else {
        {
            static std::mutex attr_mutex;
            static uint64_t attr_set = 0;   // bit d: attributes set on device d
            std::lock_guard<std::mutex> lock(attr_mutex);
            if (dev < 0 || dev >= 64) return attnw_fail(fn, -2, "device index out of range");
            if (!(attr_set >> dev & 1)) {
                for (const AttnwKernel &k : attnw_kernels)
                    if (hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes) != hipSuccess)
                        return attnw_fail(fn, -2, "cannot raise the dynamic LDS limit");
                attr_set |= 1ull << dev;
            }
        }
        const dim3 grid((B + ENC_TA - 1) / ENC_TA), block(64 * ENC_WAVES);
        if (att) {
            void *embed_args[] = {&obs, &B, (void *)&Q};
            (void)hipLaunchKernel(attnw_kernels[ATTNW_K_EMBED].fn, grid, block, embed_args, attnw_kernels[ATTNW_K_EMBED].lds_bytes, (hipStream_t)stream);
        }
        const AttnwKernel &k = attnw_kernels[att ? ATTNW_K_SCORES : s2r ? ATTNW_K_S2R : ATTNW_K_MHA];
        (void)hipLaunchKernel(k.fn, grid, block, args, k.lds_bytes, (hipStream_t)stream);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return attnw_fail(fn, -2, hipGetErrorString(e));
    return 0;
}

}

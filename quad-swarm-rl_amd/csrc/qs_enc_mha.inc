// ------------------------------------------------------------------------------------------------
// QuadMultiHeadAttentionEncoder (:124-196, --quads_encoder_type=attention): self / neighbour / obstacle MLPs, 4-head scaled
// dot-product attention over the token pair [neighbour embedding, obstacle embedding] (attention_layer.py:12-56: projections
// without bias, q / sqrt(d_k), softmax over the keys, output projection, residual, LayerNorm eps 1e-6), feed-forward.
// Wave w owns features [128w, 128w+128) of the 1024-wide projections = half of head w/2, in two chunks of 4 feature tiles:
// the 2x2 scores of a head are sums over its features, so they accumulate chunk by chunk and only one chunk of q, k is live;
// lane groups are reduced with two shuffles, the two waves of a head and (for LayerNorm) the eight waves through LDS.
// ------------------------------------------------------------------------------------------------
template <int MT, int NT>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[MT][NT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0, 0, 0, 0};
}
// 16-row MLP like mlp2_one_tile, but the fp32 result also stays in registers (the attention block's residual)
template <bool SP = false>
__device__ __forceinline__ void mlp2_keep(const EncLayer &L1, const EncLayer &L2, int mt0, const uint16_t *X, int xstride, uint16_t *hid,
    uint16_t *Y,
                                          f32x4 (&keep)[ENC_MT]) {
    const int lane = threadIdx.x & 63;
    f32x4 acc[ENC_MT][1];
    init_bias<ENC_MT, 1>(L1, mt0, acc);
    gemm_tiles<ENC_MT, 1, SP>(L1, mt0, X, xstride, acc);
    store_tanh<ENC_MT, 1, SP>(acc, mt0, hid, ENC_YS);
    __syncthreads();
    init_bias<ENC_MT, 1>(L2, mt0, acc);
    gemm_tiles<ENC_MT, 1, SP>(L2, mt0, hid, ENC_YS, acc);
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) keep[mt][r] = fast_tanh(acc[mt][0][r]);
        put4<SP>(Y + (lane & 15) * ENC_YS + (mt0 + mt) * 16 + (lane >> 4) * 4, keep[mt]);
    }
}

// one-layer embedding of 16 rows: Y[:, col..] = tanh(L X); KEEP: the fp32 result also stays in registers (the attention block's residual)
template <bool KEEP, bool SP = false>
__device__ __forceinline__ void mlp1_keep(const EncLayer &L1, int mt0, const uint16_t *X, int xstride, uint16_t *Y, int ystride,
    f32x4 (&keep)[ENC_MT]) {
    const int lane = threadIdx.x & 63;
    f32x4 acc[ENC_MT][1];
    init_bias<ENC_MT, 1>(L1, mt0, acc);
    gemm_tiles<ENC_MT, 1, SP>(L1, mt0, X, xstride, acc);
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) {
        f32x4 t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            t[r] = fast_tanh(acc[mt][0][r]);
            if constexpr (KEEP) keep[mt][r] = t[r];
        }
        put4<SP>(Y + (lane & 15) * ystride + (mt0 + mt) * 16 + (lane >> 4) * 4, t);
    }
}

template <bool S2R>
__device__ __forceinline__ void mha_body(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsMha Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_self = lds + Lds::x_self, *x_obst = lds + Lds::x_obst, *x_nbr = lds + Lds::x_nbr;
    uint16_t *hid = lds + Lds::hid, *tok = lds + Lds::tok, *obuf = lds + Lds::obuf, *cat = lds + Lds::cat;
    float *red_s = (float *)(lds + Lds::red_s), *red_ln = (float *)(lds + Lds::red_ln);
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, a0 = blockIdx.x * ENC_TA;
    const int NB = P.num_nbr, D = P.obs_dim, mt0 = wave * ENC_MT, nbw = P.nbr_dim * NB;
    traj_copy(P, a0, ENC_TA, B);

    // columns as bf16, zero padded: [self 32 | obstacle 32 | neighbours 64]
    for (int idx = tid; idx < ENC_TA * 128; idx += 64 * ENC_WAVES) {
        const int a = idx >> 7, c = idx & 127, ga = a0 + a;
        int col = -1;
        uint16_t *dst;
        if (c < 32) { dst = x_self + a * ENC_XS + c; if (c < P.self_dim) col = c; }
        else if (c < 64) { dst = x_obst + a * ENC_XS + (c - 32); if (c - 32 < P.obst_dim) col = P.self_dim + nbw + (c - 32); }
        else { dst = x_nbr + a * ENC_XW + (c - 64); if (c - 64 < nbw) col = P.self_dim + (c - 64); }
        const float v = obs_at(obs_rsrc(obs, B, D), ga < B && col >= 0, (uint32_t)ga * (uint32_t)D + col);
        *dst = __builtin_bit_cast(uint16_t, (__bf16)v);
    }
    __syncthreads();
    f32x4 resid[2][ENC_MT];   // fp32 tokens: features of this wave, rows lane & 15
    if constexpr (S2R) {   // one layer per embedding (:229-240): nothing between them to wait for
        mlp1_keep<false>(P.s1, mt0, x_self, ENC_XS, cat, ENC_CS, resid[0]);
        mlp1_keep<true>(P.n1, mt0, x_nbr, ENC_XW, tok, ENC_YS, resid[0]);
        mlp1_keep<true>(P.o1, mt0, x_obst, ENC_XS, tok + ENC_TA * ENC_YS, ENC_YS, resid[1]);
    } else {
        mlp2_one_tile(P.s1, P.s2, mt0, x_self, ENC_XS, hid, cat, ENC_CS, 0);
        __syncthreads();
        mlp2_keep<>(P.n1, P.n2, mt0, x_nbr, ENC_XW, hid, tok, resid[0]);
        __syncthreads();
        mlp2_keep<>(P.o1, P.o2, mt0, x_obst, ENC_XS, hid, tok + ENC_TA * ENC_YS, resid[1]);
    }
    __syncthreads();

    // ---- scores: s[i][j] = q_i . k_j over the head's 256 features, accumulated over this wave's two chunks ----
    // (one head: wave w owns features [32w, 32w+32) of the 256-wide projections, one chunk of 2 feature tiles)
    constexpr int QT = S2R ? 2 : 4, QC = S2R ? 1 : 2;   // feature tiles per chunk, chunks per wave
    float sc[2][2] = {{0, 0}, {0, 0}};
#pragma unroll 1
    for (int c = 0; c < QC; ++c) {
        f32x4 q[QT][2], k[QT][2];
        zero_acc<QT, 2>(q);
        gemm_tiles<QT, 2>(P.mq, (wave * QC + c) * QT, tok, ENC_YS, q);
        zero_acc<QT, 2>(k);
        gemm_tiles<QT, 2>(P.mk, (wave * QC + c) * QT, tok, ENC_YS, k);
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
    float pr[2][2];   // softmax over the keys j of (q_i / sqrt(d_k)) . k_j   (attention_layer.py:118-125)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float t[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float acc_s = 0.0f;
            if constexpr (S2R) {   // one head over all eight waves   (attention_layer.py:83)
#pragma unroll
                for (int w = 0; w < ENC_WAVES; ++w) acc_s += red_s[(w * 4 + i * 2 + j) * 16 + (lane & 15)];
            } else
                acc_s = red_s[((wave & ~1) * 4 + i * 2 + j) * 16 + (lane & 15)] + red_s[((wave | 1) * 4 + i * 2 + j) * 16 + (lane & 15)];
            t[j] = acc_s * (1.0f / 16.0f);
        }
        const float m = fmaxf(t[0], t[1]), e0 = __expf(t[0] - m), e1 = __expf(t[1] - m), rd = 1.0f / (e0 + e1);
        pr[i][0] = e0 * rd;
        pr[i][1] = e1 * rd;
    }
    // ---- o_i = sum_j p_ij v_j -> obuf[i][row][head * 256 + feature] ----
#pragma unroll 1
    for (int c = 0; c < QC; ++c) {
        f32x4 v[QT][2];
        zero_acc<QT, 2>(v);
        gemm_tiles<QT, 2>(P.mv, (wave * QC + c) * QT, tok, ENC_YS, v);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int mt = 0; mt < QT; ++mt) {
                bf16x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (__bf16)(pr[i][0] * v[mt][0][r] + pr[i][1] * v[mt][1][r]);
                *(bf16x4 *)(obuf + (i * ENC_TA + (lane & 15)) * ENC_OS + ((wave * QC + c) * QT + mt) * 16 + (lane >> 4) * 4) = o;
            }
    }
    __syncthreads();
    // ---- fc, residual, LayerNorm -> cat[:, 256 + token * 256 + feature]   (attention_layer.py:47-54) ----
    f32x4 y[ENC_MT][2];
    zero_acc<ENC_MT, 2>(y);
    gemm_tiles<ENC_MT, 2>(P.mfc, mt0, obuf, ENC_OS, y);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                y[mt][i][r] += resid[i][mt][r];
                s1 += y[mt][i][r];
                s2 += y[mt][i][r] * y[mt][i][r];
            }
        s1 = lane_groups_sum(s1);
        s2 = lane_groups_sum(s2);
        if (lane < 16) {
            red_ln[((wave * 2 + i) * 2 + 0) * 16 + lane] = s1;
            red_ln[((wave * 2 + i) * 2 + 1) * 16 + lane] = s2;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int w = 0; w < ENC_WAVES; ++w) {
            s1 += red_ln[((w * 2 + i) * 2 + 0) * 16 + (lane & 15)];
            s2 += red_ln[((w * 2 + i) * 2 + 1) * 16 + (lane & 15)];
        }
        const float mean = s1 * (1.0f / ENC_H), var = fmaxf(s2 * (1.0f / ENC_H) - mean * mean, 0.0f),
            rstd = __builtin_amdgcn_rsqf(var + 1e-6f);
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) {
            const int f0 = (mt0 + mt) * 16 + (lane >> 4) * 4;
            const f32x4 g = *(const f32x4 *)(P.ln_w + f0), bb = *(const f32x4 *)(P.ln_b + f0);
            bf16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (__bf16)((y[mt][i][r] - mean) * rstd * g[r] + bb[r]);
            *(bf16x4 *)(cat + (lane & 15) * ENC_CS + ENC_H * (1 + i) + f0) = o;
        }
    }
    __syncthreads();
    feed_forward<S2R ? ENC_MTF / 2 : ENC_MTF>(P, cat, a0, B, out, (float *)hid);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_mha_kernel(const float *__restrict__ obs, int B, EncParams P,
    float *__restrict__ out) {
    mha_body<false>(obs, B, P, out);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_s2r_kernel(const float *__restrict__ obs, int B, EncParams P,
    float *__restrict__ out) {
    mha_body<true>(obs, B, P, out);
}

// The same block in reference precision (fp16 pairs, see split2).  Two LDS planes leave room for ONE token's concatenated heads, so the
// value projection, the weighted sum and the output projection run per query token (the value GEMM twice).  Layout: EncLdsMhaSplit.
template <bool S2R>
__device__ __forceinline__ void mha_body_split(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsMhaSplit Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_self = lds + Lds::x_self, *x_obst = lds + Lds::x_obst, *x_nbr = lds + Lds::x_nbr;
    uint16_t *hid = lds + Lds::hid, *tok = lds + Lds::tok, *obuf = lds + Lds::obuf, *cat = lds + Lds::cat;
    float *red_s = (float *)(lds + Lds::red_s), *red_ln = (float *)(lds + Lds::red_ln);
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, a0 = blockIdx.x * ENC_TA;
    const int NB = P.num_nbr, D = P.obs_dim, mt0 = wave * ENC_MT, nbw = P.nbr_dim * NB;
    traj_copy(P, a0, ENC_TA, B);
    for (int idx = tid; idx < ENC_TA * 128; idx += 64 * ENC_WAVES) {
        const int a = idx >> 7, c = idx & 127, ga = a0 + a;
        int col = -1;
        uint16_t *dst;
        if (c < 32) { dst = x_self + a * ENC_XS + c; if (c < P.self_dim) col = c; }
        else if (c < 64) { dst = x_obst + a * ENC_XS + (c - 32); if (c - 32 < P.obst_dim) col = P.self_dim + nbw + (c - 32); }
        else { dst = x_nbr + a * ENC_XW + (c - 64); if (c - 64 < nbw) col = P.self_dim + (c - 64); }
        put1<true>(dst, obs_at(obs_rsrc(obs, B, D), ga < B && col >= 0, (uint32_t)ga * (uint32_t)D + col));
    }
    __syncthreads();
    f32x4 resid[2][ENC_MT];
    if constexpr (S2R) {
        mlp1_keep<false, true>(P.s1, mt0, x_self, ENC_XS, cat, ENC_CS, resid[0]);
        mlp1_keep<true, true>(P.n1, mt0, x_nbr, ENC_XW, tok, ENC_YS, resid[0]);
        mlp1_keep<true, true>(P.o1, mt0, x_obst, ENC_XS, tok + ENC_TA * ENC_YS, ENC_YS, resid[1]);
    } else {
        mlp2_one_tile<true>(P.s1, P.s2, mt0, x_self, ENC_XS, hid, cat, ENC_CS, 0);
        __syncthreads();
        mlp2_keep<true>(P.n1, P.n2, mt0, x_nbr, ENC_XW, hid, tok, resid[0]);
        __syncthreads();
        mlp2_keep<true>(P.o1, P.o2, mt0, x_obst, ENC_XS, hid, tok + ENC_TA * ENC_YS, resid[1]);
    }
    __syncthreads();
    constexpr int QT = 2, QC = S2R ? 1 : 4;   // (two feature tiles per chunk: the fp16-pair GEMM holds two weight rings and two accumulator sets)
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
    __syncthreads();   // (also: every wave is done with the inputs and `hid`, obuf may be written)
    float pr[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float t[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float acc_s = 0.0f;
            if constexpr (S2R) {
#pragma unroll
                for (int w = 0; w < ENC_WAVES; ++w) acc_s += red_s[(w * 4 + i * 2 + j) * 16 + (lane & 15)];
            } else
                acc_s = red_s[((wave & ~1) * 4 + i * 2 + j) * 16 + (lane & 15)] + red_s[((wave | 1) * 4 + i * 2 + j) * 16 + (lane & 15)];
            t[j] = acc_s * (1.0f / 16.0f);
        }
        const float m = fmaxf(t[0], t[1]), e0 = __expf(t[0] - m), e1 = __expf(t[1] - m), rd = 1.0f / (e0 + e1);
        pr[i][0] = e0 * rd;
        pr[i][1] = e1 * rd;
    }
    f32x4 y[ENC_MT][2];
#pragma unroll 1
    for (int i = 0; i < 2; ++i) {   // per query token: o_i = sum_j p_ij v_j -> obuf, then fc + residual -> y[.][i]
        const float p0 = i == 0 ? pr[0][0] : pr[1][0], p1 = i == 0 ? pr[0][1] : pr[1][1];
#pragma unroll 1
        for (int c = 0; c < QC; ++c) {
            f32x4 v[QT][2];
            zero_acc<QT, 2>(v);
            gemm_tiles<QT, 2, true>(P.mv, (wave * QC + c) * QT, tok, ENC_YS, v);
#pragma unroll
            for (int mt = 0; mt < QT; ++mt) {
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = p0 * v[mt][0][r] + p1 * v[mt][1][r];
                put4<true>(obuf + (lane & 15) * ENC_OS + ((wave * QC + c) * QT + mt) * 16 + (lane >> 4) * 4, o);
            }
        }
        __syncthreads();
        f32x4 yi[ENC_MT][1];
        zero_acc<ENC_MT, 1>(yi);
        gemm_tiles<ENC_MT, 1, true>(P.mfc, mt0, obuf, ENC_OS, yi);
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float t = yi[mt][0][r] + (i == 0 ? resid[0][mt][r] : resid[1][mt][r]);
                if (i == 0) y[mt][0][r] = t; else y[mt][1][r] = t;
                s1 += t;
                s2 += t * t;
            }
        s1 = lane_groups_sum(s1);
        s2 = lane_groups_sum(s2);
        if (lane < 16) {
            red_ln[((wave * 2 + i) * 2 + 0) * 16 + lane] = s1;
            red_ln[((wave * 2 + i) * 2 + 1) * 16 + lane] = s2;
        }
        __syncthreads();   // every wave has read this token's obuf; the sums are visible
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int w = 0; w < ENC_WAVES; ++w) {
            s1 += red_ln[((w * 2 + i) * 2 + 0) * 16 + (lane & 15)];
            s2 += red_ln[((w * 2 + i) * 2 + 1) * 16 + (lane & 15)];
        }
        const float mean = s1 * (1.0f / ENC_H), var = fmaxf(s2 * (1.0f / ENC_H) - mean * mean, 0.0f), rstd = 1.0f / __builtin_sqrtf(var + 1e-6f);
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) {
            const int f0 = (mt0 + mt) * 16 + (lane >> 4) * 4;
            const f32x4 g = *(const f32x4 *)(P.ln_w + f0), bb = *(const f32x4 *)(P.ln_b + f0);
            f32x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (y[mt][i][r] - mean) * rstd * g[r] + bb[r];
            put4<true>(cat + (lane & 15) * ENC_CS + ENC_H * (1 + i) + f0, o);
        }
    }
    __syncthreads();
    feed_forward<S2R ? ENC_MTF / 2 : ENC_MTF, true>(P, cat, a0, B, out, (float *)hid);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_mha_split_kernel(const float *__restrict__ obs, int B, EncParams P,
    float *__restrict__ out) {
    mha_body_split<false>(obs, B, P, out);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_s2r_split_kernel(const float *__restrict__ obs, int B, EncParams P,
    float *__restrict__ out) {
    mha_body_split<true>(obs, B, P, out);
}

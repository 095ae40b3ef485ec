// ------------------------------------------------------------------------------------------------
// attention, launch 1: e_i = embedding_mlp([self_obs[(a*K+k) mod B] | neighbour obs (a,k)]) -> ebuf;  g_a = W_m mean_k e_(a,k) -> gbuf
// ------------------------------------------------------------------------------------------------
template <int NTH, bool SP = false>
__device__ __forceinline__ void embed_pass(const EncParams &P, int B, int a0, int t0, bool first, const uint16_t *x_in, uint16_t *buf_a,
    f32x4 (&mean)[ENC_MT]) {
    const int wave = wave_id(), lane = threadIdx.x & 63, mt0 = wave * ENC_MT, NB = P.num_nbr;
    f32x4 acc[ENC_MT][NTH];
    init_bias<ENC_MT, NTH>(P.n1, mt0, acc);
    gemm_tiles<ENC_MT, NTH, SP>(P.n1, mt0, x_in + t0 * ENC_TA * ENC_XS, ENC_XS, acc);
    if (!first) __syncthreads();   // the previous pass is done reading buf_a
    store_tanh<ENC_MT, NTH, SP>(acc, mt0, buf_a, ENC_YS);
    __syncthreads();
    init_bias<ENC_MT, NTH>(P.n2, mt0, acc);
    gemm_tiles<ENC_MT, NTH, SP>(P.n2, mt0, buf_a, ENC_YS, acc);
    const int ga = a0 + (lane & 15);
    constexpr int ES = SP ? 2 * ENC_H : ENC_H;   // ebuf row: bf16 [256], or the two fp16 planes [2][256]
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTH; ++nt) {
            f32x4 e;
#pragma unroll
            for (int r = 0; r < 4; ++r) { e[r] = fast_tanh(acc[mt][nt][r]); mean[mt][r] += e[r]; }
            if (ga < B) put4<SP>(P.ebuf + ((size_t)ga * NB + (t0 + nt)) * ES + (mt0 + mt) * 16 + (lane >> 4) * 4, e, ENC_H);
        }
}

template <bool SP>
__device__ __forceinline__ void embed_body(const float *__restrict__ obs, int B, const EncParams &P) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsEmbed Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_in = lds + Lds::x_in, *buf_a = lds + Lds::buf_a, *emean = lds + Lds::emean;
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, a0 = blockIdx.x * ENC_TA;
    const int NB = P.num_nbr, D = P.obs_dim, mt0 = wave * ENC_MT;
    const float invB = 1.0f / (float)B;
    traj_copy(P, a0, ENC_TA, B);
    const __amdgpu_buffer_rsrc_t ors = obs_rsrc(obs, B, D);
#pragma unroll 4
    for (int idx = tid; idx < NB * ENC_TA * 32; idx += 64 * ENC_WAVES) {
        const int row = idx >> 5, c = idx & 31, k = row >> 4, a = row & 15, ga = a0 + a;
        // self_obs.repeat(K, 1)  (:84)
        const uint32_t i_self = mod_batch((uint32_t)ga * (uint32_t)NB + (uint32_t)k, (uint32_t)B, invB) * (uint32_t)D + c;
        const uint32_t i_nbr = (uint32_t)ga * (uint32_t)D + P.self_dim + k * P.nbr_dim + (c - P.self_dim);
        const float v = obs_at(ors, ga < B && c < P.self_dim + P.nbr_dim, c < P.self_dim ? i_self : i_nbr);
        put1<SP>(x_in + row * ENC_XS + c, v);
    }
    __syncthreads();
    f32x4 mean[ENC_MT];
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) mean[mt] = (f32x4){0, 0, 0, 0};
    for (int t0 = 0; t0 < NB; t0 += ENC_NH) {
#define ENC_CALL(n) embed_pass<n, SP>(P, B, a0, t0, t0 == 0, x_in, buf_a, mean)
        ENC_DISPATCH_NT(NB - t0, ENC_NH, ENC_CALL)
#undef ENC_CALL
    }
    const float inv = 1.0f / (float)NB;   // e_mean (:90-91), then its half of the score MLP's first layer once per agent
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = mean[mt][r] * inv;
        put4<SP>(emean + (lane & 15) * ENC_YS + (mt0 + mt) * 16 + (lane >> 4) * 4, v);
    }
    __syncthreads();
    f32x4 g[ENC_MT][1];
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) g[mt][0] = (f32x4){0, 0, 0, 0};
    gemm_tiles<ENC_MT, 1, SP>(P.a1m, mt0, emean, ENC_YS, g);
    const int ga = a0 + (lane & 15);
    if (ga < B) {
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) *(f32x4 *)(P.gbuf + (size_t)ga * ENC_H + (mt0 + mt) * 16 + (lane >> 4) * 4) = g[mt][0];
    }
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, ENC_OCC) qs_encoder_embed_kernel(const float *__restrict__ obs, int B,
    EncParams P) {
    embed_body<false>(obs, B, P);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_embed_split_kernel(const float *__restrict__ obs, int B,
    EncParams P) {
    embed_body<true>(obs, B, P);
}

// ------------------------------------------------------------------------------------------------
// attention, launch 2 (:88-101): value MLP, score MLP, softmax over the neighbours, weighted sum; then self / obstacle encoders
// and the feed-forward layer.  One sweep over the neighbour row tiles in groups of ENC_ANH with an online softmax (running
// maximum and denominator per agent, the partial sum rescaled when the maximum moves), so that the h_i of earlier groups do not
// have to be kept: 78 KB of LDS and <= 128 VGPRs, two workgroups per CU.
// ------------------------------------------------------------------------------------------------
struct AttnState { f32x4 o[ENC_MT]; float mx, den; };

template <int NTH, bool SP = false>
__device__ __forceinline__ void attn_load_e(const EncParams &P, int B, int a0, int t0, uint16_t *buf_a) {
    // e_i rows in 16-byte chunks, coalesced; 32-bit offsets into a buffer resource (rows past the batch read as zero: out of range)
    constexpr int PL = SP ? 2 : 1;   // reference precision: a row of ebuf is the two fp16 planes [2][256]
    const __amdgpu_buffer_rsrc_t ers = __builtin_amdgcn_make_buffer_rsrc((void *)P.ebuf, 0,
        (uint32_t)B * (uint32_t)P.num_nbr * (ENC_H * 2 * PL), 0x00020000);
    for (int idx = threadIdx.x; idx < NTH * ENC_TA * (ENC_H / 8) * PL; idx += 64 * ENC_WAVES) {
        const int row = idx / (32 * PL), pl = (idx >> 5) & (PL - 1), ch = idx & 31, k = t0 + (row >> 4), ra = a0 + (row & 15);
        const uint32_t off = ra < B ? (((uint32_t)ra * (uint32_t)P.num_nbr + (uint32_t)k) * PL + pl) * (ENC_H * 2) + ch * 16 : 0xffffffffu;
        *(bf16x8 *)(buf_a + pl * ENC_SPLANE + row * ENC_YS + ch * 8) = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ers, off, 0, 0));
    }
}

// One group of NTH neighbour row tiles: scores first (the 256 -> 1 layer is reduced from the accumulators of the layer before it),
// then the values from the same e_i tile, which go straight into the running sum - the h_i are never live together with another
// layer's accumulators.  Four barriers per group.
template <int NTH, bool SP = false>
__device__ __forceinline__ void attn_pass(const EncParams &P, int B, int a0, int t0, uint16_t *buf_a, uint16_t *buf_h, float *s_alpha,
    AttnState &st) {
    const int wave = wave_id(), lane = threadIdx.x & 63, mt0 = wave * ENC_MT;
    const int ga = a0 + (lane & 15);
    attn_load_e<NTH, SP>(P, B, a0, t0, buf_a);
    f32x4 acc[ENC_MT][NTH];
    // score MLP, first layer on [e_i | e_mean.repeat(K, 1)]: W_e e_i + b + g[(a*K + k) mod B]   (:92-94)
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
    __syncthreads();   // e_i is in buf_a; the previous group's value layers are done with buf_h
    gemm_tiles<ENC_MT, NTH, SP>(P.a1e, mt0, buf_a, ENC_YS, acc);
    store_tanh<ENC_MT, NTH, SP>(acc, mt0, buf_h, ENC_YS);
    __syncthreads();
    init_bias<ENC_MT, NTH>(P.a2, mt0, acc);
    gemm_tiles<ENC_MT, NTH, SP>(P.a2, mt0, buf_h, ENC_YS, acc);
    // last score layer 256 -> 1 straight from the accumulators: per-lane partial dot product with the fp32 weight row, two shuffles
    // over the lane groups, the eight waves' partials through LDS - no activation store, no extra MFMA pass, and e_i stays in buf_a
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
    __syncthreads();   // partial scores visible; every wave is done reading buf_h (second score layer)
    // h_i = neighbor_value_mlp(e_i)   (:88)
    init_bias<ENC_MT, NTH>(P.v1, mt0, acc);
    gemm_tiles<ENC_MT, NTH, SP>(P.v1, mt0, buf_a, ENC_YS, acc);
    store_tanh<ENC_MT, NTH, SP>(acc, mt0, buf_h, ENC_YS);
    __syncthreads();
    init_bias<ENC_MT, NTH>(P.v2, mt0, acc);
    gemm_tiles<ENC_MT, NTH, SP>(P.v2, mt0, buf_h, ENC_YS, acc);
    // online softmax over the neighbours of agent (lane & 15)   (:95-100)
    float al[NTH], mx = st.mx;
#pragma unroll
    for (int nt = 0; nt < NTH; ++nt) {
        al[nt] = P.a3b;
#pragma unroll
        for (int w = 0; w < ENC_WAVES; ++w) al[nt] += s_alpha[(w * ENC_ANH + nt) * 16 + (lane & 15)];
        mx = fmaxf(mx, al[nt]);
    }
    const float scale = __expf(st.mx - mx);
    st.den *= scale;
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) st.o[mt][r] *= scale;
#pragma unroll
    for (int nt = 0; nt < NTH; ++nt) {
        const float e = __expf(al[nt] - mx);
        st.den += e;
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) st.o[mt][r] += e * fast_tanh(acc[mt][nt][r]);
    }
    st.mx = mx;
}

template <bool SP>
__device__ __forceinline__ void attn_body(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsAttn Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_self = lds + Lds::x_self, *x_obst = lds + Lds::x_obst, *buf_a = lds + Lds::buf_a;
    uint16_t *buf_h = lds + Lds::buf_h, *cat = lds + Lds::cat;
    float *s_alpha = (float *)(lds + (SP ? EncLdsSplit::s_alpha : Lds::s_alpha));   // reference precision: behind both planes
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, a0 = blockIdx.x * ENC_TA;
    const int NB = P.num_nbr, D = P.obs_dim, mt0 = wave * ENC_MT;
    const int col_nbr = ENC_H, col_obst = 2 * ENC_H;

    for (int idx = tid; idx < 2 * ENC_TA * 32; idx += 64 * ENC_WAVES) {   // self and obstacle columns as bf16, zero padded to K = 32
        const int which = idx >> 9, a = (idx >> 5) & 15, c = idx & 31, ga = a0 + a;
        const int dim = which ? P.obst_dim : P.self_dim, col = which ? P.self_dim + P.nbr_dim * NB : 0;
        const float v = obs_at(obs_rsrc(obs, B, D), ga < B && c < dim, (uint32_t)ga * (uint32_t)D + col + c);
        put1<SP>((which ? x_obst : x_self) + a * ENC_XS + c, v);
    }
    __syncthreads();
    mlp2_one_tile<SP>(P.s1, P.s2, mt0, x_self, ENC_XS, buf_h, cat, ENC_CS, 0);
    if (P.obst_dim > 0) {
        __syncthreads();
        mlp2_one_tile<SP>(P.o1, P.o2, mt0, x_obst, ENC_XS, buf_h, cat, ENC_CS, col_obst);
    }
    __syncthreads();

    AttnState st;
    st.mx = -3.0e38f; st.den = 0.0f;
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) st.o[mt] = (f32x4){0, 0, 0, 0};
    for (int t0 = 0; t0 < NB; t0 += ENC_ANH) {
#define ENC_CALL(n) attn_pass<n, SP>(P, B, a0, t0, buf_a, buf_h, s_alpha, st)
        ENC_DISPATCH_NT(NB - t0, ENC_ANH, ENC_CALL)
#undef ENC_CALL
    }
    const float rden = 1.0f / st.den;
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = st.o[mt][r] * rden;
        put4<SP>(cat + (lane & 15) * ENC_CS + col_nbr + (mt0 + mt) * 16 + (lane >> 4) * 4, v);
    }
    __syncthreads();
    feed_forward<ENC_MTF, SP>(P, cat, a0, B, out, (float *)buf_a);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, ENC_OCC) qs_encoder_attn_kernel(const float *__restrict__ obs, int B,
    EncParams P, float *__restrict__ out) {
    attn_body<false>(obs, B, P, out);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_attn_split_kernel(const float *__restrict__ obs, int B,
    EncParams P, float *__restrict__ out) {
    attn_body<true>(obs, B, P, out);
}

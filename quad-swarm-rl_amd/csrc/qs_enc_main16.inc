// ------------------------------------------------------------------------------------------------
// mean_embed / mlp / no_encoder: one launch
// ------------------------------------------------------------------------------------------------
template <int NTH, bool SP = false>
__device__ __forceinline__ void mean_pass(const EncParams &P, int t0, const uint16_t *x_nbr, uint16_t *buf_a, f32x4 (&mean)[ENC_MT]) {
    const int wave = wave_id(), mt0 = wave * ENC_MT;
    f32x4 acc[ENC_MT][NTH];
    init_bias<ENC_MT, NTH>(P.n1, mt0, acc);
    gemm_tiles<ENC_MT, NTH, SP>(P.n1, mt0, x_nbr + t0 * ENC_TA * ENC_XS, ENC_XS, acc);
    ENC_STAMP(4);
    if (t0) __syncthreads();   // the previous pass's second layer is done reading buf_a
    store_tanh<ENC_MT, NTH, SP>(acc, mt0, buf_a, ENC_YS);
    __syncthreads();
    ENC_STAMP(5);
    init_bias<ENC_MT, NTH>(P.n2, mt0, acc);
    gemm_tiles<ENC_MT, NTH, SP>(P.n2, mt0, buf_a, ENC_YS, acc);
    ENC_STAMP(6);
    // e_i = tanh(.); the mean over neighbours is a sum over the row tiles (same lane, same register)
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTH; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) mean[mt][r] += fast_tanh(acc[mt][nt][r]);
}

template <bool SP>
__device__ __forceinline__ void main_body(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsMain Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_self = lds + Lds::x_self, *x_nbr = lds + Lds::x_nbr, *x_obst = lds + Lds::x_obst;
    uint16_t *buf_a = lds + Lds::buf_a, *buf_b = lds + Lds::buf_b, *cat = lds + Lds::cat;

    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, a0 = blockIdx.x * ENC_TA;
    const int NB = P.num_nbr, D = P.obs_dim;
    const int mode = P.nbr_encoder;
    // no_encoder: the neighbour columns are in the row but nothing reads them (:289-291)
    const bool nbr_enc = NB > 0 && mode != QS_ENC_NBR_NONE;
    const int col_nbr = ENC_H, col_obst = ENC_H * (nbr_enc ? 2 : 1);   // column blocks of `cat` in the order of the reference's torch.cat
    const int mt0 = wave * ENC_MT;   // first of this wave's 16-feature tiles of a 256-wide layer

    ENC_STAMP(0);
    traj_copy(P, a0, ENC_TA, B);
    // ---- stage the observation rows as bf16, zero padded to K = 32 ----
    // The 16 rows of the workgroup are one contiguous block of obs: read it coalesced (every load issued before the first use),
    // then scatter each element to its slot of the self / neighbour / obstacle staging rows.
    {
        uint32_t *z = (uint32_t *)x_self;   // x_self, x_nbr, x_obst are contiguous: clear the padding first
        for (int idx = tid; idx < (2 + ENC_MAX_NBR) * ENC_TA * ENC_XS / 2; idx += 64 * ENC_WAVES) {
            z[idx] = 0;
            if constexpr (SP) z[ENC_SPLANE / 2 + idx] = 0;
        }
        // upper bound on elements per thread
        constexpr int PER = (ENC_TA * (32 + 32 * ENC_MAX_NBR + 32) + 64 * ENC_WAVES - 1) / (64 * ENC_WAVES);
        const int total = ENC_TA * D;
        const size_t first = (size_t)a0 * D;
        const __amdgpu_buffer_rsrc_t ors = obs_rsrc(obs, B, D);
        const uint32_t mD = div_magic(D), mN = div_magic(P.nbr_dim > 0 ? P.nbr_dim : 1);
        float v[PER];
#pragma unroll
        for (int it = 0; it < PER; ++it) {
            const int idx = tid + it * 64 * ENC_WAVES;
            v[it] = obs_at(ors, idx < total, (uint32_t)first + idx);   // rows past the batch: beyond the resource
        }
        __syncthreads();   // zeros are in place
#pragma unroll
        for (int it = 0; it < PER; ++it) {
            const int idx = tid + it * 64 * ENC_WAVES;
            if (idx < total) {
                const int a = div_by(idx, mD), cidx = idx - a * D;
                uint16_t *dst;
                if (cidx < P.self_dim) dst = x_self + a * ENC_XS + cidx;
                else if (cidx < P.self_dim + P.nbr_dim * NB) {
                    const int q = cidx - P.self_dim, nb = div_by(q, mN), j = q - nb * P.nbr_dim;
                    dst = mode == QS_ENC_NBR_MLP ? x_nbr + a * ENC_XW + q : x_nbr + (nb * ENC_TA + a) * ENC_XS + j;
                } else dst = x_obst + a * ENC_XS + (cidx - P.self_dim - P.nbr_dim * NB);
                put1<SP>(dst, v[it]);
            }
        }
    }
    __syncthreads();

    ENC_STAMP(1);
    mlp2_one_tile<SP>(P.s1, P.s2, mt0, x_self, ENC_XS, buf_b, cat, ENC_CS, 0);                  // self encoder -> cat[:, 0:256]
    ENC_STAMP(2);
    if (P.obst_dim > 0) {
        __syncthreads();
        mlp2_one_tile<SP>(P.o1, P.o2, mt0, x_obst, ENC_XS, buf_b, cat, ENC_CS, col_obst);       // obstacle encoder -> cat[:, 512:768]
    }
    __syncthreads();

    ENC_STAMP(3);
    // ---- neighbour encoder -> cat[:, 256:512] ----
    if (nbr_enc && mode == QS_ENC_NBR_MLP) {
        // mlp neighbour encoder (:104-122): three layers on the concatenated neighbour observations of the agent
        f32x4 acc[ENC_MT][1];
        init_bias<ENC_MT, 1>(P.n1, mt0, acc);
        gemm_tiles<ENC_MT, 1, SP>(P.n1, mt0, x_nbr, ENC_XW, acc);
        store_tanh<ENC_MT, 1, SP>(acc, mt0, buf_a, ENC_YS);
        __syncthreads();
        mlp2_one_tile<SP>(P.n2, P.n3, mt0, buf_a, ENC_YS, buf_a + ENC_TA * ENC_YS, cat, ENC_CS, col_nbr);
    } else if (nbr_enc) {
        // mean_embed (:22-43) in passes of up to ENC_NH neighbour tiles: the hidden layer of the neighbour MLP is the largest LDS
        // buffer, and at half its size two workgroups fit one CU (the layer chain of one workgroup is latency-bound, a second overlaps it)
        f32x4 mean[ENC_MT];
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) mean[mt] = (f32x4){0, 0, 0, 0};
        for (int t0 = 0; t0 < NB; t0 += ENC_NH) {
#define ENC_CALL(n) mean_pass<n, SP>(P, t0, x_nbr, buf_a, mean)
            ENC_DISPATCH_NT(NB - t0, ENC_NH, ENC_CALL)
#undef ENC_CALL
        }
        const float inv = 1.0f / (float)NB;   // torch.mean(neighbor_embeds, dim=1) (:41-42)
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = mean[mt][r] * inv;
            put4<SP>(cat + (lane & 15) * ENC_CS + col_nbr + (mt0 + mt) * 16 + (lane >> 4) * 4, v);
        }
    }
    __syncthreads();

    ENC_STAMP(7);
    feed_forward<ENC_MTF, SP>(P, cat, a0, B, out, (float *)buf_a);
    ENC_STAMP(9);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, ENC_OCC) qs_encoder_kernel(const float *__restrict__ obs, int B,
    EncParams P, float *__restrict__ out) {
    main_body<false>(obs, B, P, out);
}
extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_split_kernel(const float *__restrict__ obs, int B,
    EncParams P, float *__restrict__ out) {
    main_body<true>(obs, B, P, out);
}

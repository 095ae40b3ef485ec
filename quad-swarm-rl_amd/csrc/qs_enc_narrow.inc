// ------------------------------------------------------------------------------------------------
// QuadSingleHeadAttentionEncoder_Sim2Real (quad_multi_model.py:199-248, attention_layer.py:57-92) at the widths that fit a Crazyflie's
// microcontroller: H = rnn_size = 16, 32, 64 (swarm_rl/sim2real/code_blocks.py emits 16), every layer H wide.  At these widths a layer is one
// to four MFMA tiles, so the 256-wide body's split of a layer over eight waves with barriers in between has nothing to split:
//
// ONE WAVE owns 16 agents from observation row to output row.  Agents are the N dimension of v_mfma_f32_16x16x32_f16, the packed weights
// (reference precision: fp16 pairs, pack_linear(split=True), the fragment order of include/quadswarm_encoder.h) the A operand, three MFMAs per
// product (split2, qs_enc_device.h).  An accumulator tile holds features 4 (lane >> 4) + r of agent (lane & 15); as the next layer's B operand
// the same agent's features 8 (lane >> 4) + j are wanted: the agent stays on its lane & 15, only the lane group changes, through a [16][64]
// LDS slice (two fp16 planes) PRIVATE to the wave.  No s_barrier anywhere: the writes and the reads of a slice are DS instructions of one wave,
// which the LDS serves in program order; a wavefront-scope fence between them keeps the COMPILER from hoisting the reads over the writes
// (different lanes, so no data dependence it can see).  Observation columns go from global memory straight into B fragments, one dword
// per element: rows are not 16-byte aligned in the deployed shape (obs_dim = 18 + 36 + 9 = 63).  Scores, softmax, residual and
// LayerNorm in fp32, lane-local plus two shuffles over the four lane groups of an agent.
// Epilogues as in feed_forward (qs_enc_device.h): the linear head, Gaussian sampling with qs_rollout_pre's Philox keying, the trajectory copy.
// WAVES per workgroup (ENC_NW_WAVES, a build-time constant) is a launch shape only - waves share nothing; qs_enc_narrow_plan.h has the grid and
// the LDS bytes.  Measured at 8192 agents, H = 16: one wave per workgroup 6.5 us, four waves 7.2 us (DESIGN.md 10) - one wave is built.
// ------------------------------------------------------------------------------------------------
struct NwFrag { f16x8 h, l; };   // one K-step of the B operand, 16 agents: the two fp16 planes

#define ENC_NW_PLANE (ENC_NW_AGENTS * ENC_NW_XS)   // elements between the planes of a wave's slice

__device__ __forceinline__ void nw_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// observation columns [k0, k0 + 8) of a block of `width` columns that starts at element `first` of the buffer (zero behind the block, zero for a
// row past the batch)
__device__ __forceinline__ NwFrag nw_obs_frag(__amdgpu_buffer_rsrc_t rs, bool row_ok, uint32_t first, int width, int k0) {
    NwFrag f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        _Float16 h, l;
        split2(obs_at(rs, row_ok && k0 + j < width, first + k0 + j), h, l);
        f.h[j] = h;
        f.l[j] = l;
    }
    return f;
}

template <int MT>
__device__ __forceinline__ void nw_bias(const EncLayer &L, f32x4 (&acc)[MT]) {
    const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = *(const f32x4 *)(L.b + mt * 16 + g * 4);
}
template <int MT>
__device__ __forceinline__ void nw_zero(f32x4 (&acc)[MT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0, 0, 0, 0};
}
template <int MT>
__device__ __forceinline__ void nw_tanh(f32x4 (&acc)[MT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mt][r] = fast_tanh(acc[mt][r]);
}

// acc[mt] += W[features of tile mt] x b: all MT feature tiles of the layer over (at most) KS K-steps.  Fragment addresses as in
// gemm_tiles_split; a layer packed with fewer K-steps than KS (the neighbour embedding of one to five neighbours) stops at its own count.
template <int MT, int KS>
__device__ __forceinline__ void nw_gemm(const EncLayer &L, const NwFrag (&b)[KS], f32x4 (&acc)[MT]) {
    const uint32_t voff = (threadIdx.x & 63) * 16;
    const int kl = L.K >> 5;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void *)L.w, 0, L.M * L.K * 4, 0x00020000);
    f32x4 lo[MT];
    nw_zero<MT>(lo);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks < kl) {
            f16x8 ah[MT], al[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                ah[mt] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, voff, ((mt * kl + ks) * 2 + 0) * 1024, 0));
                al[mt] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, voff, ((mt * kl + ks) * 2 + 1) * 1024, 0));
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], b[ks].h, acc[mt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) lo[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mt], b[ks].l, lo[mt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) lo[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[mt], b[ks].h, lo[mt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mt][r] += lo[mt][r] * (1.0f / ENC_SPLIT_SCALE);
}

// accumulator tiles -> columns [col0, col0 + 16 NT) of the wave's slice / 16 zero columns / one K-step of the slice as a B fragment
template <int NT>
__device__ __forceinline__ void nw_put(uint16_t *slice, const f32x4 (&c)[NT], int col0) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int t = 0; t < NT; ++t) put4<true>(slice + (lane & 15) * ENC_NW_XS + col0 + t * 16 + (lane >> 4) * 4, c[t], ENC_NW_PLANE);
}
__device__ __forceinline__ void nw_put_zero16(uint16_t *slice, int col0) {
    const int lane = threadIdx.x & 63;
    uint16_t *p = slice + (lane & 15) * ENC_NW_XS + col0 + (lane >> 4) * 4;
    *(f16x4 *)p = (f16x4){0, 0, 0, 0};
    *(f16x4 *)(p + ENC_NW_PLANE) = (f16x4){0, 0, 0, 0};
}
__device__ __forceinline__ NwFrag nw_get(const uint16_t *slice, int ks) {
    const int lane = threadIdx.x & 63;
    const uint16_t *p = slice + (lane & 15) * ENC_NW_XS + ks * 32 + (lane >> 4) * 8;
    NwFrag f;
    f.h = *(const f16x8 *)p;
    f.l = *(const f16x8 *)(p + ENC_NW_PLANE);
    return f;
}
// H features in accumulator layout -> the B fragments of a layer that reads them as its columns [0, H) (K padded to 32 with zeros)
template <int NH>
__device__ __forceinline__ void nw_as_operand(uint16_t *slice, const f32x4 (&c)[NH], NwFrag (&b)[(NH + 1) / 2]) {
    nw_fence();   // (the reads of the previous use stay in front of these writes)
    nw_put<NH>(slice, c, 0);
    if constexpr (NH & 1) nw_put_zero16(slice, 16 * NH);
    nw_fence();   // the reads below stay behind the writes above: other lanes' data
#pragma unroll
    for (int ks = 0; ks < (NH + 1) / 2; ++ks) b[ks] = nw_get(slice, ks);
}

template <int NH, int WAVES>
__device__ __forceinline__ void narrow_body(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ out) {
    constexpr int H = 16 * NH, KSH = (NH + 1) / 2, KSC = (3 * NH + 1) / 2;   // K-steps of an H-wide / a 3H-wide input
    __shared__ __align__(16) uint16_t lds[WAVES * 2 * ENC_NW_PLANE];
    const int wave = wave_id(), lane = threadIdx.x & 63, g = lane >> 4;
    const int wg0 = blockIdx.x * (ENC_NW_AGENTS * WAVES), a0 = wg0 + ENC_NW_AGENTS * wave, ga = a0 + (lane & 15);
    uint16_t *const slice = lds + wave * 2 * ENC_NW_PLANE;
    traj_copy(P, wg0, ENC_NW_AGENTS * WAVES, B);
    if (a0 >= B) return;   // a wave behind the batch: nobody waits for it
    const bool ok = ga < B;

    // ---- one-layer tanh embeddings (:222-234): self -> es, all neighbour columns -> token 0, obstacle columns -> token 1 ----
    const int nbw = P.nbr_dim * P.num_nbr;
    const uint32_t row = (uint32_t)ga * (uint32_t)P.obs_dim;
    const __amdgpu_buffer_rsrc_t rs = obs_rsrc(obs, B, P.obs_dim);
    f32x4 es[NH], tk[2][NH];
    {
        const NwFrag xs[1] = {nw_obs_frag(rs, ok, row, P.self_dim, 8 * g)};
        const NwFrag xn[2] = {nw_obs_frag(rs, ok, row + P.self_dim, nbw, 8 * g), nw_obs_frag(rs, ok, row + P.self_dim, nbw, 32 + 8 * g)};
        const NwFrag xo[1] = {nw_obs_frag(rs, ok, row + P.self_dim + nbw, P.obst_dim, 8 * g)};
        nw_bias<NH>(P.s1, es);
        nw_gemm<NH, 1>(P.s1, xs, es);
        nw_bias<NH>(P.n1, tk[0]);
        nw_gemm<NH, 2>(P.n1, xn, tk[0]);
        nw_bias<NH>(P.o1, tk[1]);
        nw_gemm<NH, 1>(P.o1, xo, tk[1]);
        nw_tanh<NH>(es);
        nw_tanh<NH>(tk[0]);
        nw_tanh<NH>(tk[1]);
    }

    // ---- OneHeadAttention over the two tokens (attention_layer.py:57-92): q, k, v, fc without bias ----
    f32x4 v[2][NH];
    float pr[2][2];
    {
        NwFrag tb[2][KSH];
        f32x4 q[2][NH], k[2][NH];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            nw_as_operand<NH>(slice, tk[i], tb[i]);
            nw_zero<NH>(q[i]);
            nw_gemm<NH, KSH>(P.mq, tb[i], q[i]);
            nw_zero<NH>(k[i]);
            nw_gemm<NH, KSH>(P.mk, tb[i], k[i]);
            nw_zero<NH>(v[i]);
            nw_gemm<NH, KSH>(P.mv, tb[i], v[i]);
        }
        constexpr float scale = NH == 1 ? 0.25f : NH == 2 ? 0.17677669529663687f : 0.125f;   // 1 / sqrt(H)   (:83)
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
            const float m = fmaxf(t[0], t[1]), e0 = __expf(t[0] - m), e1 = __expf(t[1] - m), rd = 1.0f / (e0 + e1);
            pr[i][0] = e0 * rd;
            pr[i][1] = e1 * rd;
        }
    }
    // o_i = sum_j p_ij v_j -> fc -> + token i -> LayerNorm (eps 1e-6), in place of the token
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        f32x4 o[NH], y[NH];
#pragma unroll
        for (int mt = 0; mt < NH; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[mt][r] = pr[i][0] * v[0][mt][r] + pr[i][1] * v[1][mt][r];
        NwFrag ob[KSH];
        nw_as_operand<NH>(slice, o, ob);
        nw_zero<NH>(y);
        nw_gemm<NH, KSH>(P.mfc, ob, y);
        float s1 = 0.0f;
#pragma unroll
        for (int mt = 0; mt < NH; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                y[mt][r] += tk[i][mt][r];
                s1 += y[mt][r];
            }
        const float mean = lane_groups_sum(s1) * (1.0f / H);
        float s2 = 0.0f;
#pragma unroll
        for (int mt = 0; mt < NH; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s2 += (y[mt][r] - mean) * (y[mt][r] - mean);
        const float rstd = 1.0f / __builtin_sqrtf(lane_groups_sum(s2) * (1.0f / H) + 1e-6f);
#pragma unroll
        for (int mt = 0; mt < NH; ++mt) {
            const f32x4 gw = *(const f32x4 *)(P.ln_w + mt * 16 + g * 4), gb = *(const f32x4 *)(P.ln_b + mt * 16 + g * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) tk[i][mt][r] = (y[mt][r] - mean) * rstd * gw[r] + gb[r];
        }
    }

    // ---- feed forward (:240-242): tanh(F [self | token 0 | token 1]), 3H -> H ----
    NwFrag cb[KSC];
    if constexpr (NH == 1) {   // 48 columns: the three parts share K-steps, so they meet in the slice
        nw_fence();
        nw_put<1>(slice, es, 0);
        nw_put<1>(slice, tk[0], 16);
        nw_put<1>(slice, tk[1], 32);
        nw_put_zero16(slice, 48);
        nw_fence();   // as in nw_as_operand
        cb[0] = nw_get(slice, 0);
        cb[1] = nw_get(slice, 1);
    } else {                   // H a multiple of 32: every part its own K-steps
        auto part = [&](const f32x4 (&c)[NH], int p) {
            NwFrag b[KSH];
            nw_as_operand<NH>(slice, c, b);
#pragma unroll
            for (int ks = 0; ks < KSH; ++ks) cb[p * KSH + ks] = b[ks];
        };
        part(es, 0);
        part(tk[0], 1);
        part(tk[1], 2);
    }
    f32x4 fo[NH];
    nw_bias<NH>(P.f, fo);
    nw_gemm<NH, KSC>(P.f, cb, fo);
    nw_tanh<NH>(fo);
    if (out && ok) {
#pragma unroll
        for (int mt = 0; mt < NH; ++mt) *(f32x4 *)(out + (size_t)ga * H + mt * 16 + g * 4) = fo[mt];
    }
    // ---- linear head on the features, Gaussian sampling behind it (feed_forward's epilogue on one wave) ----
    for (int h = 0; h < P.head_dim; ++h) {
        float s = 0.0f;
#pragma unroll
        for (int mt = 0; mt < NH; ++mt) {
            const f32x4 w = *(const f32x4 *)(P.head_w + h * H + mt * 16 + g * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) s += fo[mt][r] * w[r];
        }
        s = lane_groups_sum(s) + P.head_b[h];   // (every lane group of the agent holds the same sum: group h & 3 writes it)
        if (ok && g == (h & 3)) {
            P.head_out[(size_t)ga * P.head_dim + h] = s;
            if (P.sample_log_std) P.act_out[(size_t)ga * P.head_dim + h] = sample_action(P, ga, h, s);
        }
    }
}

#define ENC_NARROW_KERNEL(NH, H)                                                                                                              \
    extern "C" __global__ void __launch_bounds__(64 * ENC_NW_WAVES) qs_encoder_narrow##H##_kernel(const float *__restrict__ obs, int B, EncParams P, \
        float *__restrict__ out) {                                                                                                            \
        narrow_body<NH, ENC_NW_WAVES>(obs, B, P, out);                                                                                        \
    }
ENC_NARROW_KERNEL(1, 16) ENC_NARROW_KERNEL(2, 32) ENC_NARROW_KERNEL(4, 64)
#undef ENC_NARROW_KERNEL

// ================================================================================================
// Wide variants: 32 agents per workgroup, one workgroup per CU (batches of >= ENC_WIDE_MIN agents).
//
// Phase stamps (tools/enc_stamps.py, profiles/r02_encoder_*): one 16-agent workgroup ALONE on the GPU needs 89 % of the time 512
// of them need - the kernel is the latency of one workgroup's chain of dependent layers, and a third of that chain is exposed L2
// latency: every layer starts with a load of its bias and first weight fragments (~650 ticks of a 36 k-tick chain each), a
// 256-wide layer waits a second time for the K-steps beyond the four-deep ring, the 512-wide feed-forward four times.  Here
//   * the weight ring holds a whole 256-wide layer (ENC_WPD = 8 K-steps) and is carried ACROSS layers: the slot an MFMA group of
//     the last ENC_WPD K-steps has consumed is refilled with the NEXT layer's fragment, so those loads fly during the tail of the
//     K loop, the tanh epilogue and the barrier, and the next layer starts on weights that are already in registers;
//   * the bias is added after the K loop instead of seeding the accumulators (its load is issued before the loop and first
//     needed behind it);
//   * 32 agents per workgroup halve the weight stream per agent and the barriers per agent; the register file of the lone
//     workgroup (2 waves per SIMD, 256 VGPRs) holds the deeper ring and the wider accumulator tiles.
// ================================================================================================
#define ENC_WPD 8                   // weight ring depth (K-steps)
struct WRing { bf16x8 a[ENC_WPD][ENC_MT]; };

// a layer without weights (w == nullptr, M == 0): every load is out of range and returns zero
__device__ __forceinline__ __amdgpu_buffer_rsrc_t layer_rsrc(const EncLayer &L) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)L.w, 0, L.M * L.K * 2, 0x00020000);
}
#define ENC_RFRAG(rs, mtile, kst, mt, ks) ENC_WLOAD(__builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (((mtile) + (mt)) * (kst) + (ks)) * 1024, 0)))
// a ring slot past the layer's K-steps (the 32-wide input layers fill one of the eight): through a resource of zero records - the load
// returns zero and moves no data (in range it would read the next feature tiles' fragments: 14 KiB per wave and layer of traffic on
// the CU's 64 B / clock L2 port that nobody multiplies - a third more than the network's weights, ahead of the observation loads)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t layer_rsrc_k(const EncLayer &L, int ks) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)L.w, 0, ks < (L.K >> 5) ? L.M * L.K * 2 : 0, 0x00020000);
}
#define ENC_RFRAG_K(L, mtile, kst, mt, ks) ENC_RFRAG(layer_rsrc_k(L, ks), mtile, kst, mt, ks)

__device__ __forceinline__ void ring_fill(WRing &R, const EncLayer &L, int mtile0) {
    const uint32_t voff = (threadIdx.x & 63) * 16;
    const int kst = L.K >> 5;
    const __amdgpu_buffer_rsrc_t rs = layer_rsrc(L);
#pragma unroll
    for (int s = 0; s < ENC_WPD; ++s)
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) R.a[s][mt] = ENC_RFRAG_K(L, mtile0, kst, mt, s);
}

// acc (+)= L[features of (wave, mt)] x X[row tiles]; the ring holds L's first ENC_WPD K-steps on entry and Ln's on exit.
// KS = K / 32 of L is a template parameter: a run-time K-step count puts branches and a loop around the loads, behind which the
// compiler no longer knows how many are in flight and waits for ALL of them (s_waitcnt vmcnt(0)) at the next use of any loaded
// value - i.e. for the whole prefetched next layer at the end of every layer.
template <int NT, int KS>
__device__ __forceinline__ void gemm_ring(WRing &R, const EncLayer &L, int mtile0, const EncLayer &Ln, int mtile0n, const uint16_t *X,
    int xstride,
                                          f32x4 (&acc)[ENC_MT][NT]) {
    const int lane = threadIdx.x & 63, kn = Ln.K >> 5;
    const uint16_t *xrow = X + (lane & 15) * xstride + 8 * (lane >> 4);
    const uint32_t voff = lane * 16;
    const __amdgpu_buffer_rsrc_t rs = layer_rsrc(L), rsn = layer_rsrc(Ln);
    bf16x8 b[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b[nt] = ENC_XFRAG(nt, 0);
    if constexpr (KS < ENC_WPD) {   // the 32- and 64-wide input layers
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                mfma_tile<ENC_MT, NT>(R.a[s], b[nt], acc, nt);
                if (s + 1 < KS) b[nt] = ENC_XFRAG(nt, s + 1);
            }
#pragma unroll
        for (int s = 0; s < ENC_WPD; ++s)
#pragma unroll
            for (int mt = 0; mt < ENC_MT; ++mt) R.a[s][mt] = ENC_RFRAG_K(Ln, mtile0n, kn, mt, s);
    } else {
        static_assert(KS % ENC_WPD == 0, "K-steps of a hidden layer: a multiple of the ring depth");
#pragma unroll
        for (int ks0 = 0; ks0 + ENC_WPD < KS; ks0 += ENC_WPD) {   // K > 256: the ring is refilled with this layer's next K-steps
#pragma unroll
            for (int s = 0; s < ENC_WPD; ++s) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    mfma_tile<ENC_MT, NT>(R.a[s], b[nt], acc, nt);
                    b[nt] = ENC_XFRAG(nt, ks0 + s + 1);
                }
#pragma unroll
                for (int mt = 0; mt < ENC_MT; ++mt) R.a[s][mt] = ENC_RFRAG(rs, mtile0, KS, mt, ks0 + s + ENC_WPD);
                // keep the K-steps in program order: hoisted LDS reads of later K-steps cost 4 VGPRs per tile each
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int s = 0; s < ENC_WPD; ++s) {   // the last ENC_WPD K-steps: each consumed slot takes the next layer's fragment
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                mfma_tile<ENC_MT, NT>(R.a[s], b[nt], acc, nt);
                if (s + 1 < ENC_WPD) b[nt] = ENC_XFRAG(nt, KS - ENC_WPD + s + 1);
            }
#pragma unroll
            for (int mt = 0; mt < ENC_MT; ++mt) R.a[s][mt] = ENC_RFRAG_K(Ln, mtile0n, kn, mt, s);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

struct Bias { f32x4 v[ENC_MT]; };
__device__ __forceinline__ Bias load_bias(const EncLayer &L, int mtile0) {
    Bias b;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) b.v[mt] = *(const f32x4 *)(L.b + (mtile0 + mt) * 16 + (lane >> 4) * 4);
    return b;
}
template <int NT>
__device__ __forceinline__ void add_bias(f32x4 (&acc)[ENC_MT][NT], const Bias &b) {
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mt][nt][r] += b.v[mt][r];
}
// one layer of the chain: acc = L X + b (fp32, before the non-linearity)
template <int NT, int KS>
__device__ __forceinline__ void layer_ring(WRing &R, const EncLayer &L, int mtile0, const EncLayer &Ln, int mtile0n, const uint16_t *X,
    int xstride,
                                           f32x4 (&acc)[ENC_MT][NT]) {
    const Bias b = load_bias(L, mtile0);
    zero_acc<ENC_MT, NT>(acc);
    gemm_ring<NT, KS>(R, L, mtile0, Ln, mtile0n, X, xstride, acc);
    add_bias<NT>(acc, b);
}

// the same without the bias: acc = L X, bc = b * ENC_TANH_C for the tanh4_bias epilogues (mean_embed: wide_body, pp_body)
struct BiasC { f32x4 v[ENC_MT]; };
template <int NT, int KS>
__device__ __forceinline__ void layer_ring_raw(WRing &R, const EncLayer &L, int mtile0, const EncLayer &Ln, int mtile0n, const uint16_t *X,
    int xstride,
                                               f32x4 (&acc)[ENC_MT][NT], BiasC &bc) {
    const Bias b = load_bias(L, mtile0);
    zero_acc<ENC_MT, NT>(acc);
    gemm_ring<NT, KS>(R, L, mtile0, Ln, mtile0n, X, xstride, acc);
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) bc.v[mt] = b.v[mt] * ENC_TANH_C;
}

// A 512-wide layer (16 K-steps) on TWO rings: R holds its K-steps 0-7 and R2 its K-steps 8-15 on entry, the next layer's (or feature
// half's) on exit.  The feed-forward layer's 512 KB are half of the network's weights and four times its MFMA time on the CU's 64 B / clock
// port; with its first feature half resident when the layer starts (R through the ring as always, R2 filled while the neighbour MLP - which
// leaves the port three quarters idle - still runs), only the second half streams under the first half's K loop and epilogue.
template <int NT>
__device__ __forceinline__ void gemm_ring2(WRing &R, WRing &R2, const EncLayer &Ln, int mtile0n, const uint16_t *X, int xstride,
                                           f32x4 (&acc)[ENC_MT][NT]) {
    const int lane = threadIdx.x & 63, kn = Ln.K >> 5;
    const uint16_t *xrow = X + (lane & 15) * xstride + 8 * (lane >> 4);
    const uint32_t voff = lane * 16;
    bf16x8 b[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b[nt] = ENC_XFRAG(nt, 0);
#pragma unroll
    for (int s = 0; s < 2 * ENC_WPD; ++s) {
        WRing &Q = s < ENC_WPD ? R : R2;
        const int q = s & (ENC_WPD - 1);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            mfma_tile<ENC_MT, NT>(Q.a[q], b[nt], acc, nt);
            if (s + 1 < 2 * ENC_WPD) b[nt] = ENC_XFRAG(nt, s + 1);
        }
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) Q.a[q][mt] = ENC_RFRAG_K(Ln, mtile0n, kn, mt, s);
        __builtin_amdgcn_sched_barrier(0);
    }
}
__device__ __forceinline__ void ring2_fill(WRing &R2, const EncLayer &L, int mtile0) {   // K-steps 8-15 of L
    const uint32_t voff = (threadIdx.x & 63) * 16;
    const int kst = L.K >> 5;
#pragma unroll
    for (int s = 0; s < ENC_WPD; ++s)
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) R2.a[s][mt] = ENC_RFRAG_K(L, mtile0, kst, mt, ENC_WPD + s);
}
template <int NT>
__device__ __forceinline__ void layer_ring2_raw(WRing &R, WRing &R2, const EncLayer &L, int mtile0, const EncLayer &Ln, int mtile0n,
                                                const uint16_t *X, int xstride, f32x4 (&acc)[ENC_MT][NT], BiasC &bc) {
    const Bias b = load_bias(L, mtile0);
    zero_acc<ENC_MT, NT>(acc);
    gemm_ring2<NT>(R, R2, Ln, mtile0n, X, xstride, acc);
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt) bc.v[mt] = b.v[mt] * ENC_TANH_C;
}

// epilogues of the wide kernels: one row tile at a time (a scheduling fence after each - interleaving a dozen tanh chains costs
// more registers than it hides latency, and the weight ring has to stay resident through them)
template <int NT>
__device__ __forceinline__ void store_tanh_wide(const f32x4 (&acc)[ENC_MT][NT], int mtile0, uint16_t *Y, int ystride, int col0 = 0) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) {
            const f32x4 t = tanh4(acc[mt][nt]);
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (__bf16)t[r];
            *(bf16x4 *)(Y + (nt * 16 + (lane & 15)) * ystride + col0 + (mtile0 + mt) * 16 + (lane >> 4) * 4) = v;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int NT>
__device__ __forceinline__ void store_tanh_wide_b(const f32x4 (&acc)[ENC_MT][NT], const BiasC &bc, int mtile0, uint16_t *Y, int ystride, int col0 = 0) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) {
            const f32x4 t = tanh4_bias(acc[mt][nt], bc.v[mt]);
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (__bf16)t[r];
            *(bf16x4 *)(Y + (nt * 16 + (lane & 15)) * ystride + col0 + (mtile0 + mt) * 16 + (lane >> 4) * 4) = v;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// observation rows of the workgroup's ENC_WA agents -> bf16 staging rows (self [WA][XS] | neighbours [(k*WA + a)][XS] | obstacles [WA][XS]; the
// three are contiguous).  One lane = one 8-column chunk of one staging row: its eight observation elements through the buffer resource
// (a column past the row's width, a neighbour slot past the count, an agent past the batch: out of range, reads as zero - the padding
// needs no separate clearing), four v_cvt_pk_bf16_f32, one ds_write_b128.  Chunk-major order over rows padded to 6 waves: the chunk
// index is wave-uniform, and a chunk past every input width is written as zeros without loads.  No division, no lane-divergent branch,
// every LDS element written once (no barrier inside): ~40 instructions per lane and iteration where the element-wise version spent
// ~50 per ELEMENT on index arithmetic under exec masks - in a kernel that issues one instruction per ~5 ticks per wave.
__device__ __forceinline__ void stage_obs_wide(const float *__restrict__ obs, int B, const EncParams &P, int a0, uint16_t *x_self,
    uint16_t *x_nbr, uint16_t *x_obst) {
    (void)x_nbr; (void)x_obst;
    constexpr int ROWS = (2 + ENC_WSLOTS) * ENC_WA, ROWS_P = (ROWS + 63) / 64 * 64, ITERS = (4 * ROWS_P + 64 * ENC_WAVES - 1) / (64 * ENC_WAVES);
    static_assert(ENC_WA == 32 && ENC_XS % 8 == 0, "row decoding by shifts; 16-byte aligned chunks");
    const int tid = threadIdx.x, D = P.obs_dim, NB = P.num_nbr;
    const __amdgpu_buffer_rsrc_t ors = obs_rsrc(obs, B, D);
    const int maxdim = max(P.self_dim, max(P.nbr_dim, P.obst_dim));
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int idx = tid + it * 64 * ENC_WAVES;
        const int ch = __builtin_amdgcn_readfirstlane(idx / ROWS_P), row = idx - ch * ROWS_P, col0 = ch * 8;   // ROWS_P: a multiple of 64
        if (ch >= 4) break;
        const bool is_self = row < ENC_WA, is_obst = row >= (1 + ENC_WSLOTS) * ENC_WA;
        const int r = row - ENC_WA, nb = r >> 5;
        const int a = is_self ? row : (is_obst ? row - (1 + ENC_WSLOTS) * ENC_WA : (r & (ENC_WA - 1)));
        const int dim = is_self ? P.self_dim : (is_obst ? P.obst_dim : (nb < NB ? P.nbr_dim : 0));
        const int cbase = is_self ? 0 : (is_obst ? P.self_dim + P.nbr_dim * NB : P.self_dim + nb * P.nbr_dim);
        const int ga = a0 + a;
        const uint32_t first = (uint32_t)ga * (uint32_t)D + (uint32_t)(cbase + col0);
        const int left = (ga < B && row < ROWS) ? dim - col0 : 0;   // valid elements of this chunk
        bf16x8 h;
        if (col0 < maxdim) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = obs_at(ors, u < left, first + u);
#pragma unroll
            for (int u = 0; u < 8; ++u) h[u] = (__bf16)v[u];
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) h[u] = (__bf16)0.0f;
        }
        if (row < ROWS) *(bf16x8 *)(x_self + row * ENC_XS + col0) = h;
    }
}

// linear head on the features of the wide kernels (see feed_forward): red = [8 waves][8 heads][ENC_WA] floats; acc = the wave's tanh'd
// feed-forward outputs
__device__ __forceinline__ void wide_head(const EncParams &P, const f32x4 (&acc)[2][ENC_MT][ENC_AT], int a0, int B, float *red) {
    const int wave = wave_id(), lane = threadIdx.x & 63, mf0 = wave * ENC_MTF;
    {
        for (int hd = 0; hd < P.head_dim; ++hd) {
            float sp[ENC_AT];
#pragma unroll
            for (int h = 0; h < ENC_AT; ++h) sp[h] = 0.0f;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int mt = 0; mt < ENC_MT; ++mt) {
                    const f32x4 w = *(const f32x4 *)(P.head_w + hd * (2 * ENC_H) + (mf0 + hf * ENC_MT + mt) * 16 + (lane >> 4) * 4);
#pragma unroll
                    for (int h = 0; h < ENC_AT; ++h)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sp[h] += acc[hf][mt][h][r] * w[r];
                }
#pragma unroll
            for (int h = 0; h < ENC_AT; ++h) {
                const float t = lane_groups_sum(sp[h]);
                if (lane < 16) red[(wave * 8 + hd) * ENC_WA + h * 16 + lane] = t;
            }
        }
        __syncthreads();
        const int tid = threadIdx.x, hd = tid / ENC_WA, row = tid % ENC_WA;
        if (hd < P.head_dim && a0 + row < B) {
            float t = P.head_b[hd];
#pragma unroll
            for (int w = 0; w < ENC_WAVES; ++w) t += red[(w * 8 + hd) * ENC_WA + row];
            P.head_out[(size_t)(a0 + row) * P.head_dim + hd] = t;
            if (P.sample_log_std) P.act_out[(size_t)(a0 + row) * P.head_dim + hd] = sample_action(P, a0 + row, hd, t);
        }
    }
}

// feed forward on the ring: the wave's 64 output features as two 32-feature halves over the same `cat` rows
template <int KS>   // K-steps of the feed-forward layer: 16 ([self | neighbourhood]) or 24 (with obstacles)
__device__ __forceinline__ void feed_forward_wide(WRing &R, const EncParams &P, const uint16_t *cat, int a0, int B,
    float *__restrict__ out, float *red) {
    const int wave = wave_id(), lane = threadIdx.x & 63, mf0 = wave * ENC_MTF;
    const EncLayer none = {nullptr, nullptr, 0, 0};
    f32x4 acc[2][ENC_MT][ENC_AT];
    BiasC bc[2];
    layer_ring_raw<ENC_AT, KS>(R, P.f, mf0, P.f, mf0 + ENC_MT, cat, ENC_CS, acc[0], bc[0]);
    layer_ring_raw<ENC_AT, KS>(R, P.f, mf0 + ENC_MT, none, 0, cat, ENC_CS, acc[1], bc[1]);
    ENC_STAMP(8);
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
            for (int h = 0; h < ENC_AT; ++h) {
                const int ga = a0 + h * 16 + (lane & 15);
                acc[hf][mt][h] = tanh4_bias(acc[hf][mt][h], bc[hf].v[mt]);
                if (out && ga < B) *(f32x4 *)(out + (size_t)ga * (2 * ENC_H) + (mf0 + hf * ENC_MT + mt) * 16 + (lane >> 4) * 4) = acc[hf][mt][h];
            }
    if (P.head_dim > 0) wide_head(P, acc, a0, B, red);
}

// mean += tanh(acc + b) of the row tiles of neighbours t0.. (a neighbour slot past the count: masked out)
template <int NT>
__device__ __forceinline__ void tanh_into_mean(const f32x4 (&acc)[ENC_MT][NT], const BiasC &bc, int t0, int num_nbr, f32x4 (&mean)[ENC_MT][ENC_AT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const float keep = t0 + nt / ENC_AT < num_nbr ? 1.0f : 0.0f;
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) mean[mt][nt % ENC_AT] += keep * tanh4_bias(acc[mt][nt], bc.v[mt]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// mean_embed, wide: per-neighbour MLP in passes of WNP neighbours (WNP * ENC_AT row tiles, tile = neighbour * ENC_AT + agent half).
// WNP is a template parameter picked per neighbour count at launch (one pass body, no run-time tile counts); a last pass that
// runs past the neighbour count works on zero rows and is masked out of the mean.
template <int WNP>
__device__ __forceinline__ void mean_pass_wide(WRing &R, const EncParams &P, int t0, const EncLayer &after, int mt_after,
    const uint16_t *x_nbr, uint16_t *buf_a,
                                               f32x4 (&mean)[ENC_MT][ENC_AT]) {
    constexpr int NT = WNP * ENC_AT;
    const int wave = wave_id(), mt0 = wave * ENC_MT;
    f32x4 acc[ENC_MT][NT];
    BiasC bc;
    layer_ring_raw<NT, 1>(R, P.n1, mt0, P.n2, mt0, x_nbr + t0 * ENC_WA * ENC_XS, ENC_XS, acc, bc);
    ENC_STAMP(4);
    if (t0) __syncthreads();   // the previous pass's second layer is done reading buf_a
    store_tanh_wide_b<NT>(acc, bc, mt0, buf_a, ENC_YS);
    __syncthreads();
    ENC_STAMP(5);
    layer_ring_raw<NT, 8>(R, P.n2, mt0, after, mt_after, buf_a, ENC_YS, acc, bc);
    ENC_STAMP(6);
    tanh_into_mean<NT>(acc, bc, t0, P.num_nbr, mean);
}

template <int WNP>
__device__ __forceinline__ void wide_body(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsWide Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_self = lds + Lds::x_self, *x_nbr = lds + Lds::x_nbr, *x_obst = lds + Lds::x_obst;
    uint16_t *buf_a = lds + Lds::buf_a, *buf_b = lds + Lds::buf_b, *cat = lds + Lds::cat;
    const int wave = wave_id(), lane = threadIdx.x & 63, a0 = blockIdx.x * ENC_WA, mt0 = wave * ENC_MT, NB = P.num_nbr;
    const bool obst = P.obst_dim > 0;
    const int col_nbr = ENC_H, col_obst = 2 * ENC_H;

    ENC_STAMP(0);
    WRing R;
    ring_fill(R, P.s1, mt0);   // in flight while the observations are staged
    traj_copy(P, a0, ENC_WA, B);
    stage_obs_wide(obs, B, P, a0, x_self, x_nbr, x_obst);
    __syncthreads();
    ENC_STAMP(1);
    {
        f32x4 acc[ENC_MT][ENC_AT];
        BiasC bc;
        layer_ring_raw<ENC_AT, 1>(R, P.s1, mt0, P.s2, mt0, x_self, ENC_XS, acc, bc);
        store_tanh_wide_b<ENC_AT>(acc, bc, mt0, buf_b, ENC_YS);
        __syncthreads();
        layer_ring_raw<ENC_AT, 8>(R, P.s2, mt0, obst ? P.o1 : P.n1, mt0, buf_b, ENC_YS, acc, bc);
        store_tanh_wide_b<ENC_AT>(acc, bc, mt0, cat, ENC_CS, 0);                              // self encoder -> cat[:, 0:256]
        ENC_STAMP(2);
        if (obst) {
            layer_ring_raw<ENC_AT, 1>(R, P.o1, mt0, P.o2, mt0, x_obst, ENC_XS, acc, bc);
            __syncthreads();   // the self encoder's second layer is done reading buf_b
            store_tanh_wide_b<ENC_AT>(acc, bc, mt0, buf_b, ENC_YS);
            __syncthreads();
            layer_ring_raw<ENC_AT, 8>(R, P.o2, mt0, P.n1, mt0, buf_b, ENC_YS, acc, bc);
            store_tanh_wide_b<ENC_AT>(acc, bc, mt0, cat, ENC_CS, col_obst);                   // obstacle encoder -> cat[:, 512:768]
        }
    }
    ENC_STAMP(3);
    f32x4 mean[ENC_MT][ENC_AT];
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
        for (int h = 0; h < ENC_AT; ++h) mean[mt][h] = (f32x4){0, 0, 0, 0};
#pragma unroll 1
    for (int t0 = 0; t0 < NB; t0 += WNP) {
        const bool last = t0 + WNP >= NB;
        mean_pass_wide<WNP>(R, P, t0, last ? P.f : P.n1, last ? wave * ENC_MTF : mt0, x_nbr, buf_a, mean);
    }
    const float inv = 1.0f / (float)NB;   // torch.mean(neighbor_embeds, dim=1) (:41-42)
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
        for (int h = 0; h < ENC_AT; ++h) {
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (__bf16)(mean[mt][h][r] * inv);
            *(bf16x4 *)(cat + (h * 16 + (lane & 15)) * ENC_CS + col_nbr + (mt0 + mt) * 16 + (lane >> 4) * 4) = v;
        }
    __syncthreads();
    ENC_STAMP(7);
    if (obst) feed_forward_wide<24>(R, P, cat, a0, B, out, (float *)buf_a);
    else feed_forward_wide<16>(R, P, cat, a0, B, out, (float *)buf_a);
    ENC_STAMP(9);
}
#define ENC_WIDE_KERNEL(n)                                                                                                                          \
    extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_wide##n##_kernel(const float *__restrict__ obs, int B, EncParams P, \
                                                                                                 float *__restrict__ out) {                         \
        wide_body<n>(obs, B, P, out);                                                                                                               \
    }
ENC_WIDE_KERNEL(1) ENC_WIDE_KERNEL(2) ENC_WIDE_KERNEL(3)

// ------------------------------------------------------------------------------------------------
// mean_embed, 32 agents per workgroup, the two waves of every SIMD half a layer apart ("ping-pong").
//
// In wide_body all eight waves run the same phase at the same time: the two waves of a SIMD queue for its matrix pipe through every
// K loop and for its VALU through every tanh epilogue, and each of the two units idles through the other's phase.  Here the work is cut
// into JOBS - one layer on one group of row tiles: G (K loop: MFMA + LDS fragment reads + weight stream) then T (bias, tanh, bf16, LDS
// store) - and waves 4-7 (the second wave of SIMD 0-3) run the same job list ONE SLOT behind waves 0-3: while one wave of a SIMD is in a
// G the other is in a T, matrix pipe beside VALU (MI355X_MICROARCH.md, two waves per SIMD).  One s_barrier per slot keeps the two halves
// in that pairing.  A job that reads what job j wrote has to be at least two jobs behind j (the late half's T(j) ends one slot after
// the early half's); the list is ordered for that, with one empty job in front of the feed-forward layer:
//     n1(A) s1 n2(A) n1(B) s2 n2(B) [o1 - o2] - f(lo) f(hi)          A / B: the first / second WNP neighbours, 2 * WNP row tiles each
// LDS buffers as in wide_body; the single hidden buffer of the neighbour MLP is rewritten by T(n1(B)) two slots after the last G(n2(A))
// has read it.  Same MFMA order per output, same epilogues: the features are those of wide_body bit for bit.
// ------------------------------------------------------------------------------------------------
#define ENC_SLOT() __syncthreads()   // end of a slot: LDS writes of this wave's T visible, every wave of both halves has arrived
template <int WNP, bool OBST>
__device__ __forceinline__ void pp_body(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsWide Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_self = lds + Lds::x_self, *x_nbr = lds + Lds::x_nbr, *x_obst = lds + Lds::x_obst;
    uint16_t *buf_a = lds + Lds::buf_a, *buf_b = lds + Lds::buf_b, *cat = lds + Lds::cat;
    constexpr int NT = WNP * ENC_AT, KSF = OBST ? 24 : 16;
    const int wave = wave_id(), lane = threadIdx.x & 63, a0 = blockIdx.x * ENC_WA, mt0 = wave * ENC_MT, mf0 = wave * ENC_MTF, NB = P.num_nbr;
    const bool late = wave >= ENC_WAVES / 2;
    const EncLayer none = {nullptr, nullptr, 0, 0};

    ENC_STAMP(0);
    WRing R;
    ring_fill(R, P.n1, mt0);   // in flight while the observations are staged
    traj_copy(P, a0, ENC_WA, B);
    stage_obs_wide(obs, B, P, a0, x_self, x_nbr, x_obst);
    __syncthreads();
    ENC_STAMP(1);
    if (late) ENC_SLOT();
    f32x4 accn[ENC_MT][NT], accs[ENC_MT][ENC_AT], mean[ENC_MT][ENC_AT];
    BiasC bcn, bcs;
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
        for (int h = 0; h < ENC_AT; ++h) mean[mt][h] = (f32x4){0, 0, 0, 0};
    // n1(A)
    layer_ring_raw<NT, 1>(R, P.n1, mt0, P.s1, mt0, x_nbr, ENC_XS, accn, bcn);
    ENC_SLOT();
    store_tanh_wide_b<NT>(accn, bcn, mt0, buf_a, ENC_YS);
    ENC_SLOT();
    // s1
    layer_ring_raw<ENC_AT, 1>(R, P.s1, mt0, P.n2, mt0, x_self, ENC_XS, accs, bcs);
    ENC_SLOT();
    store_tanh_wide_b<ENC_AT>(accs, bcs, mt0, buf_b, ENC_YS);
    ENC_SLOT();
    ENC_STAMP(2);
    // n2(A)
    layer_ring_raw<NT, 8>(R, P.n2, mt0, P.n1, mt0, buf_a, ENC_YS, accn, bcn);
    ENC_SLOT();
    tanh_into_mean<NT>(accn, bcn, 0, NB, mean);
    ENC_SLOT();
    ENC_STAMP(3);
    // n1(B)
    layer_ring_raw<NT, 1>(R, P.n1, mt0, P.s2, mt0, x_nbr + WNP * ENC_WA * ENC_XS, ENC_XS, accn, bcn);
    ENC_SLOT();
    store_tanh_wide_b<NT>(accn, bcn, mt0, buf_a, ENC_YS);
    ENC_SLOT();
    ENC_STAMP(4);
    // s2
    layer_ring_raw<ENC_AT, 8>(R, P.s2, mt0, P.n2, mt0, buf_b, ENC_YS, accs, bcs);
    ENC_SLOT();
    store_tanh_wide_b<ENC_AT>(accs, bcs, mt0, cat, ENC_CS, 0);                                       // self encoder -> cat[:, 0:256]
    ENC_SLOT();
    ENC_STAMP(5);
    // n2(B)
    WRing R2;
    if constexpr (!OBST) ring2_fill(R2, P.f, mf0);   // the feed-forward layer's K-steps 8-15 (gemm_ring2): in flight from here on
    layer_ring_raw<NT, 8>(R, P.n2, mt0, OBST ? P.o1 : P.f, OBST ? mt0 : mf0, buf_a, ENC_YS, accn, bcn);
    ENC_SLOT();
    tanh_into_mean<NT>(accn, bcn, WNP, NB, mean);
    {
        const float inv = 1.0f / (float)NB;   // torch.mean(neighbor_embeds, dim=1) (:41-42)
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
            for (int h = 0; h < ENC_AT; ++h) {
                bf16x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (__bf16)(mean[mt][h][r] * inv);
                *(bf16x4 *)(cat + (h * 16 + (lane & 15)) * ENC_CS + ENC_H + (mt0 + mt) * 16 + (lane >> 4) * 4) = v;
            }
    }
    ENC_SLOT();
    ENC_STAMP(6);
    if constexpr (OBST) {
        // o1 (buf_b: the last G(s2) read it two slots ago)
        layer_ring_raw<ENC_AT, 1>(R, P.o1, mt0, P.o2, mt0, x_obst, ENC_XS, accs, bcs);
        ENC_SLOT();
        store_tanh_wide_b<ENC_AT>(accs, bcs, mt0, buf_b, ENC_YS);
        ENC_SLOT();
        ENC_SLOT(); ENC_SLOT();   // (empty job)
        // o2
        layer_ring_raw<ENC_AT, 8>(R, P.o2, mt0, P.f, mf0, buf_b, ENC_YS, accs, bcs);
        ENC_SLOT();
        store_tanh_wide_b<ENC_AT>(accs, bcs, mt0, cat, ENC_CS, 2 * ENC_H);                           // obstacle encoder -> cat[:, 512:768]
        ENC_SLOT();
    }
    ENC_SLOT(); ENC_SLOT();   // (empty job: the feed-forward layer reads what the late half's T of the job before wrote)
    ENC_STAMP(7);
    // f: the wave's 64 output features as two 32-feature halves over the same `cat` rows
    f32x4 acc[2][ENC_MT][ENC_AT];
    BiasC bcf[2];
    if constexpr (OBST) layer_ring_raw<ENC_AT, KSF>(R, P.f, mf0, P.f, mf0 + ENC_MT, cat, ENC_CS, acc[0], bcf[0]);
    else layer_ring2_raw<ENC_AT>(R, R2, P.f, mf0, P.f, mf0 + ENC_MT, cat, ENC_CS, acc[0], bcf[0]);
    ENC_SLOT();
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        if (hf == 1) {
            ENC_SLOT();
            if constexpr (OBST) layer_ring_raw<ENC_AT, KSF>(R, P.f, mf0 + ENC_MT, none, 0, cat, ENC_CS, acc[1], bcf[1]);
            else layer_ring2_raw<ENC_AT>(R, R2, P.f, mf0 + ENC_MT, none, 0, cat, ENC_CS, acc[1], bcf[1]);
            ENC_SLOT();
            ENC_STAMP(8);
        }
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
            for (int h = 0; h < ENC_AT; ++h) {
                const int ga = a0 + h * 16 + (lane & 15);
                acc[hf][mt][h] = tanh4_bias(acc[hf][mt][h], bcf[hf].v[mt]);
                if (out && ga < B) *(f32x4 *)(out + (size_t)ga * (2 * ENC_H) + (mf0 + hf * ENC_MT + mt) * 16 + (lane >> 4) * 4) = acc[hf][mt][h];
            }
    }
    ENC_SLOT();
    if (!late) ENC_SLOT();
    if (P.head_dim > 0) wide_head(P, acc, a0, B, (float *)buf_a);
    ENC_STAMP(9);
}
#define ENC_PP_KERNEL(n)                                                                                                                           \
    extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_pp##n##_kernel(const float *__restrict__ obs, int B, EncParams P,  \
                                                                                               float *__restrict__ out) {                         \
        pp_body<n, false>(obs, B, P, out);                                                                                                          \
    }                                                                                                                                               \
    extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_pp##n##o_kernel(const float *__restrict__ obs, int B, EncParams P, \
                                                                                                float *__restrict__ out) {                         \
        pp_body<n, true>(obs, B, P, out);                                                                                                           \
    }
ENC_PP_KERNEL(1) ENC_PP_KERNEL(2) ENC_PP_KERNEL(3)

// ------------------------------------------------------------------------------------------------
// attention, wide.  Launch 1: e_i -> ebuf, g = W_m e_mean -> gbuf (see qs_encoder_embed_kernel).
// ------------------------------------------------------------------------------------------------
template <int WNP>
__device__ __forceinline__ void embed_wide_body(const float *__restrict__ obs, int B, const EncParams &P) {
    constexpr int NT = WNP * ENC_AT;
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsEmbedWide Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_in = lds + Lds::x_in, *buf_a = lds + Lds::buf_a, *emean = lds + Lds::emean;
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, a0 = blockIdx.x * ENC_WA;
    const int NB = P.num_nbr, D = P.obs_dim, mt0 = wave * ENC_MT;
    const EncLayer none = {nullptr, nullptr, 0, 0};
    WRing R;
    ring_fill(R, P.n1, mt0);
    traj_copy(P, a0, ENC_WA, B);
    {
        const float invB = 1.0f / (float)B;
        const __amdgpu_buffer_rsrc_t ors = obs_rsrc(obs, B, D);
#pragma unroll 6
        // 18 iterations; neighbour slots past NB are zero rows
        for (int idx = tid; idx < ENC_WSLOTS * ENC_WA * 32; idx += 64 * ENC_WAVES) {
            const int row = idx >> 5, c = idx & 31, k = row / ENC_WA, a = row % ENC_WA, ga = a0 + a;
            // self_obs.repeat(K, 1)  (:84)
            const uint32_t i_self = mod_batch((uint32_t)ga * (uint32_t)NB + (uint32_t)k, (uint32_t)B, invB) * (uint32_t)D + c;
            const uint32_t i_nbr = (uint32_t)ga * (uint32_t)D + P.self_dim + k * P.nbr_dim + (c - P.self_dim);
            const float v = obs_at(ors, ga < B && k < NB && c < P.self_dim + P.nbr_dim, c < P.self_dim ? i_self : i_nbr);
            x_in[row * ENC_XS + c] = __builtin_bit_cast(uint16_t, (__bf16)v);
        }
    }
    __syncthreads();
    f32x4 mean[ENC_MT][ENC_AT];
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
        for (int h = 0; h < ENC_AT; ++h) mean[mt][h] = (f32x4){0, 0, 0, 0};
#pragma unroll 1
    for (int t0 = 0; t0 < NB; t0 += WNP) {
        const bool last = t0 + WNP >= NB;
        f32x4 acc[ENC_MT][NT];
        layer_ring<NT, 1>(R, P.n1, mt0, P.n2, mt0, x_in + t0 * ENC_WA * ENC_XS, ENC_XS, acc);
        if (t0) __syncthreads();   // the previous pass is done reading buf_a
        store_tanh_wide<NT>(acc, mt0, buf_a, ENC_YS);
        __syncthreads();
        layer_ring<NT, 8>(R, P.n2, mt0, last ? P.a1m : P.n1, mt0, buf_a, ENC_YS, acc);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int k = t0 + nt / ENC_AT, ga = a0 + (nt % ENC_AT) * 16 + (lane & 15);
            const bool live = k < NB;
#pragma unroll
            for (int mt = 0; mt < ENC_MT; ++mt) {
                bf16x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float e = fast_tanh(acc[mt][nt][r]); mean[mt][nt % ENC_AT][r] += live ? e : 0.0f;
                    v[r] = (__bf16)e; }
                if (live && ga < B) *(bf16x4 *)(P.ebuf + ((size_t)ga * NB + k) * ENC_H + (mt0 + mt) * 16 + (lane >> 4) * 4) = v;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const float inv = 1.0f / (float)NB;   // e_mean (:90-91), then its half of the score MLP's first layer once per agent
#pragma unroll
    for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
        for (int h = 0; h < ENC_AT; ++h) {
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (__bf16)(mean[mt][h][r] * inv);
            *(bf16x4 *)(emean + (h * 16 + (lane & 15)) * ENC_YS + (mt0 + mt) * 16 + (lane >> 4) * 4) = v;
        }
    __syncthreads();
    f32x4 g[ENC_MT][ENC_AT];
    zero_acc<ENC_MT, ENC_AT>(g);
    gemm_ring<ENC_AT, 8>(R, P.a1m, mt0, none, 0, emean, ENC_YS, g);
#pragma unroll
    for (int h = 0; h < ENC_AT; ++h) {
        const int ga = a0 + h * 16 + (lane & 15);
        if (ga < B) {
#pragma unroll
            for (int mt = 0; mt < ENC_MT; ++mt) *(f32x4 *)(P.gbuf + (size_t)ga * ENC_H + (mt0 + mt) * 16 + (lane >> 4) * 4) = g[mt][h];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// attention, wide.  Launch 2: groups of WNP neighbours (WNP * ENC_AT row tiles): score MLP, value MLP, online softmax (see attn_pass).
// ------------------------------------------------------------------------------------------------
struct AttnStateWide { f32x4 o[ENC_MT][ENC_AT]; float mx[ENC_AT], den[ENC_AT]; };

template <int WNP>
__device__ __forceinline__ void attn_wide_body(const float *__restrict__ obs, int B, const EncParams &P, float *__restrict__ out) {
    constexpr int NT = WNP * ENC_AT;
    extern __shared__ __align__(16) unsigned char smem[];
    typedef EncLdsAttnWide Lds;
    uint16_t *const lds = (uint16_t *)smem, *x_self = lds + Lds::x_self, *x_obst = lds + Lds::x_obst, *buf_a = lds + Lds::buf_a;
    uint16_t *buf_h = lds + Lds::buf_h, *cat = lds + Lds::cat;
    float *s_alpha = (float *)(lds + Lds::s_alpha);
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, a0 = blockIdx.x * ENC_WA;
    const int NB = P.num_nbr, D = P.obs_dim, mt0 = wave * ENC_MT;
    const bool obst = P.obst_dim > 0;
    const int col_nbr = ENC_H, col_obst = 2 * ENC_H;
    const float invB = 1.0f / (float)B;

    WRing R;
    ring_fill(R, P.s1, mt0);
    {
        const __amdgpu_buffer_rsrc_t ors = obs_rsrc(obs, B, D);
#pragma unroll
        for (int idx = tid; idx < 2 * ENC_WA * 32; idx += 64 * ENC_WAVES) {   // self and obstacle columns as bf16, zero padded to K = 32
            const int which = idx / (ENC_WA * 32), a = (idx >> 5) % ENC_WA, c = idx & 31, ga = a0 + a;
            const int dim = which ? P.obst_dim : P.self_dim, col = which ? P.self_dim + P.nbr_dim * NB : 0;
            const float v = obs_at(ors, ga < B && c < dim, (uint32_t)ga * (uint32_t)D + col + c);
            (which ? x_obst : x_self)[a * ENC_XS + c] = __builtin_bit_cast(uint16_t, (__bf16)v);
        }
    }
    __syncthreads();
    {
        f32x4 acc[ENC_MT][ENC_AT];
        layer_ring<ENC_AT, 1>(R, P.s1, mt0, P.s2, mt0, x_self, ENC_XS, acc);
        store_tanh_wide<ENC_AT>(acc, mt0, buf_h, ENC_YS);
        __syncthreads();
        layer_ring<ENC_AT, 8>(R, P.s2, mt0, obst ? P.o1 : P.a1e, mt0, buf_h, ENC_YS, acc);
        store_tanh_wide<ENC_AT>(acc, mt0, cat, ENC_CS, 0);
        if (obst) {
            layer_ring<ENC_AT, 1>(R, P.o1, mt0, P.o2, mt0, x_obst, ENC_XS, acc);
            __syncthreads();   // the self encoder's second layer is done reading buf_h
            store_tanh_wide<ENC_AT>(acc, mt0, buf_h, ENC_YS);
            __syncthreads();
            layer_ring<ENC_AT, 8>(R, P.o2, mt0, P.a1e, mt0, buf_h, ENC_YS, acc);
            store_tanh_wide<ENC_AT>(acc, mt0, cat, ENC_CS, col_obst);
        }
    }
    AttnStateWide st;
#pragma unroll
    for (int h = 0; h < ENC_AT; ++h) {
        st.mx[h] = -3.0e38f; st.den[h] = 0.0f;
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) st.o[mt][h] = (f32x4){0, 0, 0, 0};
    }
    const __amdgpu_buffer_rsrc_t ers = __builtin_amdgcn_make_buffer_rsrc((void *)P.ebuf, 0, (uint32_t)B * (uint32_t)NB * (ENC_H * 2),
        0x00020000);
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void *)P.gbuf, 0, (uint32_t)B * (ENC_H * 4), 0x00020000);
#pragma unroll 1
    for (int t0 = 0; t0 < NB; t0 += WNP) {
        const bool last = t0 + WNP >= NB;
        f32x4 acc[ENC_MT][NT];
        // score MLP, first layer on [e_i | e_mean.repeat(K, 1)]: W_e e_i + b + g[(a*K + k) mod B]   (:92-94): g seeds the accumulators
        // (issued first; it has landed by the time the e_i tile has made its round trip through the registers into LDS)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int k = t0 + nt / ENC_AT, ga = a0 + (nt % ENC_AT) * 16 + (lane & 15);
            const uint32_t j = mod_batch((uint32_t)ga * (uint32_t)NB + (uint32_t)k, (uint32_t)B, invB);
            // padding rows: out of range, reads zero
            const uint32_t off = (ga < B && k < NB) ? j * (ENC_H * 4) + (lane >> 4) * 16 : 0xffffffffu;
#pragma unroll
            for (int mt = 0; mt < ENC_MT; ++mt) acc[mt][nt] = __builtin_bit_cast(f32x4,
                __builtin_amdgcn_raw_buffer_load_b128(grs, off, (mt0 + mt) * 64, 0));
        }
        {   // e_i rows of the group in 16-byte chunks, coalesced
            constexpr int PER = NT * 16 * (ENC_H / 8) / (64 * ENC_WAVES);
            bf16x8 ev[PER];
#pragma unroll
            for (int it = 0; it < PER; ++it) {
                const int idx = tid + it * 64 * ENC_WAVES, row = idx >> 5, ch = idx & 31, k = t0 + row / ENC_WA, ra = a0 + row % ENC_WA;
                const uint32_t off = (ra < B && k < NB) ? ((uint32_t)ra * (uint32_t)NB + (uint32_t)k) * (ENC_H * 2) + ch * 16 : 0xffffffffu;
                ev[it] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ers, off, 0, 0));
            }
            if (t0) __syncthreads();   // the previous group's value layers are done with buf_a / buf_h
#pragma unroll
            for (int it = 0; it < PER; ++it) {
                const int idx = tid + it * 64 * ENC_WAVES, row = idx >> 5, ch = idx & 31;
                *(bf16x8 *)(buf_a + row * ENC_YS + ch * 8) = ev[it];
            }
        }
        const Bias b1 = load_bias(P.a1e, mt0);
        __syncthreads();   // e_i is in buf_a
        gemm_ring<NT, 8>(R, P.a1e, mt0, P.a2, mt0, buf_a, ENC_YS, acc);
        add_bias<NT>(acc, b1);
        store_tanh_wide<NT>(acc, mt0, buf_h, ENC_YS);
        __syncthreads();
        layer_ring<NT, 8>(R, P.a2, mt0, P.v1, mt0, buf_h, ENC_YS, acc);
        // last score layer 256 -> 1 straight from the accumulators (see attn_pass)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float sp = 0.0f;
#pragma unroll
            for (int mt = 0; mt < ENC_MT; ++mt) {
                const f32x4 w = *(const f32x4 *)(P.a3w + (mt0 + mt) * 16 + (lane >> 4) * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) sp += fast_tanh(acc[mt][nt][r]) * w[r];
            }
            sp = lane_groups_sum(sp);
            if (lane < 16) s_alpha[(wave * (3 * ENC_AT) + nt) * 16 + lane] = sp;
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();   // partial scores visible; every wave is done reading buf_h (second score layer)
        layer_ring<NT, 8>(R, P.v1, mt0, P.v2, mt0, buf_a, ENC_YS, acc);
        store_tanh_wide<NT>(acc, mt0, buf_h, ENC_YS);
        __syncthreads();
        layer_ring<NT, 8>(R, P.v2, mt0, last ? P.f : P.a1e, last ? wave * ENC_MTF : mt0, buf_h, ENC_YS, acc);
        // online softmax over the neighbours of agent (h, lane & 15)   (:95-100)
#pragma unroll
        for (int h = 0; h < ENC_AT; ++h) {
            float al[WNP], mx = st.mx[h];
#pragma unroll
            for (int j = 0; j < WNP; ++j) {
                al[j] = P.a3b;
#pragma unroll
                for (int w = 0; w < ENC_WAVES; ++w) al[j] += s_alpha[(w * (3 * ENC_AT) + j * ENC_AT + h) * 16 + (lane & 15)];
                if (t0 + j >= NB) al[j] = -3.0e38f;   // padded neighbour slot of the last group
                mx = fmaxf(mx, al[j]);
            }
            const float scale = __expf(st.mx[h] - mx);
            st.den[h] *= scale;
#pragma unroll
            for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) st.o[mt][h][r] *= scale;
#pragma unroll
            for (int j = 0; j < WNP; ++j) {
                const float e = t0 + j < NB ? __expf(al[j] - mx) : 0.0f;
                st.den[h] += e;
#pragma unroll
                for (int mt = 0; mt < ENC_MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) st.o[mt][h][r] += e * fast_tanh(acc[mt][j * ENC_AT + h][r]);
                __builtin_amdgcn_sched_barrier(0);
            }
            st.mx[h] = mx;
        }
    }
#pragma unroll
    for (int h = 0; h < ENC_AT; ++h) {
        const float rden = 1.0f / st.den[h];
#pragma unroll
        for (int mt = 0; mt < ENC_MT; ++mt) {
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (__bf16)(st.o[mt][h][r] * rden);
            *(bf16x4 *)(cat + (h * 16 + (lane & 15)) * ENC_CS + col_nbr + (mt0 + mt) * 16 + (lane >> 4) * 4) = v;
        }
    }
    __syncthreads();
    if (obst) feed_forward_wide<24>(R, P, cat, a0, B, out, (float *)buf_a);
    else feed_forward_wide<16>(R, P, cat, a0, B, out, (float *)buf_a);
}
#define ENC_WIDE_ATT_KERNELS(n)                                                                                                                        \
    extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_embed_wide##n##_kernel(const float *__restrict__ obs, int B, EncParams P) { \
        embed_wide_body<n>(obs, B, P);                                                                                                                 \
    }                                                                                                                                                  \
    extern "C" __global__ void __launch_bounds__(64 * ENC_WAVES, 2) qs_encoder_attn_wide##n##_kernel(const float *__restrict__ obs, int B, EncParams P,   \
                                                                                                      float *__restrict__ out) {                       \
        attn_wide_body<n>(obs, B, P, out);                                                                                                             \
    }
ENC_WIDE_ATT_KERNELS(1) ENC_WIDE_ATT_KERNELS(2) ENC_WIDE_ATT_KERNELS(3)

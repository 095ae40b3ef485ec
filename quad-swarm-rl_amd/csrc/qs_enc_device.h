// qs_enc_device.h - device pieces every body of qs_policy_encoder.hip shares: vector types, tanh, the fp16-pair split, observation loads,
// the GEMM on weight fragments (gemm_tiles), epilogues, the feed-forward layer with its fused head.  Included by that unit only, behind
// qs_enc_plan.h (tile constants, LDS layouts) and include/quadswarm_encoder.h (the parameter block).
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

#ifndef ENC_OCC
#define ENC_OCC 4     // waves per SIMD the register budget is set for: two workgroups per CU (<= 128 VGPRs)
#endif
#define ENC_MT (16 / ENC_WAVES)       // 16-feature tiles of a 256-wide layer per wave
#define ENC_MTF (32 / ENC_WAVES)      // ... of the 512-wide feed-forward layer

typedef qs_enc_layer EncLayer;     // K padded to a multiple of 32, M to a multiple of 16
typedef qs_enc_params EncParams;

// (rollout segments) reward / done of the previous control step -> trajectory, by the workgroup that owns the agents [a0, a0 + agents)
__device__ __forceinline__ void traj_copy(const EncParams &P, int a0, int agents, int B) {
    if (P.traj_rew_dst != nullptr) {
        const int a = a0 + (int)threadIdx.x;
        if ((int)threadIdx.x < agents && a < B) { P.traj_rew_dst[a] = P.traj_rew_src[a]; P.traj_done_dst[a] = P.traj_done_src[a]; }
    }
}

#ifdef ENC_TIMING   // phase stamps of workgroup 0, wave 0 (tools/enc_quick.py prints them)
__device__ unsigned long long enc_stamps[16];
__device__ unsigned long long enc_wg_times[2 * 8192];   // start / end of every workgroup on the constant 100 MHz clock
#define ENC_STAMP(k) do { if (threadIdx.x == 0) { if (blockIdx.x == 0) enc_stamps[k] = clock64(); \
                                                  if (((k) == 0 || (k) == 9) && blockIdx.x < 8192) enc_wg_times[2 * blockIdx.x + ((k) == 9)] = wall_clock64(); } } while (0)
#else
#define ENC_STAMP(k) do { } while (0)
#endif

__device__ __forceinline__ void glue_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
    uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// action = mean + exp(log_std) * N(0, 1) for component h of agent a: Box-Muller on the Philox group (agent, counter, 0x51, h / 4) - the
// values qs_rollout_pre_kernel draws (one group = two pairs = four components)
__device__ __forceinline__ float sample_action(const EncParams &P, int a, int h, float mean) {
    uint32_t w[4];
    glue_philox((uint32_t)a, *P.sample_counter + P.sample_step, 0x51u, (uint32_t)(h >> 2), P.sample_seed_lo, P.sample_seed_hi, w);
    const int pr = (h >> 1) & 1;
    const float ua = ((float)(w[2 * pr] >> 9) + 0.5f) * (1.0f / 8388608.0f),
        ub = ((float)(w[2 * pr + 1] >> 9) + 0.5f) * (1.0f / 8388608.0f);
    const float r = sqrtf(-2.0f * __logf(ua));
    float sn, cs;
    __sincosf(6.283185307179586f * ub, &sn, &cs);
    return mean + __expf(P.sample_log_std[h]) * r * ((h & 1) ? sn : cs);
}

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }   // in a scalar register

__device__ __forceinline__ float fast_tanh(float x) {   // 1 - 2 / (exp(2x) + 1); v_exp_f32 + v_rcp_f32
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);   // exp(2x): one multiply, v_exp_f32
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}
// The same on two values at once.  A wave issues one VALU instruction every ~5 cycles whatever it is (tools/ubench_valu.hip: v_fma_f32 6.6,
// v_pk_fma_f32 7.0, v_exp_f32 / v_rcp_f32 9-10 ticks per instruction for a wave alone, unchanged with a second wave on the SIMD), so
// the epilogues are bound by their instruction COUNT: the plain half of the tanh as v_pk_* (one issue per two values), and in
// tanh2_bias the bias add and the scale of the exponent in one v_pk_fma_f32:  2^(c (a + b)) with c = 2 log2(e) is 2^(a c + bc), bc = b c.
typedef __attribute__((ext_vector_type(2))) float f32x2;
#define ENC_TANH_C 2.8853900817779268f
__device__ __forceinline__ f32x2 tanh2_of_exponent(f32x2 t) {   // t = 2 log2(e) x
    f32x2 e = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
    e = e + (f32x2){1.0f, 1.0f};
    const f32x2 r = {__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
    return __builtin_elementwise_fma(r, (f32x2){-2.0f, -2.0f}, (f32x2){1.0f, 1.0f});
}
__device__ __forceinline__ f32x2 tanh2(f32x2 x) { return tanh2_of_exponent(x * (f32x2){ENC_TANH_C, ENC_TANH_C}); }
__device__ __forceinline__ f32x4 tanh4(const f32x4 &x) {
    const f32x2 lo = tanh2((f32x2){x[0], x[1]}), hi = tanh2((f32x2){x[2], x[3]});
    return (f32x4){lo.x, lo.y, hi.x, hi.y};
}
// tanh(a + b) with bc = {b * ENC_TANH_C}: one fused multiply-add instead of an add and a multiply
__device__ __forceinline__ f32x4 tanh4_bias(const f32x4 &a, const f32x4 &bc) {
    const f32x2 c = {ENC_TANH_C, ENC_TANH_C};
    const f32x2 lo = tanh2_of_exponent(__builtin_elementwise_fma((f32x2){a[0], a[1]}, c, (f32x2){bc[0], bc[1]}));
    const f32x2 hi = tanh2_of_exponent(__builtin_elementwise_fma((f32x2){a[2], a[3]}, c, (f32x2){bc[2], bc[3]}));
    return (f32x4){lo.x, lo.y, hi.x, hi.y};
}

// ------------------------------------------------------------------------------------------------
// Reference precision (qs_enc_params.precision = 1; template parameter SP of the 16-agent kernels).  The reference's modules run in
// fp32 (quad_multi_model.py:250-350); bf16 operands leave the fused features ~1e-2 away from them.  Here every operand of every GEMM -
// weight or activation - is the pair x = h + l / 2048 of fp16 numbers: h = fp16(x) carries 11 significant bits, l = fp16((x - h) * 2048)
// the next 11 (x - h is exact in fp32; the scale keeps l a normal fp16 number whatever the size of x).  A product becomes three
// v_mfma_f32_16x16x32_f16 - h.h into the accumulator, h.l and l.h into a second one that is folded in, times 1 / 2048, behind the K loop;
// the dropped l.l term and the roundings of the l halves are <= 2^-22 relative per product, i.e. fp32-grade.  Weights arrive split from
// the host (two 1 KiB planes per fragment), activations are kept as two planes ENC_SPLANE elements (qs_enc_plan.h) apart in LDS (and in `ebuf`).  The
// matrix cores do three times the work of the bf16 kernels, at a sixteenth of the price of the fp32 MFMA (v_mfma_f32_16x16x4_f32).
// Values below the smallest normal fp16 go into l alone (h = 0: no subnormal operand), values beyond +-65504 (no observation is) clamp.
// ------------------------------------------------------------------------------------------------
#define ENC_SPLIT_SCALE 2048.0f
__device__ __forceinline__ void split2(float x, _Float16 &h, _Float16 &l) {
    x = __builtin_amdgcn_fmed3f(x, -65504.0f, 65504.0f);
    h = __builtin_fabsf(x) < 6.103515625e-05f ? (_Float16)0.0f : (_Float16)x;
    l = (_Float16)((x - (float)h) * ENC_SPLIT_SCALE);
}
// one activation / four consecutive ones -> LDS (or `ebuf`): bf16, or the two fp16 planes `plane` elements apart
template <bool SP>
__device__ __forceinline__ void put1(uint16_t *p, float v) {
    if constexpr (SP) {
        _Float16 h, l;
        split2(v, h, l);
        p[0] = __builtin_bit_cast(uint16_t, h);
        p[ENC_SPLANE] = __builtin_bit_cast(uint16_t, l);
    } else p[0] = __builtin_bit_cast(uint16_t, (__bf16)v);
}
template <bool SP>
__device__ __forceinline__ void put4(uint16_t *p, const f32x4 &x, int plane = ENC_SPLANE) {
    if constexpr (SP) {
        f16x4 vh, vl;
#pragma unroll
        for (int r = 0; r < 4; ++r) { _Float16 h, l; split2(x[r], h, l); vh[r] = h; vl[r] = l; }
        *(f16x4 *)p = vh;
        *(f16x4 *)(p + plane) = vl;
    } else {
        bf16x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (__bf16)x[r];
        *(bf16x4 *)p = v;
    }
}

// floor(n / d) for small operands (n * d < 2^32) from m = ceil(2^32 / d), computed once per thread: integer division by a
// run-time divisor is ~40 instructions, and the staging loops did two per element
__device__ __forceinline__ uint32_t div_magic(uint32_t d) { return 0xffffffffu / d + 1u; }
__device__ __forceinline__ uint32_t div_by(uint32_t n, uint32_t magic) { return __umulhi(n, magic); }
// j mod B for j < 2^24 (the host bounds batch x neighbours): float estimate of the quotient, one correction step
__device__ __forceinline__ uint32_t mod_batch(uint32_t j, uint32_t B, float invB) {
    const uint32_t q = (uint32_t)((float)j * invB);
    int32_t r = (int32_t)(j - q * B);
    if (r < 0) r += (int32_t)B;
    else if (r >= (int32_t)B) r -= (int32_t)B;
    return (uint32_t)r;
}

// Observation elements through a buffer resource: an invalid element (padding column, row past the batch) gets an out-of-range
// offset and reads as zero, so the staging loops have no branch around their loads and issue them back to back (a conditional
// load per iteration is a branch plus s_waitcnt vmcnt(0): the memory latency once per element instead of once per loop).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t obs_rsrc(const float *obs, int B, int D) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)obs, 0, (uint32_t)B * (uint32_t)D * 4u, 0x00020000);
}
__device__ __forceinline__ float obs_at(__amdgpu_buffer_rsrc_t rs, bool valid, uint32_t index) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, valid ? index * 4u : 0xffffffffu, 0, 0));
}

// acc[mt][nt] (+)= W[features of (wave, mt)] x X[rows of tile nt], K-loop over the whole layer.  NT is a compile-time tile count
// and the steady-state loop has no conditional loads: a run-time bound puts a branch in front of every MFMA and LDS read (a lone
// pair of waves per SIMD pays for each of them) and makes the compiler drain the load counters every iteration.
// Weight fragments come from L2 and are software-pipelined ENC_PD K-steps ahead through a ring of register sets (the slot an
// MFMA group has just consumed is refilled with the fragment of K-step ks + ENC_PD); the activation fragment of a row tile is
// re-read from LDS for K-step ks + 1 as soon as its MFMAs of K-step ks are issued.
#define ENC_PD 4
#define ENC_WLOAD(x) (x)
template <int MT, int NT>
__device__ __forceinline__ void mfma_tile(const bf16x8 (&a)[MT], const bf16x8 &b, f32x4 (&acc)[MT][NT], int nt) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], b, acc[mt][nt], 0, 0, 0);
}

// reference precision (see split2): A fragments in two planes per (tile, K-step), B fragments in two LDS planes, three MFMAs per product
template <int MT, int NT>
__device__ __forceinline__ void gemm_tiles_split(const EncLayer &L, int mtile0, const uint16_t *X, int xstride, f32x4 (&acc)[MT][NT]) {
    const int lane = threadIdx.x & 63, ksteps = L.K >> 5;
    const uint16_t *xrow = X + (lane & 15) * xstride + 8 * (lane >> 4);
    const uint32_t voff = lane * 16;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void *)L.w, 0, L.M * L.K * 4, 0x00020000);
#define ENC_SW(mt, ks, pl) __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, voff, (((mtile0 + (mt)) * ksteps + (ks)) * 2 + (pl)) * 1024, 0))
#define ENC_SX(nt, ks, pl) (*(const f16x8 *)(xrow + (pl) * ENC_SPLANE + (nt) * 16 * xstride + (ks) * 32))
    f32x4 lo[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) lo[mt][nt] = (f32x4){0, 0, 0, 0};
    // one K-step of every tile: h.h for all tiles first, then the two cross terms - consecutive MFMAs never share an accumulator
#define ENC_SSTEP(AH, AL, BH, BL)                                                                                        \
    do {                                                                                                                  \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                                                 \
            _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                             \
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16((AH)[mt], (BH)[nt], acc[mt][nt], 0, 0, 0);           \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                                                 \
            _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                             \
                lo[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16((AH)[mt], (BL)[nt], lo[mt][nt], 0, 0, 0);             \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                                                 \
            _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                                             \
                lo[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16((AL)[mt], (BH)[nt], lo[mt][nt], 0, 0, 0);             \
    } while (0)
    f16x8 bh[NT], bl[NT];
    if (ksteps & (ENC_PD - 1)) {   // the 32- and 64-wide input layers
        for (int ks = 0; ks < ksteps; ++ks) {
            f16x8 ah[MT], al[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) { ah[mt] = ENC_SW(mt, ks, 0); al[mt] = ENC_SW(mt, ks, 1); }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { bh[nt] = ENC_SX(nt, ks, 0); bl[nt] = ENC_SX(nt, ks, 1); }
            ENC_SSTEP(ah, al, bh, bl);
        }
    } else {
        f16x8 ah[ENC_PD][MT], al[ENC_PD][MT];   // weight ring, ENC_PD K-steps ahead (as in gemm_tiles)
#pragma unroll
        for (int s = 0; s < ENC_PD; ++s)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) { ah[s][mt] = ENC_SW(mt, s, 0); al[s][mt] = ENC_SW(mt, s, 1); }
        int ks0 = 0;
        for (; ks0 + ENC_PD < ksteps; ks0 += ENC_PD) {
#pragma unroll
            for (int s = 0; s < ENC_PD; ++s) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) { bh[nt] = ENC_SX(nt, ks0 + s, 0); bl[nt] = ENC_SX(nt, ks0 + s, 1); }
                ENC_SSTEP(ah[s], al[s], bh, bl);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) { ah[s][mt] = ENC_SW(mt, ks0 + s + ENC_PD, 0); al[s][mt] = ENC_SW(mt, ks0 + s + ENC_PD, 1); }
            }
        }
#pragma unroll
        for (int s = 0; s < ENC_PD; ++s) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { bh[nt] = ENC_SX(nt, ks0 + s, 0); bl[nt] = ENC_SX(nt, ks0 + s, 1); }
            ENC_SSTEP(ah[s], al[s], bh, bl);
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[mt][nt][r] += lo[mt][nt][r] * (1.0f / ENC_SPLIT_SCALE);
#undef ENC_SSTEP
#undef ENC_SX
#undef ENC_SW
}

template <int MT, int NT, bool SP = false>
__device__ __forceinline__ void gemm_tiles(const EncLayer &L, int mtile0, const uint16_t *X, int xstride, f32x4 (&acc)[MT][NT]) {
    if constexpr (SP) { gemm_tiles_split<MT, NT>(L, mtile0, X, xstride, acc); return; }
    const int lane = threadIdx.x & 63, ksteps = L.K >> 5;
    const uint16_t *xrow = X + (lane & 15) * xstride + 8 * (lane >> 4);
    // fragment address = buffer resource of the layer (scalar registers) + wave-uniform scalar offset (mtile0 is uniform) + one
    // per-lane byte offset shared by every layer: no per-layer 64-bit address pairs in vector registers
    const uint32_t voff = lane * 16;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void *)L.w, 0, L.M * L.K * 2, 0x00020000);
#define ENC_WFRAG(mt, ks) ENC_WLOAD(__builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, voff, ((mtile0 + (mt)) * ksteps + (ks)) * 1024, 0)))
#define ENC_XFRAG(nt, ks) (*(const bf16x8 *)(xrow + (nt) * 16 * xstride + (ks) * 32))
    if (ksteps & (ENC_PD - 1)) {   // the 32- and 64-wide input layers: one or two K-steps, nothing to pipeline
        for (int ks = 0; ks < ksteps; ++ks) {
            bf16x8 a[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[mt] = ENC_WFRAG(mt, ks);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) mfma_tile<MT, NT>(a, ENC_XFRAG(nt, ks), acc, nt);
        }
        return;
    }
    bf16x8 a[ENC_PD][MT], b[NT];
#pragma unroll
    for (int s = 0; s < ENC_PD; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[s][mt] = ENC_WFRAG(mt, s);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b[nt] = ENC_XFRAG(nt, 0);
    int ks0 = 0;
    for (; ks0 + ENC_PD < ksteps; ks0 += ENC_PD) {   // steady state: every load unconditional, so the wait counters stay exact
#pragma unroll
        for (int s = 0; s < ENC_PD; ++s) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                mfma_tile<MT, NT>(a[s], b[nt], acc, nt);
                b[nt] = ENC_XFRAG(nt, ks0 + s + 1);   // this row tile's fragment is consumed: refill it while the other tiles' MFMAs run
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[s][mt] = ENC_WFRAG(mt, ks0 + s + ENC_PD);
        }
    }
#pragma unroll
    for (int s = 0; s < ENC_PD; ++s)   // the last ENC_PD K-steps: their weights are already in flight
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            mfma_tile<MT, NT>(a[s], b[nt], acc, nt);
            if (s + 1 < ENC_PD) b[nt] = ENC_XFRAG(nt, ks0 + s + 1);
        }
}

template <int MT, int NT>
__device__ __forceinline__ void init_bias(const EncLayer &L, int mtile0, f32x4 (&acc)[MT][NT]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const f32x4 bias = *(const f32x4 *)(L.b + (mtile0 + mt) * 16 + (lane >> 4) * 4);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = bias;
    }
}

// tanh, bf16, store: lane holds features f0..f0+3 of row (nt*16 + lane&15)
template <int MT, int NT, bool SP = false>
__device__ __forceinline__ void store_tanh(const f32x4 (&acc)[MT][NT], int mtile0, uint16_t *Y, int ystride, int col0 = 0) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            f32x4 t;
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = fast_tanh(acc[mt][nt][r]);
            put4<SP>(Y + (nt * 16 + (lane & 15)) * ystride + col0 + (mtile0 + mt) * 16 + (lane >> 4) * 4, t);
        }
}

// one 16-row MLP: Y[:, col0:col0+256] = tanh(L2 tanh(L1 X)), hidden layer through `hid` (one barrier inside)
template <bool SP = false>
__device__ __forceinline__ void mlp2_one_tile(const EncLayer &L1, const EncLayer &L2, int mt0, const uint16_t *X, int xstride,
    uint16_t *hid,
                                              uint16_t *Y, int ystride, int col0) {
    f32x4 acc[ENC_MT][1];
    init_bias<ENC_MT, 1>(L1, mt0, acc);
    gemm_tiles<ENC_MT, 1, SP>(L1, mt0, X, xstride, acc);
    store_tanh<ENC_MT, 1, SP>(acc, mt0, hid, ENC_YS);
    __syncthreads();
    init_bias<ENC_MT, 1>(L2, mt0, acc);
    gemm_tiles<ENC_MT, 1, SP>(L2, mt0, hid, ENC_YS, acc);
    store_tanh<ENC_MT, 1, SP>(acc, mt0, Y, ystride, col0);
}

__device__ __forceinline__ float lane_groups_sum(float v) {   // sum over the 4 lane groups that hold the same row (lane & 15)
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// feed forward: tanh(F [self | neighbourhood | obstacles]) -> out[a][0:512] (fp32)   (:329-332, :349), and optionally a linear
// head on it (Sample Factory's action-parameter or value layer, 512 -> head_dim <= 8) so that a rollout does not have to write
// and re-read the features: per-lane partial dot products, two shuffles over the lane groups, the eight waves through `red`
// (LDS scratch, >= ENC_WAVES * 8 * 16 floats in a buffer nobody reads any more and that is not `cat`).
template <int MTF = ENC_MTF, bool SP = false>   // 16-feature tiles per wave: 512 outputs = 32 tiles; the Sim2Real encoder's 256 = 16 tiles
__device__ __forceinline__ void feed_forward(const EncParams &P, const uint16_t *cat, int a0, int B, float *__restrict__ out, float *red) {
    const int wave = wave_id(), lane = threadIdx.x & 63;
    constexpr int OUT = MTF * ENC_WAVES * 16;
    f32x4 acc[MTF][1];
    const int mf0 = wave * MTF;
    init_bias<MTF, 1>(P.f, mf0, acc);
    gemm_tiles<MTF, 1, SP>(P.f, mf0, cat, ENC_CS, acc);
    ENC_STAMP(8);
    const int ga = a0 + (lane & 15);
    f32x4 v[MTF];
#pragma unroll
    for (int mt = 0; mt < MTF; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[mt][r] = fast_tanh(acc[mt][0][r]);
        if (out && ga < B) *(f32x4 *)(out + (size_t)ga * OUT + (mf0 + mt) * 16 + (lane >> 4) * 4) = v[mt];
    }
    if (P.head_dim > 0) {
        for (int h = 0; h < P.head_dim; ++h) {
            float s = 0.0f;
#pragma unroll
            for (int mt = 0; mt < MTF; ++mt) {
                const f32x4 w = *(const f32x4 *)(P.head_w + h * OUT + (mf0 + mt) * 16 + (lane >> 4) * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) s += v[mt][r] * w[r];
            }
            s = lane_groups_sum(s);
            if (lane < 16) red[(wave * 8 + h) * 16 + lane] = s;
        }
        __syncthreads();
        const int tid = threadIdx.x, h = tid >> 4, row = tid & 15;
        if (h < P.head_dim && a0 + row < B) {
            float s = P.head_b[h];
#pragma unroll
            for (int w = 0; w < ENC_WAVES; ++w) s += red[(w * 8 + h) * 16 + row];
            P.head_out[(size_t)(a0 + row) * P.head_dim + h] = s;
            if (P.sample_log_std) P.act_out[(size_t)(a0 + row) * P.head_dim + h] = sample_action(P, a0 + row, h, s);
        }
    }
}

// run CALL(<tile count>) for min(n, LIMIT) tiles; only the counts a pass size of LIMIT can see are instantiated
#define ENC_CASE_NT(k, LIMIT, CALL) case k: if constexpr (k <= (LIMIT)) { CALL(k); } break;
#define ENC_DISPATCH_NT(n, LIMIT, CALL)                                        \
    switch ((n) < (LIMIT) ? (n) : (LIMIT)) {                                   \
        ENC_CASE_NT(1, LIMIT, CALL) ENC_CASE_NT(2, LIMIT, CALL) ENC_CASE_NT(3, LIMIT, CALL) ENC_CASE_NT(4, LIMIT, CALL) \
        ENC_CASE_NT(5, LIMIT, CALL) ENC_CASE_NT(6, LIMIT, CALL) ENC_CASE_NT(7, LIMIT, CALL) ENC_CASE_NT(8, LIMIT, CALL) \
    default: break;                                                            \
    }

// qs_enc_narrow_plan.h - what the HOST decides about a forward pass of the Sim2Real encoder at the deployable widths (H = rnn_size = 16, 32,
// 64; the kernels are csrc/qs_enc_narrow.inc), in plain C++17 without HIP: which widths are narrow, whether the layers of a parameter block
// agree on one width, agents per workgroup, the grid and the LDS bytes.  tests/test_narrow_plan_cpu.py compiles this header alone with the
// host compiler.  The width is read from params->s1.M: nothing in qs_enc_params names it.
#ifndef QS_ENC_NARROW_PLAN_H
#define QS_ENC_NARROW_PLAN_H
#include <initializer_list>

#include "../../include/quadswarm_encoder.h"

#define ENC_NW_AGENTS 16     // agents per wave: the N dimension of one 16x16x32 MFMA
#define ENC_NW_XS 72         // row stride (fp16 elements) of a wave's LDS slice: 64 columns + 8 (spreads the banks)
#ifndef ENC_NW_WAVES
#define ENC_NW_WAVES 1       // waves per workgroup, a build-time constant: 1 measured faster than 4 at 8192 agents (DESIGN.md 10 has both times)
#endif

// QS_ENC_MODEL_S2R with 0 < s1.M < 256 goes to the narrow kernels; of those widths these are built
inline bool enc_narrow_route(int model, int width) { return model == QS_ENC_MODEL_S2R && width > 0 && width < 256; }
inline bool enc_narrow_width(int width) { return width == 16 || width == 32 || width == 64; }
inline int enc_narrow_ceil32(int n) { return (n + 31) / 32 * 32; }

// every layer has M = H; the attention block's projections have K = ceil32(H), the feed-forward layer K = ceil32(3 H)
inline bool enc_narrow_consistent(const qs_enc_params &P) {
    const int H = P.s1.M, kh = enc_narrow_ceil32(H);
    for (const qs_enc_layer *L : {&P.s1, &P.n1, &P.o1, &P.mq, &P.mk, &P.mv, &P.mfc, &P.f})
        if (L->M != H) return false;
    for (const qs_enc_layer *L : {&P.mq, &P.mk, &P.mv, &P.mfc})
        if (L->K != kh) return false;
    return P.f.K == enc_narrow_ceil32(3 * H);
}

// one wave owns 16 agents from observation row to output row; a workgroup is `waves` of them with nothing shared
inline int enc_narrow_agents(int waves) { return ENC_NW_AGENTS * waves; }
inline int enc_narrow_grid(int B, int waves) { return (B + enc_narrow_agents(waves) - 1) / enc_narrow_agents(waves); }
// static LDS: per wave one [16][ENC_NW_XS] slice in two fp16 planes - the scratch through which a layer's accumulators become the next layer's B operand
inline int enc_narrow_lds_bytes(int waves) { return waves * 2 * ENC_NW_AGENTS * ENC_NW_XS * 2; }

#endif

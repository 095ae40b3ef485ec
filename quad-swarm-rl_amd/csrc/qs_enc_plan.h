// qs_enc_plan.h - what the HOST decides about a forward pass of the policy encoder (qs_policy_encoder.hip), in plain C++17 without HIP:
// the tile and stride constants, the LDS layout of every kernel body, the list of the encoder kernels, and the rule that picks the
// kernels of a forward pass.  The device bodies take their `smem` pointers from the layouts below and the launch asks for the same
// layout's end; tests/test_enc_select.py compiles this header alone with the host compiler.
#ifndef QS_ENC_PLAN_H
#define QS_ENC_PLAN_H
#include "../../include/quadswarm_encoder.h"

#define ENC_H 256            // hidden size of every MLP (rnn_size = neighbor_hidden_size = obst_hidden_size = 256)
#define ENC_TA 16            // agents per workgroup = one 16-row tile
#define ENC_MAX_NBR 8        // neighbours per agent (6 or 2 in the reference's configurations)
#ifndef ENC_NH
#define ENC_NH (ENC_MAX_NBR / 2)   // neighbour row tiles per pass of the neighbour MLP
#endif
#ifndef ENC_ANH
#define ENC_ANH 3            // ... per group of the attention kernel (attn_pass)
#endif
#ifndef ENC_WAVES
// 2 waves per SIMD: the layer chain of one workgroup is latency-bound, a second wave hides part of it (49 -> 40 us at 8192 agents)
#define ENC_WAVES 8
#endif
#define ENC_XS 40            // row stride (bf16) of the 32-wide input staging rows  (+8 pad: spreads the LDS banks)
#define ENC_YS (ENC_H + 8)   // row stride of a 256-wide activation buffer
#define ENC_CS (3 * ENC_H + 8)
#define ENC_XW 72            // row stride of the mlp neighbour encoder's input rows (all neighbours of one agent, K padded to 64)
#define ENC_OS (4 * ENC_H + 8)   // row stride of the concatenated-heads buffer
// the 32-agent kernels
#define ENC_AT 2                    // agent tiles per workgroup
#define ENC_WA (16 * ENC_AT)        // agents per workgroup
#define ENC_WSLOTS (ENC_MAX_NBR + 1)   // neighbour slots in the staging rows: ceil(8 / 3) * 3

// ------------------------------------------------------------------------------------------------
// LDS layouts: offsets in uint16_t elements from the start of `smem`, `end` = the first element behind the layout, `bytes` = what the
// launch asks for.  Buffers are [rows][row stride]; a float scratch area takes two elements per float.
// ------------------------------------------------------------------------------------------------
struct EncLdsMain {        // main_body: mean_embed / mlp / no_encoder, 16 agents
    static constexpr int x_self = 0;                                       // [16][XS]
    static constexpr int x_nbr = x_self + ENC_TA * ENC_XS;                 // [NBR*16][XS]
    static constexpr int x_obst = x_nbr + ENC_MAX_NBR * ENC_TA * ENC_XS;   // [16][XS]
    static constexpr int buf_a = x_obst + ENC_TA * ENC_XS;                 // [NH*16][YS]  hidden layer of the neighbour MLP (one pass at a time)
    static constexpr int buf_b = buf_a + ENC_NH * ENC_TA * ENC_YS;         // [16][YS]     hidden layer of the self / obstacle MLPs
    static constexpr int cat = buf_b + ENC_TA * ENC_YS;                    // [16][CS]: self | neighbourhood | obstacles
    static constexpr int end = cat + ENC_TA * ENC_CS, bytes = 2 * end;
};
struct EncLdsEmbed {       // embed_body: attention, launch 1
    static constexpr int x_in = 0;                                         // [NBR*16][XS]
    static constexpr int buf_a = x_in + ENC_MAX_NBR * ENC_TA * ENC_XS;     // [NH*16][YS]
    static constexpr int emean = buf_a + ENC_NH * ENC_TA * ENC_YS;         // [16][YS]
    static constexpr int end = emean + ENC_TA * ENC_YS, bytes = 2 * end;
};
struct EncLdsAttn {        // attn_body: attention, launch 2
    static constexpr int x_self = 0;                                       // [16][XS]
    static constexpr int x_obst = x_self + ENC_TA * ENC_XS;                // [16][XS]
    static constexpr int buf_a = x_obst + ENC_TA * ENC_XS;                 // [ANH*16][YS]  e_i of the group, later the second score layer
    static constexpr int buf_h = buf_a + ENC_ANH * ENC_TA * ENC_YS;        // [ANH*16][YS]  hidden layers; first the self / obstacle MLPs' (one tile)
    static constexpr int cat = buf_h + ENC_ANH * ENC_TA * ENC_YS;          // [16][CS]: self | neighbourhood | obstacles
    static constexpr int s_alpha = cat + ENC_TA * ENC_CS;                  // float [8 waves][ANH][16] partial scores of the group
    static constexpr int end = s_alpha + 2 * ENC_WAVES * ENC_ANH * 16, bytes = 2 * end;
};
struct EncLdsMha {         // mha_body: multi-head / Sim2Real
    static constexpr int x_self = 0;                                       // [16][XS]
    static constexpr int x_obst = x_self + ENC_TA * ENC_XS;                // [16][XS]
    static constexpr int x_nbr = x_obst + ENC_TA * ENC_XS;                 // [16][XW]  all neighbour columns of the agent, K padded to 64
    static constexpr int hid = x_nbr + ENC_TA * ENC_XW;                    // [16][YS]  hidden layer of the three MLPs
    static constexpr int tok = hid + ENC_TA * ENC_YS;                      // [2][16][YS]  tokens: neighbour embedding, obstacle embedding
    static constexpr int obuf = tok + 2 * ENC_TA * ENC_YS;                 // [2][16][OS]  attention output, heads concatenated
    static constexpr int cat = obuf + 2 * ENC_TA * ENC_OS;                 // [16][CS]: self | token 0 | token 1
    static constexpr int red_s = cat + ENC_TA * ENC_CS;                    // float [4 heads][2 waves][4 (i,j)][16]  partial scores
    static constexpr int red_ln = red_s + 2 * (4 * 2 * 4 * 16);            // float [8 waves][2 tokens][2 (sum, sum of squares)][16]
    static constexpr int end = red_ln + 2 * (ENC_WAVES * 2 * 2 * 16), bytes = 2 * end;
};
// Reference precision: every 16-agent layout twice, the h plane and ENC_SPLANE elements behind it the l plane; one plane is the largest
// of those layouts (main_body's).  The attention kernel's partial scores sit behind both planes.
constexpr int ENC_SPLANE = EncLdsMain::end;
struct EncLdsSplit {
    static constexpr int s_alpha = 2 * ENC_SPLANE;
    static constexpr int bytes = 2 * s_alpha, bytes_scores = bytes + 4 * ENC_WAVES * ENC_ANH * 16;
};
// mha_body_split, inside one plane: two planes leave room for ONE token's concatenated heads; the inputs and the MLPs' hidden layer share
// their space with that buffer (dead before it is written), the reduction scratch sits behind it in the h plane
struct EncLdsMhaSplit {
    static constexpr int tok = 0;                                          // [2][16][YS]
    static constexpr int cat = tok + 2 * ENC_TA * ENC_YS;                  // [16][CS]
    static constexpr int obuf = cat + ENC_TA * ENC_CS;                     // [16][OS]  attention output of ONE query token, heads concatenated
    static constexpr int x_self = obuf;                                    // [16][XS]
    static constexpr int x_obst = x_self + ENC_TA * ENC_XS;                // [16][XS]
    static constexpr int x_nbr = x_obst + ENC_TA * ENC_XS;                 // [16][XW]
    static constexpr int hid = x_nbr + ENC_TA * ENC_XW;                    // [16][YS]
    static constexpr int red_s = obuf + ENC_TA * ENC_OS;                   // float, as in EncLdsMha
    static constexpr int red_ln = red_s + 2 * (4 * 2 * 4 * 16);
    static constexpr int end = red_ln + 2 * (ENC_WAVES * 2 * 2 * 16);
};
static_assert(EncLdsAttn::s_alpha <= ENC_SPLANE && EncLdsEmbed::end <= ENC_SPLANE && EncLdsMhaSplit::end <= ENC_SPLANE,
              "ENC_SPLANE holds one plane of every 16-agent layout");
static_assert(EncLdsMhaSplit::hid + ENC_TA * ENC_YS <= EncLdsMhaSplit::red_s, "inputs + hidden layer fit under the heads buffer");
static_assert(EncLdsSplit::bytes_scores <= 160 * 1024, "two planes fit a CU's LDS");

struct EncLdsWide {        // wide_body, pp_body: mean_embed, 32 agents
    static constexpr int x_self = 0;                                       // [WA][XS]
    static constexpr int x_nbr = x_self + ENC_WA * ENC_XS;                 // [WSLOTS*WA][XS]
    static constexpr int x_obst = x_nbr + ENC_WSLOTS * ENC_WA * ENC_XS;    // [WA][XS]
    static constexpr int buf_a = x_obst + ENC_WA * ENC_XS;                 // [3*WA][YS]   hidden layer of the neighbour MLP (one pass / group at a time)
    static constexpr int buf_b = buf_a + 3 * ENC_WA * ENC_YS;              // [WA][YS]     hidden layer of the self / obstacle MLPs
    static constexpr int cat = buf_b + ENC_WA * ENC_YS;                    // [WA][CS]: self | neighbourhood | obstacles
    static constexpr int end = cat + ENC_WA * ENC_CS, bytes = 2 * end;
};
struct EncLdsEmbedWide {   // embed_wide_body
    static constexpr int x_in = 0;                                         // [WSLOTS*WA][XS]
    static constexpr int buf_a = x_in + ENC_WSLOTS * ENC_WA * ENC_XS;      // [3*WA][YS]
    static constexpr int emean = buf_a + 3 * ENC_WA * ENC_YS;              // [WA][YS]
    static constexpr int end = emean + ENC_WA * ENC_YS, bytes = 2 * end;
};
struct EncLdsAttnWide {    // attn_wide_body
    static constexpr int x_self = 0;                                       // [WA][XS]
    static constexpr int x_obst = x_self + ENC_WA * ENC_XS;                // [WA][XS]
    static constexpr int buf_a = x_obst + ENC_WA * ENC_XS;                 // [3*WA][YS]  e_i of the group
    static constexpr int buf_h = buf_a + 3 * ENC_WA * ENC_YS;              // [3*WA][YS]  hidden layers; first the self / obstacle MLPs'
    static constexpr int cat = buf_h + 3 * ENC_WA * ENC_YS;                // [WA][CS]: self | neighbourhood | obstacles
    static constexpr int s_alpha = cat + ENC_WA * ENC_CS;                  // float [8 waves][3*AT tiles][16] partial scores of the group
    static constexpr int end = s_alpha + 2 * ENC_WAVES * 3 * ENC_AT * 16, bytes = 2 * end;
};

// ------------------------------------------------------------------------------------------------
// The encoder kernels, once: X(symbol, dynamic LDS bytes, agents per workgroup, takes `out`).  The unit expands the list into its table of
// function pointers (attribute loop, launch routine); a row's index is ENC_K(<middle of the symbol>).  Rows that differ in the
// neighbours per pass (1, 2, 3) are consecutive: enc_select indexes them from the first.
// ------------------------------------------------------------------------------------------------
#define ENC_KERNELS(X)                                                          \
    X(qs_encoder_kernel, EncLdsMain::bytes, ENC_TA, 1)                          \
    X(qs_encoder_embed_kernel, EncLdsEmbed::bytes, ENC_TA, 0)                   \
    X(qs_encoder_attn_kernel, EncLdsAttn::bytes, ENC_TA, 1)                     \
    X(qs_encoder_mha_kernel, EncLdsMha::bytes, ENC_TA, 1)                       \
    X(qs_encoder_s2r_kernel, EncLdsMha::bytes, ENC_TA, 1)                       \
    X(qs_encoder_split_kernel, EncLdsSplit::bytes, ENC_TA, 1)                   \
    X(qs_encoder_embed_split_kernel, EncLdsSplit::bytes, ENC_TA, 0)             \
    X(qs_encoder_attn_split_kernel, EncLdsSplit::bytes_scores, ENC_TA, 1)       \
    X(qs_encoder_mha_split_kernel, EncLdsSplit::bytes, ENC_TA, 1)               \
    X(qs_encoder_s2r_split_kernel, EncLdsSplit::bytes, ENC_TA, 1)               \
    X(qs_encoder_wide1_kernel, EncLdsWide::bytes, ENC_WA, 1)                    \
    X(qs_encoder_wide2_kernel, EncLdsWide::bytes, ENC_WA, 1)                    \
    X(qs_encoder_wide3_kernel, EncLdsWide::bytes, ENC_WA, 1)                    \
    X(qs_encoder_pp1_kernel, EncLdsWide::bytes, ENC_WA, 1)                      \
    X(qs_encoder_pp2_kernel, EncLdsWide::bytes, ENC_WA, 1)                      \
    X(qs_encoder_pp3_kernel, EncLdsWide::bytes, ENC_WA, 1)                      \
    X(qs_encoder_pp1o_kernel, EncLdsWide::bytes, ENC_WA, 1)                     \
    X(qs_encoder_pp2o_kernel, EncLdsWide::bytes, ENC_WA, 1)                     \
    X(qs_encoder_pp3o_kernel, EncLdsWide::bytes, ENC_WA, 1)                     \
    X(qs_encoder_embed_wide1_kernel, EncLdsEmbedWide::bytes, ENC_WA, 0)         \
    X(qs_encoder_embed_wide2_kernel, EncLdsEmbedWide::bytes, ENC_WA, 0)         \
    X(qs_encoder_embed_wide3_kernel, EncLdsEmbedWide::bytes, ENC_WA, 0)         \
    X(qs_encoder_attn_wide1_kernel, EncLdsAttnWide::bytes, ENC_WA, 1)           \
    X(qs_encoder_attn_wide2_kernel, EncLdsAttnWide::bytes, ENC_WA, 1)           \
    X(qs_encoder_attn_wide3_kernel, EncLdsAttnWide::bytes, ENC_WA, 1)

struct EncKernel { const void *fn; const char *name; int lds_bytes, agents, has_out; };
#define ENC_KERNEL_INDEX(sym, lds, agents, has_out) ENC_K_##sym,
enum { ENC_KERNELS(ENC_KERNEL_INDEX) ENC_NUM_KERNELS };
#undef ENC_KERNEL_INDEX
#define ENC_K(middle) ENC_K_qs_encoder##middle##_kernel
static_assert(ENC_K(_wide3) == ENC_K(_wide1) + 2 && ENC_K(_pp3) == ENC_K(_pp1) + 2 && ENC_K(_pp3o) == ENC_K(_pp1o) + 2 &&
              ENC_K(_embed_wide3) == ENC_K(_embed_wide1) + 2 && ENC_K(_attn_wide3) == ENC_K(_attn_wide1) + 2, "variants 1, 2, 3 in a row");

// ------------------------------------------------------------------------------------------------
// The kernels of one forward pass, in launch order (rows of ENC_KERNELS); each runs on ceil(B / agents of its row) workgroups.
// `wide_min`: batches from this many agents on take the 32-agent workgroups (0: never); `pingpong`: pp_body instead of wide_body where
// it is built (2, 4, 5, 6 neighbours).  Both are measured product decisions (tools/enc_threshold.sh, tools/enc_pp_ab.sh).
// ------------------------------------------------------------------------------------------------
struct EncPlan { int n; int kernel[2]; };
inline EncPlan enc_select(int model, int num_nbr, int obst_dim, int precision, int B, int wide_min, int pingpong) {
    const bool att = model == QS_ENC_NBR_ATTENTION && num_nbr > 0, s2r = model == QS_ENC_MODEL_S2R, mha = model == QS_ENC_MODEL_MHA || s2r;
    if (precision == 1) {   // reference precision: the 16-agent bodies on fp16 pairs, one workgroup per CU (two LDS planes)
        if (s2r) return {1, {ENC_K(_s2r_split)}};
        if (mha) return {1, {ENC_K(_mha_split)}};
        if (att) return {2, {ENC_K(_embed_split), ENC_K(_attn_split)}};
        return {1, {ENC_K(_split)}};
    }
    if (wide_min > 0 && B >= wide_min && num_nbr > 0 && (model == QS_ENC_NBR_MEAN_EMBED || att)) {
        // neighbours per pass: the fewest padded neighbour slots, then the fewest passes (1 -> 1; 2, 4 -> 2; 3, 5, 6, 7, 8 -> 3)
        const int w = num_nbr == 1 ? 1 : (num_nbr == 2 || num_nbr == 4) ? 2 : 3;
        if (att) return {2, {ENC_K(_embed_wide1) + w - 1, ENC_K(_attn_wide1) + w - 1}};
        // two groups of ceil(K / 2) neighbours, the two waves of a SIMD half a layer apart (pp_body)
        if (pingpong && (num_nbr == 2 || (num_nbr >= 4 && num_nbr <= 6)))
            return {1, {(obst_dim > 0 ? ENC_K(_pp1o) : ENC_K(_pp1)) + (num_nbr + 1) / 2 - 1}};
        return {1, {ENC_K(_wide1) + w - 1}};
    }
    if (s2r) return {1, {ENC_K(_s2r)}};
    if (mha) return {1, {ENC_K(_mha)}};
    if (att) return {2, {ENC_K(_embed), ENC_K(_attn)}};
    return {1, {ENC_K()}};   // mean_embed, mlp, no_encoder, attention without neighbours
}

#endif

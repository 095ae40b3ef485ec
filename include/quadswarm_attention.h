/*
 * quadswarm_attention.h - C ABI of the attention probe: the attention weights a policy encoder computes on its observation rows.
 * Exported by libquadswarm_encoder.so; qs_enc_params is that of quadswarm_encoder.h.
 *
 * Reference: three encoder classes of swarm_rl/models/quad_multi_model.py decide by attention what an agent looks at -
 * QuadNeighborhoodEncoderAttention (:44-101, a softmax over the K neighbour slots), QuadMultiHeadAttentionEncoder (:124-196, 4 heads
 * over the token pair [neighbour embedding, obstacle embedding]) and QuadSingleHeadAttentionEncoder_Sim2Real (:199-248, one head over
 * the same pair).  The reference computes the weights and drops them (:191; attention_layer.py returns `attn`); the figure of its
 * paper that shows them (paper/attn_heatmap.py) is typed in by hand.  qs_enc_forward computes the same softmaxes inside its kernels
 * and keeps them in registers.  qs_attn_weights is a launch of its own that stops at the softmax and stores it.
 *
 * Row layouts, fp32, rows dense (weights[B, row_elems]):
 *   QS_ENC_NBR_ATTENTION   [K]          the softmax of :95-100 over the agent's K = num_nbr neighbour slots, in the slot order of the
 *                                       observation row
 *   QS_ENC_MODEL_MHA       [4][2][2]    head, query token, key token; token 0 = neighbour embedding, token 1 = obstacle embedding
 *                                       (attention_layer.py:103-108)
 *   QS_ENC_MODEL_S2R       [2][2]       query token, key token (attention_layer.py:82-84); width 256 and the narrow widths 16 / 32 / 64
 * Every row of a softmax sums to 1.
 *
 * Batch coupling.  QuadNeighborhoodEncoderAttention tiles the WHOLE batch (`self_obs.repeat(K, 1)` :84, `mean.repeat(K, 1)` :92): row
 * (agent a, slot k) is paired with the self observation and the mean embedding of agent (a*K + k) mod B.  That pairing is part of the
 * function here exactly as it is in qs_enc_forward: the weights of an agent depend on the batch it is evaluated in.  The two
 * multi-head classes treat every row on its own.
 *
 * Precision.  Reference precision only: params->precision must be 1 and every layer arrives in the split fp16-pair packing of
 * quadswarm_encoder.h, whatever precision the sampler itself runs in; scores and softmax are fp32.  Weights within 1e-5 of the fp32
 * module (tests/test_attention_weights_gpu.py).
 *
 * Fields read - everything else in qs_enc_params is ignored and may be zero (self encoder, value MLP, mv, mfc, LayerNorm, f, head,
 * sampling, trajectory copy):
 *   attention   self_dim nbr_dim num_nbr obs_dim precision, n1 n2 a1e a1m a2 a3w a3b, ebuf gbuf (the scratch of qs_enc_forward, same
 *               sizes: it is overwritten)
 *   MHA         self_dim nbr_dim num_nbr obst_dim obs_dim precision, n1 n2 o1 o2 mq mk
 *   S2R         self_dim nbr_dim num_nbr obst_dim obs_dim precision, n1 o1 mq mk; the width is n1.M (256, or 16 / 32 / 64)
 *
 * Launch rules.  Stream-ordered, allocation-free, no synchronisation: a call records into a HIP graph.  Deterministic: one thread owns
 * each output element, no atomics.  Rows >= B of `weights` are never written.  attention: two launches (the embedding launch of
 * qs_enc_forward, unchanged, then the scores); MHA / S2R: one.
 *
 * Both functions validate BEFORE anything is launched and leave a qs_enc_last_error() message:
 *   -1  a NULL required pointer (obs, params, weights, a weight / bias / scratch pointer of a field read), B < 1
 *   -4  mean_embed / mlp / no_encoder (no attention), attention with num_nbr == 0, precision != 1, and the layer / width combinations
 *       qs_enc_forward refuses (more than 8 neighbours, inputs wider than 32 - 64 for the multi-head classes' neighbour columns -,
 *       MHA / S2R without neighbours or obstacle columns, a Sim2Real width other than 16 / 32 / 64 / 256, layers that disagree on it)
 *   -2  a failed launch
 */
#ifndef QUADSWARM_ATTENTION_H
#define QUADSWARM_ATTENTION_H

#include <stddef.h>
#include <stdint.h>

#include "quadswarm_encoder.h"

#ifdef __cplusplus
extern "C" {
#endif

/* elements of one agent's row of weights for this model (K, 16 or 4), or < 0 (same codes as qs_attn_weights; no pointer of
 * `params` is looked at but `params` itself) */
int32_t qs_attn_row_elems(const qs_enc_params *params);

/* weights[B, row_elems] fp32 = the attention weights the encoder of `params` computes on obs[B, obs_dim], on `stream` */
int qs_attn_weights(const float *obs, int32_t B, const qs_enc_params *params, float *weights, void *stream);

#ifdef __cplusplus
}
#endif
#endif

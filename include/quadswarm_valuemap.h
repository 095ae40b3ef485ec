/*
 * quadswarm_valuemap.h - C ABI of the critic value map: what a critic answers for every agent if the agent stood somewhere else.
 * Exported by libquadswarm_encoder.so (it calls qs_enc_forward); qs_enc_params is that of quadswarm_encoder.h.
 *
 * Reference: swarm_rl/env_wrappers/v_value_map.py:39-67 (V_ValueMapWrapper.get_v_value_map_2d, behind --visualize_v_value,
 * quad_utils.py:96-108): one agent's observation row, columns 0 and 1 (x / y relative to the goal) overwritten with
 * init + i * 0.2 and init + j * 0.2 for i, j in -10..10, the critic called once per cell - 441 forward passes of batch one.
 *
 * Semantics.  For agent a, grid cell (i, j) with 0 <= i < nx, 0 <= j < ny, and row r = a * nx * ny + i * ny + j:
 *     rows[r, c] = obs[a, c]                                        for every column c that no shift entry names,
 *     rows[r, col] = obs[a, col] + sign * off_axis[index]           for a shift entry {col, axis, sign}: index = i and off = off_x
 *                                                                   for axis 0, index = j and off = off_y for axis 1; sign is +1 or -1.
 * That is ONE float32 add per shifted element (sign * off is exact) and a bit copy of every other one.  A column is named at most once.
 *     values[a, i, j] = critic_head(encoder(rows[r]))               the reference's tmp_score[i][j]: i moves x
 *     vmax[a], vmin[a] = the largest / smallest of the agent's nx * ny values, argmax[a] = the flat index i * ny + j of the largest.
 * The first index wins on ties (-0.0 and +0.0 tie), and vmax / vmin carry the bits of the element that won.  With a NaN among the
 * values vmax and vmin are NaN and argmax is the first NaN's index - what numpy's max / min / argmax answer.
 *
 * The offset tables are float32 and come from the caller; the reference's `float32 tensor + python float` is
 * obs + (float)(k * 0.2) with k * 0.2 evaluated in double, so tables filled that way give the reference's rows bit for bit.
 * Only columns of the observation can be shifted: the obstacle SDF columns of a row are a function of the map, not of an offset,
 * and stay what they were.
 *
 * The encoder sees the rows in batches of at most cap_rows.  Every encoder but `attention` treats a row on its own; the
 * `attention` neighbour encoder pairs rows ACROSS a batch (quad_multi_model.py:84,92 tile the whole batch), so for it the batching
 * is part of the function, and only cap_rows = 1 is the reference's batch of one per cell.
 *
 * Everything is stream-ordered; nothing is allocated and nothing is synchronised: a call records into a HIP graph (tables and shift
 * list travel in launch arguments, a graph keeps the ones it was captured with).  Deterministic: no atomics, fixed combine order.
 */
#ifndef QUADSWARM_VALUEMAP_H
#define QUADSWARM_VALUEMAP_H

#include <stddef.h>
#include <stdint.h>

#include "quadswarm_encoder.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QS_VMAP_MAX_GRID 64        /* 1 <= nx, ny <= 64 */
#define QS_VMAP_MAX_SHIFTS 64      /* entries of the shift list */
#define QS_VMAP_MAX_OBS_DIM 4096   /* columns of a row (the per-column shift codes of a workgroup live in LDS) */

typedef struct qs_value_map_params {
    int32_t A, obs_dim;                        /* agents (>= 1), columns of a row */
    int32_t nx, ny;
    const float *obs;                          /* [A, obs_dim], device */
    float off_x[QS_VMAP_MAX_GRID];             /* [nx] used */
    float off_y[QS_VMAP_MAX_GRID];             /* [ny] used */
    int32_t n_shifts;                          /* 0 .. QS_VMAP_MAX_SHIFTS */
    int32_t shift_col[QS_VMAP_MAX_SHIFTS];     /* < obs_dim, each column at most once */
    int32_t shift_axis[QS_VMAP_MAX_SHIFTS];    /* 0: off_x[i], 1: off_y[j] */
    int32_t shift_sign[QS_VMAP_MAX_SHIFTS];    /* +1 or -1 */
    float *rows;                               /* scratch [cap_rows, obs_dim], device */
    int32_t cap_rows;                          /* >= 1 */
    float *values;                             /* [A, nx, ny], device */
    float *vmax, *vmin;                        /* [A] each, device; each may be NULL */
    int32_t *argmax;                           /* [A], device; may be NULL */
} qs_value_map_params;

size_t qs_value_map_sizeof_params(void);

/* Rows only: rows[0 .. n_rows) = the hypothetical rows row0 .. row0 + n_rows (global numbering above), 0 <= row0,
 * row0 + n_rows <= A * nx * ny, 1 <= n_rows <= cap_rows.  One launch.  obs_dim % 4 == 0 with 16-byte aligned obs and rows takes
 * one 16-byte load and store per thread; anything else the 4-byte path.  values / vmax / vmin / argmax are not looked at. */
int qs_value_map_expand(const qs_value_map_params *p, int64_t row0, int32_t n_rows, void *stream);

/* vmax / vmin / argmax of the values buffer the caller supplies (p->values [A, nx * ny]); one wave per agent, one launch - none
 * when all three outputs are NULL.  obs, rows, the tables and the shift list are not looked at. */
int qs_value_map_reduce(const qs_value_map_params *p, void *stream);

/* The whole map: for every chunk of at most cap_rows rows, expand and then qs_enc_forward on a copy of `critic` with
 * head_out = values + row0 and no feature output; after the last chunk the reduction.  `critic` carries a head of ONE row
 * (head_dim == 1, head_w, head_b), obs_dim equal to p->obs_dim and - for the attention encoder - scratch for cap_rows rows; its
 * head_out and sampling / trajectory fields are ignored.
 *
 * All three functions validate BEFORE the first launch and return -1 with a qs_enc_last_error() message for: a NULL required
 * pointer, head_dim != 1, nx or ny outside 1..QS_VMAP_MAX_GRID, A < 1, obs_dim outside 1..QS_VMAP_MAX_OBS_DIM, more than
 * QS_VMAP_MAX_SHIFTS shifts, a shift column outside the row or named twice, an axis other than 0 / 1, a sign other than +1 / -1,
 * cap_rows < 1, a row range outside the map, critic->obs_dim != p->obs_dim; -2 for a failed launch; what qs_enc_forward returns
 * when it refuses the critic. */
int qs_value_map(const qs_value_map_params *p, const qs_enc_params *critic, void *stream);

#ifdef __cplusplus
}
#endif
#endif

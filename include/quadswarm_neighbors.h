/*
 * quadswarm_neighbors.h - C ABI of the neighbour identities: WHICH drone stands behind each of the K neighbour slots of an observation
 * row, and the scatter of per-slot values (attention weights) into drone-by-drone matrices.  Exported by libquadswarm_hip.so; the handle
 * is that of quadswarm.h.
 *
 * The environment fills slot s of drone i with clip(pos_j - pos_i, +-nbr_clip_pos), clip(vel_j - vel_i, +-nbr_clip_vel) of the s-th
 * nearest drone j (gym_art/quadrotor_multi/quadrotor_multi.py:233-274) and keeps j to itself.  That slot is ONE subtraction in the
 * handle's precision on the very positions the step kernel stores back to the state, so a launch of its own that redoes the subtraction
 * from the stored state gets the same bits and finds j by exact comparison.  The answer is defined by the row ("which drone is behind
 * this slot"), not by a second ranking - which matters at an episode's first observation, where the reference ranks with the previous
 * episode's velocities (the reset kernel reproduces that) and a fresh ranking would name other drones.
 *
 * Definition, for drone i of environment e and slot s = 0 .. K-1 in order (K = qs_config.num_neighbors):
 *   - a CANDIDATE is a drone j != i of the same environment that no earlier slot of this row was given, whose clipped position
 *     difference equals the row's three columns self_dim + 6 s .. + 2 by value (-0 == +0), in the handle's precision;
 *   - with more than one candidate, those whose clipped velocity difference equals columns self_dim + 6 s + 3 .. + 5 as well are
 *     preferred; among those - or among all candidates if none matches the velocity - the lowest index wins;
 *   - without a candidate the slot's id is -1: the row is not of the moment of the stored state (qs_set_state in between, an old copy
 *     of the rows passed as obs_dev).
 * Neither the velocity columns nor the neighbour metric is used for anything else.
 */
#ifndef QUADSWARM_NEIGHBORS_H
#define QUADSWARM_NEIGHBORS_H

#include <stdint.h>

#include "quadswarm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Neighbour identities of every observation row of the handle, as ONE launch on `stream` (stream-ordered, allocation-free, deterministic:
 * it can be captured into a HIP graph behind a step; one thread owns each output row, rows >= E*N are never written):
 *   obs_dev      real [E*N, obs_dim] row-major, device, of the handle's precision; NULL = qs_buffers.obs
 *   ids_out_dev  int32 [E*N, K], device
 * QS_ERR_INVALID for a NULL handle, a NULL output or a handle with num_neighbors == 0; QS_ERR_UNSUPPORTED while a gated launch of the
 * handle is resident (qs_step_gated: the state is not in device memory then; qs_sync ends that). */
int qs_neighbor_ids(qs_handle *h, const void *obs_dev, int32_t *ids_out_dev, void *stream);

/* out[e, i, j] = w[e*N + i, s] for the slot s with ids[e*N + i, s] == j, every other entry 0 (the diagonal included); slots whose id is
 * outside [0, N) - the -1 above - are dropped.  ids_dev int32 [E*N, K], w_dev float [E*N, K], out_dev float [E, N, N], all device; the
 * values are bit copies.  One launch on `stream`, one thread owns a row of the output: it zeroes the row, then fills it.  Needs no handle.
 * Returns -1 for a NULL pointer, N < 2, N > QS_MAX_AGENTS, K < 1, K > N - 1 or E < 1 (qs_last_error has the text), -2 for a HIP error. */
int qs_neighbor_scatter(const int32_t *ids_dev, const float *w_dev, int32_t E, int32_t N, int32_t K, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif

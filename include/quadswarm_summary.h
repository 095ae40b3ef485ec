/*
 * quadswarm_summary.h - C ABI of the episode summary: per-key sums and counts of the finished episodes of a handle, kept on the device.
 * Exported by libquadswarm_hip.so; the handle is that of quadswarm.h.
 *
 * What a training run plots - per-scenario success / deadlock / collision rates, distances to the goal, collision counters, reward-term
 * sums, true_reward, action moments - is the MEAN, key by key, of the per-agent dicts {"true_reward", **episode_extra_stats} that the
 * reference's wrapper stack attaches at an episode end (quadrotor_multi.py:626-718, reward_shaping.py:85-118).  Every input of those
 * dicts is in device memory behind the step kernel: ep_sums, ep_stats, ep_counters, ep_scenario, scenario_id and the replay wrapper's
 * per-environment flags.  The summary adds them up there: two launches behind a step, two small tables, no per-agent traffic to the host.
 *
 * A WINDOW is everything accumulated since the last clear.  Both tables have QS_SUMM_SCENARIOS rows, one per scenario id (the values of
 * qs_config.scenario; under `mix` the sub-scenario), and the column says WHICH scenario of the environment indexes the row:
 *
 *   sums   double [QS_SUMM_SCENARIOS][QS_SUMM_D_COUNT]
 *     row = ep_scenario (the scenario that ENDED), episodes that were NOT replayed only:
 *       QS_SUMM_D_DIST_1S .. _5S       sum over the agents of ep_stats rows QS_EPS_DIST_1S .. _5S
 *       QS_SUMM_D_SUCCESS .. _OBST_COL sum over the environments of the per-episode rates (success, deadlock, collision, neighbour
 *                                      collision, obstacle collision): counts of the agents' flags divided by N, as quadrotor_multi.py:690-705
 *     row = ep_scenario, every finished episode:
 *       QS_SUMM_D_REW + r              sum over the agents of ep_sums row r (r < QS_RI_COUNT)
 *       QS_SUMM_D_TRUE_REWARD          sum over the agents of  ep_sums[QS_RI_RAW_MAIN] + 1000 * ep_sums[QS_RI_RAW_QUADCOL]  (formed per agent)
 *       QS_SUMM_D_ACT_MEAN + q         sum over the environments of the episode's mean of raw action q over agents x steps
 *       QS_SUMM_D_ACT_STD + q          ... of the episode's standard deviation sqrt(max(E[a^2] - E[a]^2, 0))   (formed per episode)
 *     row = scenario_id (the scenario that STARTS behind the end - reward_shaping.py:95-98 names its two keys after the auto-reset):
 *       QS_SUMM_D_START_REW_POS, QS_SUMM_D_START_REW_CRASH   sum over the agents of ep_sums rows QS_RI_REW_POS / QS_RI_REW_CRASH
 *
 *   counts int64 [QS_SUMM_SCENARIOS][QS_SUMM_I_COUNT]
 *     row = ep_scenario:
 *       QS_SUMM_I_EPISODES             finished episodes (environments, not agents)
 *       QS_SUMM_I_REPLAYED             ... of them replayed ones (qs_replay_enable: the episode started from a checkpoint)
 *       QS_SUMM_I_CNT + c              sum of ep_counters row c (c < QS_CNT_COUNT) over the episodes that were not replayed
 *       QS_SUMM_I_COL_REPLAY, _OBST_REPLAY   sum of ep_counters rows QS_CNT_COLLISIONS / QS_CNT_OBST over the replayed ones (:629-633)
 *       QS_SUMM_I_OVERRUN              environments that ended more than once inside one accumulate call (below)
 *     row = scenario_id:
 *       QS_SUMM_I_START_EPISODES       finished episodes
 *
 * The action moments divide by N * steps of the episode: the replay wrapper's step count of the episode where replay is on (a replayed
 * episode starts at its checkpoint's tick), ep_len + 1 otherwise.  On a handle without episode_sums the QS_SUMM_D_REW .. _START_REW_CRASH
 * columns stay 0.
 *
 * Arithmetic: every floating-point sum is a double, integers are summed as integers, and there are no floating-point atomics: each
 * element of a table is owned by one thread and receives its terms in an order fixed by (E, N) - agents in index order inside a tile of
 * environments, tiles in order inside a workgroup, workgroups in order in the second launch.  Two handles of the same shape that saw the
 * same episodes hold bitwise equal tables.
 */
#ifndef QUADSWARM_SUMMARY_H
#define QUADSWARM_SUMMARY_H

#include <stdint.h>

#include "quadswarm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QS_SUMM_SCENARIOS 16
enum { QS_SUMM_D_DIST_1S = 0, QS_SUMM_D_DIST_3S, QS_SUMM_D_DIST_5S,
       QS_SUMM_D_SUCCESS, QS_SUMM_D_DEADLOCK, QS_SUMM_D_COL, QS_SUMM_D_NBR_COL, QS_SUMM_D_OBST_COL,
       QS_SUMM_D_REW,                                          /* QS_RI_COUNT columns */
       QS_SUMM_D_TRUE_REWARD = QS_SUMM_D_REW + QS_RI_COUNT,
       QS_SUMM_D_ACT_MEAN,                                     /* 4 columns */
       QS_SUMM_D_ACT_STD = QS_SUMM_D_ACT_MEAN + 4,             /* 4 columns */
       QS_SUMM_D_START_REW_POS = QS_SUMM_D_ACT_STD + 4, QS_SUMM_D_START_REW_CRASH,
       QS_SUMM_D_COUNT };
enum { QS_SUMM_I_EPISODES = 0, QS_SUMM_I_REPLAYED,
       QS_SUMM_I_CNT,                                          /* QS_CNT_COUNT columns */
       QS_SUMM_I_COL_REPLAY = QS_SUMM_I_CNT + QS_CNT_COUNT, QS_SUMM_I_OBST_REPLAY,
       QS_SUMM_I_OVERRUN, QS_SUMM_I_START_EPISODES,
       QS_SUMM_I_COUNT };

/* Allocates the two tables (zeroed) and the per-workgroup partial tables of the handle, once; further calls do nothing.  qs_destroy
 * frees them. */
int qs_episode_summary_enable(qs_handle *h);

/* Adds the episodes that ended to the tables, as two launches on `stream` (stream-ordered, allocation-free: it can be captured into a
 * HIP graph behind a step):
 *   done_dev   uint8 [steps][E*N], device: the done flags of `steps` consecutive control steps; NULL = qs_buffers.done with steps = 1.
 * Environment e is counted ONCE if any of the rows has done[t][e*N] set, with what the ep_* buffers hold now - so the call is valid any
 * time before the environment's NEXT episode end.  An environment with two or more ends in the rows adds 1 to QS_SUMM_I_OVERRUN: its
 * earlier episode is gone from the ep_* buffers and is not in the tables (segments are meant to be shorter than episodes).  A call
 * whose rows hold no end leaves both tables bitwise as they were.
 * QS_ERR_INVALID before qs_episode_summary_enable or for steps < 1; QS_ERR_UNSUPPORTED while a gated launch of the handle is resident
 * (qs_step_gated; qs_sync ends that). */
int qs_episode_summary_accumulate(qs_handle *h, const uint8_t *done_dev, int32_t steps, void *stream);

/* Copies the tables to the host - sums_host double [QS_SUMM_SCENARIOS * QS_SUMM_D_COUNT], counts_host int64 [QS_SUMM_SCENARIOS *
 * QS_SUMM_I_COUNT], either may be NULL - then, with clear != 0, zeroes both (a new window).  Ordered on `stream`; returns after the
 * copies have landed. */
int qs_episode_summary_read(qs_handle *h, double *sums_host, int64_t *counts_host, int32_t clear, void *stream);

#ifdef __cplusplus
}
#endif
#endif

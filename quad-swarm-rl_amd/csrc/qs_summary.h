// qs_summary.h - what qs_episode_summary.hip (include/quadswarm_summary.h) sees of a handle.  `struct qs_handle` and the text behind
// qs_last_error are private to quadswarm_hip.hip, which implements the two functions below.
#pragma once
#include "../../include/quadswarm_summary.h"

struct QsSummaryView {
    int E, N, device, real_size, ep_len, episode_sums;
    int gate_resident;           // a qs_step_gated launch has not been joined on the host
    const uint8_t *done;         // qs_buffers.done
    const void *ep_sums, *ep_stats;                               // real [QS_SUM_COUNT, E*N], [QS_EPS_COUNT, E*N]
    const int32_t *ep_counters, *ep_scenario, *scenario_id;       // [QS_CNT_COUNT, E], [E], [E]
    const uint8_t *ep_was_replay;                                 // [E], nullptr without qs_replay_enable
    const int32_t *ep_steps;                                      // [E] control steps of the last finished episode, nullptr likewise
    void **store;                // the handle's slot for the summary's one device allocation (hipMalloc'd here, hipFree'd by qs_destroy)
};
extern "C" int qs_summary_view(struct qs_handle *h, QsSummaryView *out);
extern "C" int qs_summary_fail(int code, const char *msg);   // sets qs_last_error's text, returns `code`

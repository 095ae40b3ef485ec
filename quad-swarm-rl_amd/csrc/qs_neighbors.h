// qs_neighbors.h - what qs_neighbor_ids.hip (include/quadswarm_neighbors.h) sees of a handle.  `struct qs_handle` and the text behind
// qs_last_error are private to quadswarm_hip.hip, which implements the two functions below.
#pragma once
#include "../../include/quadswarm_neighbors.h"
#include "qs_state_blk.h"

struct QsNeighborsView {
    const qs_config *cfg;
    StateBlk blk;                // the wave-blocked state allocation (qs_state_blk.h)
    int device, real_size, cus;
    int gate_resident;           // a qs_step_gated launch has not been joined on the host: the state lives in its registers / LDS
    const void *obs;             // qs_buffers.obs
    int obs_dim, self_dim;       // columns of a row, and of its self block in front of the neighbour slots
};
extern "C" int qs_neighbors_view(struct qs_handle *h, QsNeighborsView *out);
extern "C" int qs_neighbors_fail(int code, const char *msg);   // sets qs_last_error's text, returns `code`

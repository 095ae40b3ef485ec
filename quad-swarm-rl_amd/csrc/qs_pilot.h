// qs_pilot.h - what qs_pilot.hip (include/quadswarm_control.h) sees of a handle.  `struct qs_handle` and the text behind qs_last_error are
// private to quadswarm_hip.hip, which implements the two functions below.
#pragma once
#include "../../include/quadswarm_control.h"
#include "qs_state_blk.h"

struct QsPilotView {
    const qs_config *cfg;
    StateBlk blk;                // the wave-blocked state allocation (qs_state_blk.h)
    int device, real_size, cus;
    int gate_resident;           // a qs_step_gated launch has not been joined on the host: the state lives in its registers / LDS
    void *actions;               // qs_buffers.actions
    qs_pilot_params **params;    // the handle's slot for its controller parameters (malloc'd by qs_pilot.hip, freed by qs_destroy)
};
extern "C" int qs_pilot_view(struct qs_handle *h, QsPilotView *out);
extern "C" int qs_pilot_fail(int code, const char *msg);   // sets qs_last_error's text, returns `code`

// qs_step_kernel_modes.inc - the single-wave step body in its two launch modes, for the arguments and QS_SCEN_FULL that
// qs_step_flavours.inc has set: one control step per launch, then the open-loop rollout.
#define QS_MULTI 0
#include "qs_step_kernel.inc"
#undef QS_MULTI
#define QS_MULTI 1
#include "qs_step_kernel.inc"
#undef QS_MULTI

// qs_step_team_modes.inc - the team step body in its three launch modes, for the arguments, QS_TW and QS_SCEN_FULL that
// qs_step_flavours.inc has set: one control step per launch, the open-loop rollout, then the resident-state kernel of qs_step_gated.
#define QS_MULTI 0
#include "qs_step_team.inc"
#undef QS_MULTI
#define QS_MULTI 1
#include "qs_step_team.inc"
#undef QS_GATED
#define QS_GATED 1
#include "qs_step_team.inc"
#undef QS_GATED
#undef QS_MULTI

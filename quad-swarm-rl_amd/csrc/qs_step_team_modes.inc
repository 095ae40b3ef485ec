// qs_step_team_modes.inc - the team step body in its three launch modes, for the arguments, QS_TW and QS_SCEN_FULL that
// qs_step_flavours.inc has set: one control step per launch, the open-loop rollout, then the resident-state kernel of qs_step_gated.
// The one-step body comes twice: without the fused observation exchange (QS_XCHG 0: qs_spec_step / qs_step_team[_full], what a handle
// launches while no exchange is attached) and with it (QS_XCHG 1: the same names + `_x`, launched while qs_set_obs_exchange is in effect).
// What the ISA shows: with the epilogue inlined behind a run-time test the C2 object has an `s_waitcnt vmcnt(0)` between wave 0's output
// stores and its state stores on the path that exchanges nothing (the waitcnt pass merges the exchange branch's pending memory operations
// into the join), 9 barriers and ~1050 more instructions; the split body has none of it (tests/test_step_tail_asm.py).  What that is worth
// on the clock was measured by same-box A/B: DESIGN 5.1 (C3 and the C4 shard gain, C2 within the noise).  -DQS_XCHG_INLINE=1: the single
// body again (A/B and identity switch; such an object has no `_x` entry point, so qs_set_obs_exchange refuses it).
#ifndef QS_XCHG_INLINE
#define QS_XCHG_INLINE 0
#endif
// (the body's second inclusion below goes through this macro: tests/test_kernel_table.py pins the list of quoted includes of this file -
// one per launch mode - and the `_x` instantiation is a fourth inclusion, not a fourth mode)
#define QS_TEAM_BODY "qs_step_team.inc"
#define QS_MULTI 0
#define QS_XCHG QS_XCHG_INLINE
#include "qs_step_team.inc"
#undef QS_XCHG
#if !QS_XCHG_INLINE && !(defined(QS_SPEC) && QS_SPEC_PRECISION == 8)   // (the exchange lives in the float32 kernels)
#define QS_XCHG 1
#define qs_spec_step qs_spec_step_x
#define qs_step_team qs_step_team_x
#define qs_step_team_full qs_step_team_full_x
#include QS_TEAM_BODY
#undef qs_spec_step
#undef qs_step_team
#undef qs_step_team_full
#undef QS_XCHG
#endif
#define QS_XCHG 0
#undef QS_MULTI
#define QS_MULTI 1
#include "qs_step_team.inc"
#undef QS_GATED
#define QS_GATED 1
#include "qs_step_team.inc"
#undef QS_GATED
#undef QS_MULTI
#undef QS_XCHG
#undef QS_TEAM_BODY

// qs_kernels.h - device side of the MI355X (gfx950) QuadSwarm stepper, in its parts: buffers, LDS layout, observation rows, responses,
// reset, the step semantics and the step kernels of one flavour.  Included by quadswarm_hip.hip (generic library; it adds
// qs_replay_kernels.h), by qs_tape_kernels.hip (QS_TAPE) and by qs_spec_kernels.hip (QS_SPEC: config-specialised code objects).
#pragma once
// "team" kernels (qs_step_team.inc): 4 waves per workgroup.  Their exchanges go through LDS only, so the workgroup
// barrier waits for LDS traffic but leaves global loads / stores in flight; inside one wave LDS operations are
// processed in issue order, so a wave-local hand-over needs a compiler barrier only.
#define QS_TEAM_WAVES 4
#define QS_TEAM_THREADS (QS_WAVE * QS_TEAM_WAVES)
#define QS_TEAM_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define QS_WAVE_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#include "qs_state_blk.h"        // QS_WAVE, StateBlk, BlkOff, blk_at: the state allocation
#include "qs_state_rows.h"       // Ptrs, BufRow, QS_ROW: the kernels' views of it
#include "qs_step_debug.h"       // QS_STAMP*, QS_POISON_*
#include "qs_lds_layout.h"       // LdsLayout, lds_layout() (host)
#include "qs_nbr_obs.h"          // neighbour keys / metrics / selection / emission, team_rank_local
#include "qs_obs_rows.h"         // obs_st*, obs_copy_rows, sdf_obs, stream_rows
#include "qs_xchg_fused.h"       // fused_prefetch, fused_push: the one-step team kernels' observation exchange
#include "qs_pair_responses.h"   // collide_drones_*, room_obst_responses
#include "qs_reset.h"            // scen_lds_*, ScenRegs, reset_body, qs_reset_impl
#include "qs_step_sem.h"         // the step semantics shared by the two step bodies
#include "qs_step_flavours.inc"  // the step / rollout / gated / reset kernels of this unit's flavour (spec / tape / generic)

// qs_env_plan.h - small rules that the HOST side of the environment stepper (quadswarm_hip.hip) decides by, in plain C++17 without HIP:
// scenario set, team width and observation width, each stated once.  tests/test_env_plan.py compiles this header alone with the host
// compiler.  The LDS layout has a header of its own in the same style, qs_lds_layout.h (tests/test_lds_layout.py).
#ifndef QS_ENV_PLAN_H
#define QS_ENV_PLAN_H
#include "../../include/quadswarm.h"

// scenario outside the fast set => the kernels compiled with QS_SCEN_FULL (per-env scenario state in LDS)
inline bool scenario_is_full(int scenario) {
    return !(scenario == QS_SCENARIO_STATIC_SAME_GOAL || scenario == QS_SCENARIO_O_STATIC_SAME_GOAL
        || scenario == QS_SCENARIO_SWARM_VS_SWARM);
}
// Specialised team kernels: 8 waves (2 per SIMD) halve the striped phases once more for N <= 8 (C2 8.65 -> 8.15 us); with
// N > 8 the merge of 8 sorted lists outweighs that (C4 24.6 -> 28.3 us), so those keep 4 waves.
inline int spec_team_waves(int num_agents) { return num_agents <= 8 ? 8 : 4; }
// Team kernels pay off while the whole batch still fits at <= 8 waves per CU (measured on MI355X, specialised fp32 kernels, us per
// step team / single-wave: C2 shape 1024 envs 8.3 / 9.1, 2048 envs 9.1 / 9.8, 3072 envs 13.8 / 10.8; C4 shape 1024 envs 23.1 / 26.4)
inline bool team_default(int blocks, int cus, int num_agents) { return (long)blocks * spec_team_waves(num_agents) <= 8L * cus; }
// columns of a drone's own observation (QS_OBS_*: xyz_vxyz_R_omega, _floor, _wall)
inline int qs_self_dim(int obs_repr) { return obs_repr == 0 ? 18 : (obs_repr == 1 ? 19 : 24); }

#endif

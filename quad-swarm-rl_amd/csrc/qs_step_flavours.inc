// qs_step_flavours.inc - the kernels of one translation unit: which step bodies (qs_step_kernel_modes.inc: single-wave step + rollout;
// qs_step_team_modes.inc: team step + rollout + gated) get which kernel arguments for which scenario sets, and the unit's reset
// kernel.  Included once, by qs_kernels.h; the flavour is the includer's QS_SPEC / QS_TAPE / neither.
// Generic library: template kernels (single-wave / team) x (fast / full scenario set) x (step / rollout; team: + gated) x
// (float / double), every configuration value a run-time kernel argument.
// Config-specialised code object (qs_spec_kernels.hip, -DQS_SPEC_FILE="<header from qs_spec_header()>"): the three kernels
// one configuration needs, with every constant of the configuration, the LDS layout and the envs-per-workgroup count as
// literals - loops over drones / neighbours / obstacles unroll, LDS addresses fold into instruction offsets and the
// scalar bookkeeping of the generic kernels disappears (a lone wave per SIMD issues one instruction every ~4.5 cycles
// whatever its type, so instruction count is what the per-step latency is made of).  What stays a run-time argument:
// seed, env_id_offset, num_envs; the reward coefficients (annealed by the reward-shaping wrapper) are read from device memory.
#ifdef QS_SPEC   // ---- one configuration: constants, layout and envs per workgroup from the generated header; the header's scenario set ----
#if QS_SPEC_PRECISION == 8
typedef double real;
#else
typedef float real;
#endif
__device__ __forceinline__ Consts<real> qs_spec_consts(const Consts<real> &rt) {
    Consts<real> c = __builtin_bit_cast(Consts<real>, qs_spec_cw);
    c.seed_lo = rt.seed_lo; c.seed_hi = rt.seed_hi; c.env_id_offset = rt.env_id_offset; c.num_envs = rt.num_envs;
    return c;
}
#define QS_KARGS const Consts<real> c_rt, Ptrs<real> p, const real *__restrict__ actions, LdsLayout L_rt
#define QS_EPB_ARG epb_rt
#define QS_SPEC_PROLOGUE const Consts<real> c = qs_spec_consts(c_rt); const LdsLayout L = __builtin_bit_cast(LdsLayout, qs_spec_lw); const int epb = QS_SPEC_EPB; (void)L_rt; (void)epb_rt;
#define QS_SCEN_FULL QS_SPEC_FULL
#if QS_SPEC_TEAM
#define QS_TW QS_SPEC_TEAM
#include "qs_step_team_modes.inc"
#else
#include "qs_step_kernel_modes.inc"
#endif
extern "C" __global__ void __launch_bounds__(QS_WAVE) qs_spec_reset(const Consts<real> c_rt, Ptrs<real> p, LdsLayout L_rt, int epb_rt) {
    QS_SPEC_PROLOGUE
    qs_reset_impl<real, (QS_SPEC_FULL != 0)>(c, p, L, epb);
}
#undef QS_SCEN_FULL

#elif defined(QS_TAPE)   // ---- noise-tape flavour (qs_tape_kernels.hip): single-wave single-step kernels + reset, own names ----
#define QS_KARGS const Consts<real> c, Ptrs<real> p, const real *__restrict__ actions, LdsLayout L
#define QS_EPB_ARG epb
#define QS_SPEC_PROLOGUE
#define qs_step_kernel qs_tape_step_kernel
#define qs_step_kernel_full qs_tape_step_kernel_full
#define QS_MULTI 0
#define QS_SCEN_FULL 0
#include "qs_step_kernel.inc"
#undef QS_SCEN_FULL
#define QS_SCEN_FULL 1
#include "qs_step_kernel.inc"
#undef QS_SCEN_FULL
#undef QS_MULTI
#undef qs_step_kernel
#undef qs_step_kernel_full
template <typename real, bool FULL>
__global__ void __launch_bounds__(QS_WAVE) qs_tape_reset_kernel(const Consts<real> c, Ptrs<real> p, LdsLayout L, int epb) {
    qs_reset_impl<real, FULL>(c, p, L, epb);
}

#else   // ---- generic kernels: both bodies, both scenario sets, every value a run-time argument ----
#define QS_KARGS const Consts<real> c, Ptrs<real> p, const real *__restrict__ actions, LdsLayout L
#define QS_EPB_ARG epb
#define QS_SPEC_PROLOGUE
#define QS_SCEN_FULL 0
#include "qs_step_kernel_modes.inc"
#undef QS_SCEN_FULL
#define QS_SCEN_FULL 1      // all scenarios incl. `mix` (qs_scenarios.h); scenario state in LDS
#include "qs_step_kernel_modes.inc"
#undef QS_SCEN_FULL
// the same four kernels as a team of 4 waves per workgroup (latency variant for small batches)
#define QS_TW QS_TEAM_WAVES
#define QS_SCEN_FULL 0
#include "qs_step_team_modes.inc"
#undef QS_SCEN_FULL
#define QS_SCEN_FULL 1
#include "qs_step_team_modes.inc"
#undef QS_SCEN_FULL

// reset kernel (qs_reset): resets the envs flagged in reset_mask
template <typename real, bool FULL>
__global__ void __launch_bounds__(QS_WAVE) qs_reset_kernel(const Consts<real> c, Ptrs<real> p, LdsLayout L, int epb) {
    qs_reset_impl<real, FULL>(c, p, L, epb);
}
#endif

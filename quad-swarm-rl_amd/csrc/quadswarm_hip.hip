// quadswarm_hip.hip - MI355X (gfx950) QuadSwarm environment stepper: kernels + C ABI (include/quadswarm.h).
//
// One translation unit.  This file: the handle, the constants fill, validation, allocation, create / destroy, the launch path of reset /
// step and the small setters / getters.  Included below, each where the old single file defined it:
// qs_spec_cache.inc (config-specialised code objects), qs_gate.inc (resident-state stepping), qs_snapshot_replay.inc (snapshots, the
// replay wrapper's setup), qs_env_debug.inc (state I/O, noise tape, debug and profiling calls); the generic kernels: kStepKernels.
//
// Mapping (wave64): one lane = one drone, one workgroup = one wavefront = floor(64/N) whole environments,
// so every cross-drone exchange of an environment (pair scan, neighbour selection, downwash, collision
// responses) goes through LDS inside one wave and needs no inter-workgroup traffic.  State is
// struct-of-arrays in HBM (component-major), so lane l of a wave reads word l of each component row:
// fully coalesced.  Observations are staged in LDS and copied out as one contiguous block per workgroup.
//
// Reference path (gym_art/quadrotor_multi/): quadrotor_multi.py:413-724 (step), :339-411 (reset); the
// per-piece citations are in qs_device.h and next to each phase below.  SURVEY.md Appendix A gives the
// order of operations that the step kernel follows.
#include <hip/hip_runtime.h>

#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "qs_codeobj_check.h"
#include "qs_kernels.h"
#include "qs_replay_kernels.h"
#include "qs_env_plan.h"
#include "qs_pilot.h"
#include "qs_summary.h"
#include "qs_neighbors.h"

using namespace qs_check;   // read_file, file_exists, run_program and the checker itself

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// noise-tape flavour of the kernels (qs_tape_kernels.hip, compiled with QS_TAPE)
extern "C" int qs_tape_lds_bytes(const qs_config *cfg, int obs_dim, int full, int real_size);
extern "C" int qs_tape_launch(int which, const qs_config *cfg, int obs_dim, int full, int real_size, const void *consts,
    const void *ptrs, const void *actions, void *stream);
static thread_local std::string g_last_error;
static int fail(int code, const std::string &msg) { g_last_error = msg; return code; }
#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(QS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)

struct qs_handle {
    qs_config cfg;
    int device = 0;
    int real_size = 4;
    int obs_dim = 0, epb = 1, blocks = 0;
    LdsLayout lds;
    bool full = false;     // scenario outside the fast set => kernels compiled with QS_SCEN_FULL
    int cus = 256;
    // waves per workgroup of the team kernels (qs_step_team.inc): 4 generic, 8 (or 4) specialised; 0 = single-wave kernels
    int team = 0;
    // environment snapshots (qs_snapshot_*): `snap_slots` packed copies of one environment's complete state
    // strides / counts in elements; kind: 1 = obs, 2 = episode sums; group > 0: wave-blocked (envs per block, bytes between blocks)
    struct SnapArray { char *base; size_t elem, comps, comp_stride, per_env; int kind; size_t group, group_stride; };
    std::vector<SnapArray> snap_arrays;
    size_t snap_bytes = 0;
    char *snap_pool = nullptr;
    int32_t snap_slots = 0;
    // config-specialised code object (qs_spec_kernels.hip), when one is cached / could be built
    hipModule_t spec_mod = nullptr;
    // (spec_gated: team objects only; spec_step_x: float32 team objects - the one-step kernel with the fused exchange epilogue)
    hipFunction_t spec_step = nullptr, spec_rollout = nullptr, spec_reset = nullptr, spec_gated = nullptr, spec_step_x = nullptr;
    std::string spec_note;   // why the handle runs the generic kernels (empty when it runs a config-specialised code object)
    Consts<float> kf;    // kernel constants, passed by value in the kernarg segment
    Consts<double> kd;
    Ptrs<float> pf;     // same field layout for float/double: only the pointee type differs
    std::vector<void *> allocs;
    qs_buffers bufs;
    void *d_actions = nullptr;
    void *obs_target = nullptr;   // qs_set_obs_target: where the next launches write their observation rows (nullptr = bufs.obs)
    double *d_state_buf = nullptr;
    int32_t *d_tick_io = nullptr;
    // cached hipGraph of a K-step rollout (qs_step_many): K identical step-kernel nodes
    hipStream_t cap_stream = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    const void *graph_actions = nullptr;
    int32_t graph_k = 0;
    uint8_t *h_mask = nullptr;   // pinned staging for qs_reset masks
    // batched experience replay (qs_replay_enable)
    bool replay_on = false;
    // a step was taken since qs_replay_enable: an explicit reset from now on is recorded by the wrapper state
    bool replay_stepped = false;
    ReplayParams rp;
    // noise tape (qs_set_noise_tape): device copy [E][tape_len] + per-env cursor; while set, reset / step run the tape kernels
    double *d_tape = nullptr;
    int32_t *d_tape_pos = nullptr;
    int64_t tape_len = 0;
    // resident-state stepping (qs_gate_create / qs_step_gated): device descriptor + action ring + sequence flags, one allocation
    qsx::Gate *d_gate = nullptr;
    qsx::Gate gate_host = {};
    // control steps launched so far by qs_step_gated / fed so far by qs_gate_produce
    unsigned long long gate_step_seq = 0, gate_prod_seq = 0;
    // The gated launch must be RESIDENT while its producer runs: two streams of one process may share a hardware queue (the runtime maps
    // streams onto a few HSA queues per priority level), and a queue runs its kernels one after the other - the producer behind a stepper
    // that waits for it would be a bounded deadlock (seen: 500 ms per launch in one of two otherwise identical bench runs).  The gated
    // kernel therefore runs on a stream of the library's own with the HIGHEST priority - a different queue pool than the caller's normal-
    // priority streams - stream-ordered with the caller's stream through two events.
    bool gate_pending = false;   // a gated launch was issued and has not been joined on the host since
    hipStream_t gate_stream = nullptr;
    hipEvent_t gate_ev_in = nullptr, gate_ev_out = nullptr;
    // profiling of the step kernel
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t events_used = 0;
    // controller parameters of qs_pilot_actions (qs_pilot.hip allocates them on first use; include/quadswarm_control.h)
    qs_pilot_params *pilot = nullptr;
    // tables and per-workgroup partials of the episode summary (qs_episode_summary.hip allocates them; include/quadswarm_summary.h)
    void *summary = nullptr;
};

template <typename real> static void fill_consts(const qs_config &c, Consts<real> &k) {
    memset(&k, 0, sizeof k);
    for (int q = 0; q < 3; ++q) { k.inertia[q] = (real)c.inertia[q]; k.inv_inertia[q] = (real)(1.0 / c.inertia[q]);
                                  k.room_lo[q] = (real)c.room_lo[q]; k.room_hi[q] = (real)c.room_hi[q];
                                  k.nbr_clip_pos[q] = (real)c.nbr_clip_pos[q]; k.nbr_clip_vel[q] = (real)c.nbr_clip_vel[q]; }
    k.arm = (real)c.arm; k.mass = (real)c.mass; k.inv_mass = (real)(1.0 / c.mass);
    for (int m = 0; m < 4; ++m) { for (int q = 0; q < 3; ++q) k.prop_cross[m][q] = (real)c.prop_cross[m][q];
                                  k.prop_ccw[m] = (real)c.prop_ccw[m]; k.thrust_max[m] = (real)c.thrust_max[m];
                                  k.torque_max[m] = (real)c.torque_max[m]; }
    k.motor_tau_up = (real)c.motor_tau_up; k.motor_tau_down = (real)c.motor_tau_down; k.motor_linearity = (real)c.motor_linearity;
    k.vel_damp = (real)c.vel_damp; k.damp_omega_quadratic = (real)c.damp_omega_quadratic; k.omega_max = (real)c.omega_max;
    k.thrust_noise_sigma = (real)c.thrust_noise_sigma; k.ou_theta = (real)c.ou_theta;
    k.dt = (real)c.dt; k.control_dt = (real)(c.dt * c.sim_steps);
    k.floor_threshold = (real)(c.floor_mode == QS_FLOOR_NUMPY ? 0.05 : c.arm);   // quadrotor_dynamics.py:75 / :378
    k.pos_norm_std = (real)c.pos_norm_std; k.pos_unif_range = (real)c.pos_unif_range; k.vel_norm_std = (real)c.vel_norm_std;
    k.vel_unif_range = (real)c.vel_unif_range; k.quat_norm_std = (real)c.quat_norm_std; k.quat_unif_range = (real)c.quat_unif_range;
    k.gyro_noise_density = (real)c.gyro_noise_density;
    k.collision_threshold = (real)c.collision_threshold; k.collision_falloff_threshold = (real)c.collision_falloff_threshold;
    for (int q = 0; q < QS_REW_COUNT; ++q) k.rew_coeff[q] = (real)c.rew_coeff[q];
    k.spawn_box = (real)c.spawn_box; k.approach_goal_metric = (real)c.approach_goal_metric;
    k.obst_radius = (real)(c.obst_size / 2.0); k.obst_hit_threshold = (real)(c.arm + c.obst_size / 2.0); k.obst_size = (real)c.obst_size;
    k.room_mid_z = (real)((c.room_hi[2] - c.room_lo[2]) / 2.0);
    k.sim_steps = c.sim_steps; k.ep_len = c.ep_len; k.floor_mode = c.floor_mode; k.svd_period = c.svd_period; k.sense_noise = c.sense_noise;
    k.obs_repr = c.obs_repr; k.self_dim = qs_self_dim(c.obs_repr); k.obs_dim = qs_obs_dim(&c);
    k.num_neighbors = c.num_neighbors; k.use_downwash = c.use_downwash; k.use_obstacles = c.use_obstacles; k.scenario = c.scenario;
    k.num_obstacles = c.num_obstacles; k.obst_area[0] = c.obst_area[0]; k.obst_area[1] = c.obst_area[1];
    const double control_freq = 1.0 / (c.dt * c.sim_steps);
    k.control_freq = (int)(control_freq + 0.5);
    k.grace_steps = (int)std::ceil(1.5 * control_freq - 1e-9);    // tick >= 1.5*control_freq (quadrotor_multi.py:146,:451)
    k.final_steps = (int)std::floor(5.0 * control_freq + 1e-9);   // time_remain <= 5*control_freq (:150,:455)
    k.cube_fd_all = (int)pow((double)c.num_agents, 1.0 / 3);
    k.cube_fd[0] = (int)pow((double)(c.num_agents / 2), 1.0 / 3);
    k.cube_fd[1] = (int)pow((double)(c.num_agents - c.num_agents / 2), 1.0 / 3);
    k.seed_lo = (uint32_t)(c.seed & 0xffffffffu); k.seed_hi = (uint32_t)(c.seed >> 32);
    k.env_id_offset = c.env_id_offset; k.num_envs = c.num_envs; k.num_agents = c.num_agents;
    k.write_rew_info = c.write_rew_info;
    k.episode_sums = c.episode_sums;
    k.dr_num_density = c.use_obstacles ? c.dr_num_density : 0; k.dr_num_size = c.use_obstacles ? c.dr_num_size : 0;
    k.dr_on = (k.dr_num_density > 0 || k.dr_num_size > 0) ? 1 : 0;
    k.arm_r = (real)c.arm;
    k.inv_dt = (real)(1.0 / c.dt);
    k.prox_ratio = (real)(-c.rew_coeff[QS_REW_QUADCOL_SMOOTH_MAX] / c.collision_falloff_threshold);
    for (int w = 0; w < 3; ++w) {
        const int win = (w == 0 ? 1 : (w == 1 ? 3 : 5)) * k.control_freq, total = c.ep_len + 1;
        k.inv_win[w] = (real)(1.0 / (double)(total < win ? total : win));
    }
}

// Rows per pass of the observation output of a config-specialised single-wave kernel (qs_lds_layout.h, lds_layout): 16 rows keep a
// workgroup under 10 KB of LDS (16 workgroups per CU); the register-held row values need D - S <= QS_NV_MAX, i.e. K <= 8.
// QS_OBS_RP=16|32|64 overrides (64 = complete rows at once, the generic kernels' layout).
static int spec_rows_per_pass(const qs_config *cfg, int team) {
    if (team || qs_obs_dim(cfg) - qs_self_dim(cfg->obs_repr) > QS_NV_MAX) return QS_WAVE;
    int rp = 16;
    if (const char *ev = getenv("QS_OBS_RP")) { const int v = atoi(ev); if (v == 16 || v == 32 || v == 64) rp = v; }
    return rp;
}

// The LDS layout of a handle's kernels (qs_lds_layout.h): `team` waves per workgroup (0 = single-wave), the generic kernels' complete rows
// or the specialised ones' rows per pass.  One wave of floor(64 / N) whole environments per workgroup, always.
static LdsLayout handle_layout(const qs_config *cfg, int team, bool specialised) {
    return lds_layout(cfg->precision == QS_PRECISION_F64 ? 8 : 4, QS_WAVE, cfg->num_agents, QS_WAVE / cfg->num_agents, qs_obs_dim(cfg),
                      cfg->num_obstacles, cfg->num_neighbors, team, scenario_is_full(cfg->scenario), false, cfg->scenario,
                      specialised ? spec_rows_per_pass(cfg, team) : QS_WAVE);
}

static int validate(const qs_config *c) {
    if (c->num_envs < 1) return fail(QS_ERR_INVALID, "num_envs must be >= 1");
    if (c->num_agents < 1 || c->num_agents > QS_MAX_AGENTS) return fail(QS_ERR_INVALID, "num_agents must be in [1, 64]");
    if (c->num_neighbors < 0 || c->num_neighbors > c->num_agents - 1) return fail(QS_ERR_INVALID, "Incorrect number of neigbors");
    if (c->precision != QS_PRECISION_F32 && c->precision != QS_PRECISION_F64) return fail(QS_ERR_INVALID, "bad precision");
    if (c->scenario < 0 || c->scenario >= QS_SCENARIO_COUNT) return fail(QS_ERR_UNSUPPORTED, "unsupported scenario");
    if (c->scenario == QS_SCENARIO_SWARM_VS_SWARM && c->num_agents < 2) return fail(QS_ERR_INVALID, "swarm_vs_swarm needs >= 2 drones");
    if (c->scenario == QS_SCENARIO_RUN_AWAY && c->num_agents < 2) return fail(QS_ERR_INVALID, "run_away needs >= 2 drones");
    {
        const bool o_scen = c->scenario == QS_SCENARIO_O_STATIC_SAME_GOAL || c->scenario == QS_SCENARIO_O_RANDOM ||
                            c->scenario == QS_SCENARIO_O_DYNAMIC_SAME_GOAL || c->scenario == QS_SCENARIO_O_SWAP_GOALS ||
                            c->scenario == QS_SCENARIO_O_EP_RAND_BEZIER;
        if (c->scenario != QS_SCENARIO_MIX && o_scen != (c->use_obstacles != 0))
            return fail(QS_ERR_INVALID, "obstacle scenario <=> use_obstacles");
    }
    if (c->use_obstacles) {
        if (c->obst_area[0] < 1 || c->obst_area[1] < 1 || c->obst_area[0] > 16 || c->obst_area[1] > 16)
            return fail(QS_ERR_UNSUPPORTED, "obst_area must be within [1,16]x[1,16]");
        if (c->num_obstacles < 1 || c->num_obstacles > QS_MAX_OBSTACLES
            || c->num_obstacles > c->obst_area[0] * c->obst_area[1]) return fail(QS_ERR_INVALID, "bad num_obstacles");
        if (c->obst_area[0] * c->obst_area[1] - c->num_obstacles < c->num_agents)
            return fail(QS_ERR_INVALID, "not enough free cells to spawn the drones");
    }
    if (handle_layout(c, spec_team_waves(c->num_agents) /* the largest layout qs_create may pick */, false).total > 160 * 1024)
        return fail(QS_ERR_UNSUPPORTED, "observation staging does not fit the 160 KiB LDS of a CU");
    if (c->dr_num_density < 0 || c->dr_num_density > QS_MAX_DR_CHOICES || c->dr_num_size < 0 || c->dr_num_size > QS_MAX_DR_CHOICES)
        return fail(QS_ERR_INVALID, "bad number of domain-randomisation choices");
    if (c->use_obstacles)
        for (int q = 0; q < c->dr_num_density; ++q)
            if (c->dr_obst_count[q] < 1 || c->dr_obst_count[q] > c->num_obstacles)
                return fail(QS_ERR_INVALID, "domain randomisation: obstacle counts must be in [1, num_obstacles]");
    if (c->sim_steps < 1 || c->ep_len < 1 || c->svd_period < 1 || c->svd_period > 255)
        return fail(QS_ERR_INVALID, "bad sim_steps/ep_len/svd_period");
    return QS_OK;
}

#include "qs_spec_cache.inc"

// ---- what the cache key of a specialised object hashes, and where the cache lives (declared in qs_spec_cache.inc) ----
static std::string lib_dir() {
    Dl_info info;
    if (dladdr((const void *)&qs_obs_dim, &info) && info.dli_fname) {
        std::string f = info.dli_fname;
        size_t k = f.rfind('/');
        return k == std::string::npos ? std::string(".") : f.substr(0, k);
    }
    return ".";
}
static uint64_t fnv1a(uint64_t h, const std::string &s) { for (unsigned char ch : s) { h ^= ch; h *= 1099511628211ull; } return h; }
static const char *const kSpecSources[] = {"qs_spec_kernels.hip", "qs_kernels.h", "qs_state_blk.h", "qs_state_rows.h", "qs_step_debug.h",
    "qs_lds_layout.h", "qs_scen_slots.h", "qs_nbr_obs.h", "qs_obs_rows.h", "qs_pair_responses.h", "qs_reset.h", "qs_device.h",
    "qs_scenarios.h", "qs_step_sem.h", "qs_xchg_dev.h", "qs_xchg_fused.h", "qs_step_flavours.inc", "qs_step_kernel_modes.inc", "qs_step_team_modes.inc",
    "qs_step_kernel.inc", "qs_step_team.inc"};

// key = hash(header text, kernel sources, flags); false if the sources are not next to the library
static bool spec_key(const std::string &header, std::string &key) {
    uint64_t h = fnv1a(14695981039346656037ull, header);
    h = fnv1a(h, kSpecFlags);
    h = fnv1a(h, kSpecFlagsF32);
    // (the header carries team width and precision: all strings, whichever applies)
    h = fnv1a(h, spec_team_flags(4)); h = fnv1a(h, spec_team_flags(8)); h = fnv1a(h, spec_sched_flags(0, QS_PRECISION_F32));
    if (const char *xf = getenv("QS_SPEC_EXTRA_FLAGS")) h = fnv1a(h, xf);   // e.g. -DQS_TIMING for tools/phase_timing.py
    const std::string dir = lib_dir();
    for (const char *src : kSpecSources) {
        std::string text;
        if (!read_file(dir + "/" + src, text)) return false;
        h = fnv1a(h, text);
    }
    for (const char *pub_name : {"quadswarm.h", "quadswarm_exchange.h"}) {   // the public headers the device code includes
        std::string pub;
        if (!read_file(dir + "/../../include/" + pub_name, pub)) return false;
        h = fnv1a(h, pub);
    }
    char t[32];
    snprintf(t, sizeof t, "%016llx", (unsigned long long)h);
    key = t;
    return true;
}
static std::string spec_cache_dir() {
    const char *ev = getenv("QS_SPEC_CACHE");
    return (ev && ev[0]) ? std::string(ev) : lib_dir() + "/spec_cache";
}

template <typename T> static int dalloc(qs_handle *h, T **ptr, size_t count) {
    void *q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    HIP_TRY(hipMalloc(&q, bytes));
    HIP_TRY(hipMemset(q, 0, bytes));
    h->allocs.push_back(q);
    *ptr = (T *)q;
    return QS_OK;
}

// the run-time reward coefficients (+ proximity slope) of `k` into a handle's rew_rt buffer
template <typename real> static int upload_reward_coeffs(const Consts<real> &k, const void *rew_rt) {
    real host[QS_REW_COUNT + 1];
    for (int q = 0; q < QS_REW_COUNT; ++q) host[q] = k.rew_coeff[q];
    host[QS_REW_COUNT] = k.prox_ratio;
    HIP_TRY(hipMemcpy((void *)rew_rt, host, sizeof host, hipMemcpyHostToDevice));
    return QS_OK;
}

template <typename real> static int create_typed(qs_handle *h) {
    const qs_config &c = h->cfg;
    const size_t E = c.num_envs, N = c.num_agents, T = E * N, D = h->obs_dim, M_ = c.num_obstacles;
    Ptrs<real> p;
    memset(&p, 0, sizeof p);
    int rc;
#define DA(field, count) if ((rc = dalloc(h, &p.field, (count))) != QS_OK) return rc
    const size_t EPB = QS_WAVE / N, NBLK = (E + EPB - 1) / EPB;   // environments per wave block, blocks
    {   // the state allocation (StateBlk, qs_state_blk.h): wave-blocked state rows, then the flat per-step outputs; 32-bit offsets
        const size_t R = sizeof(real);
        size_t row = 0;   // inside a block: array after array, each 64 lanes x comps elements (component rows or lane-major: qs_state_blk.h)
        auto rows = [&](size_t comps, size_t elem) { size_t o = row; row += comps * 64 * elem; return o; };
        const size_t o_pos = rows(3, R), o_vel = rows(3, R), o_rot = rows(9, R), o_omega = rows(3, R), o_rd = rows(4, R),
                     o_cd = rows(4, R), o_ou = rows(4, R), o_goal = rows(3, R), o_ring = rows(4, R), o_sums = rows(3, R),
                     o_flags = rows(1, 4), o_pair = rows(1, 8);
        const size_t block_bytes = row;
        typedef BlkOff<real> BO;
        if ((int)block_bytes != qs_block_bytes((int)R) || block_bytes != BO::bytes || o_pos != BO::pos || o_vel != BO::vel ||
            o_rot != BO::rot || o_omega != BO::omega || o_rd != BO::rot_damp || o_cd != BO::cmds_damp || o_ou != BO::ou ||
            o_goal != BO::goal || o_ring != BO::ring || o_sums != BO::sums || o_flags != BO::flags || o_pair != BO::pair)
            return fail(QS_ERR_INVALID, "state block layout out of step with BlkOff / qs_block_bytes()");
        size_t off = NBLK * block_bytes;
        auto carve = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
        const size_t o_newpair = carve(T * 8), o_reward = carve(T * R), o_done = carve(T), o_ohit = carve(T * 4);
        if (off >= ((size_t)1 << 32))
            return fail(QS_ERR_UNSUPPORTED, "per-drone state exceeds the 4 GiB a buffer resource addresses: use fewer envs per handle");
        char *blk = nullptr;
        if ((rc = dalloc(h, &blk, off)) != QS_OK) return rc;
        p.blk = {blk, (uint32_t)off, (uint32_t)block_bytes, (uint32_t)EPB, (uint32_t)o_pos, (uint32_t)o_vel, (uint32_t)o_rot,
                 (uint32_t)o_omega, (uint32_t)o_rd, (uint32_t)o_cd, (uint32_t)o_ou, (uint32_t)o_goal, (uint32_t)o_ring, (uint32_t)o_sums,
                 (uint32_t)o_flags, (uint32_t)o_pair, (uint32_t)o_newpair, (uint32_t)o_reward, (uint32_t)o_done, (uint32_t)o_ohit,
                 // lane-major <=> the specialised 8-wave team kernels step this handle
                 (uint32_t)(h->team == 8 ? 1 : 0)};
        // block 0's first row of each blocked array (what qs_buffers hands out; layout in include/quadswarm.h)
        p.pos = (real *)(blk + o_pos); p.vel = (real *)(blk + o_vel); p.rot = (real *)(blk + o_rot); p.omega = (real *)(blk + o_omega);
        p.rot_damp = (real *)(blk + o_rd); p.cmds_damp = (real *)(blk + o_cd); p.ou = (real *)(blk + o_ou); p.goal = (real *)(blk + o_goal);
        p.dist_ring = (real *)(blk + o_ring); p.dist_sums = (real *)(blk + o_sums); p.flags = (uint32_t *)(blk + o_flags);
        p.pair_mask = (uint64_t *)(blk + o_pair); p.new_pair_mask = (uint64_t *)(blk + o_newpair); p.reward = (real *)(blk + o_reward);
        p.done = (uint8_t *)(blk + o_done); p.obst_hit_idx = (int32_t *)(blk + o_ohit);
    }
    DA(obs, T * D); DA(rew_info, QS_RI_COUNT * T);
    {   // the per-environment rows of every step: ONE allocation of QS_ENVROW_COUNT rows of E 32-bit words (qs_state_rows.h), so that the team
        // kernels' one-step body reaches all of them through one buffer resource made from `unique_col`; everybody else uses the pointers
        uint32_t *rows = nullptr;
        if ((rc = dalloc(h, &rows, (size_t)QS_ENVROW_COUNT * E)) != QS_OK) return rc;
        p.unique_col = (uint64_t *)(rows + QS_ENVROW_unique * E); p.obst_new = (uint64_t *)(rows + QS_ENVROW_obst_new * E);
        p.room_new = (uint64_t *)(rows + QS_ENVROW_room_new * E); p.counters = (int32_t *)(rows + QS_ENVROW_counters * E);
        p.tick = (int32_t *)(rows + QS_ENVROW_tick * E); p.step_ctr = rows + QS_ENVROW_step_ctr * E;
    }
    DA(obst_pos, 2 * E * (M_ ? M_ : 1)); DA(ep_stats, QS_EPS_COUNT * T); DA(ep_counters, QS_CNT_COUNT * E);
    DA(run_sums, QS_SUM_COUNT * T); DA(ep_sums, QS_SUM_COUNT * T);
    DA(obst_count, E); DA(obst_size_env, E); DA(obst_density_env, E);
    {   // --quads_domain_random choice tables
        int32_t *dc = nullptr; real *dd = nullptr, *ds = nullptr;
        if ((rc = dalloc(h, &dc, QS_MAX_DR_CHOICES)) != QS_OK || (rc = dalloc(h, &dd, QS_MAX_DR_CHOICES)) != QS_OK
            || (rc = dalloc(h, &ds, QS_MAX_DR_CHOICES)) != QS_OK) return rc;
        real hd[QS_MAX_DR_CHOICES], hs[QS_MAX_DR_CHOICES];
        for (int q = 0; q < QS_MAX_DR_CHOICES; ++q) { hd[q] = (real)c.dr_density[q]; hs[q] = (real)c.dr_size[q]; }
        HIP_TRY(hipMemcpy(dc, c.dr_obst_count, sizeof c.dr_obst_count, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dd, hd, sizeof hd, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ds, hs, sizeof hs, hipMemcpyHostToDevice));
        p.dr_count = dc; p.dr_density = dd; p.dr_size = ds;
    }
    {   // until the first reset draws: the configured density / size
        std::vector<int32_t> cnt(E, c.num_obstacles);
        std::vector<real> sz(E, (real)c.obst_size), dn(E, (real)c.obst_density);
        HIP_TRY(hipMemcpy(p.obst_count, cnt.data(), E * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(p.obst_size_env, sz.data(), E * sizeof(real), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(p.obst_density_env, dn.data(), E * sizeof(real), hipMemcpyHostToDevice));
    }
    DA(scen_real, SR_COUNT * E); DA(scen_int, SI_COUNT * E); DA(scen_omap, 4 * E); DA(scenario_id, E); DA(ep_scenario, E);
    // the running episode's scenario: the resets of the full scenario set (mix: a new one per episode) keep it up to date; the three scenarios of
    {
        // the fast set never change it, so it is filled here (it stayed 0 = static_same_goal for o_static_same_goal / swarm_vs_swarm until round 5:
        // the per-scenario reward keys of the Sample Factory env carried the wrong name - found by tests/test_sf_env_vs_reference_gpu.py)
        std::vector<int32_t> sid(E, c.scenario);
        HIP_TRY(hipMemcpy(p.scenario_id, sid.data(), E * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    // QS_TIMING builds: phase stamps of workgroup 0, then {start, end, HW_ID, XCC_ID, wall start, wall end} of every workgroup
    DA(error_flag, 1); DA(reset_mask, E); DA(timing, 128 + 16 * NBLK);
#undef DA
    {   // run-time reward coefficients (+ proximity slope), read by every launch
        real *rw = nullptr;
        if ((rc = dalloc(h, &rw, QS_REW_COUNT + 1)) != QS_OK) return rc;
        p.rew_rt = rw;
        Consts<real> k;
        fill_consts<real>(c, k);
        if ((rc = upload_reward_coeffs(k, rw)) != QS_OK) return rc;
    }
    real *act = nullptr;
    if ((rc = dalloc(h, &act, 4 * T)) != QS_OK) return rc;
    h->d_actions = act;
    static_assert(sizeof(Ptrs<float>) == sizeof(Ptrs<double>), "layout");
    memcpy(&h->pf, &p, sizeof p);
    fill_consts<float>(c, h->kf);
    fill_consts<double>(c, h->kd);
    qs_buffers &b = h->bufs;
    memset(&b, 0, sizeof b);
    b.obs = p.obs; b.reward = p.reward; b.done = p.done; b.rew_info = p.rew_info; b.actions = act;
    b.pos = p.pos; b.vel = p.vel; b.omega = p.omega; b.rot = p.rot; b.thrust_rot_damp = p.rot_damp; b.thrust_cmds_damp = p.cmds_damp;
    b.ou_state = p.ou; b.goal = p.goal; b.flags = p.flags; b.obst_hit_idx = p.obst_hit_idx; b.col_pair_mask = p.pair_mask;
    b.new_pair_mask = p.new_pair_mask; b.unique_col_mask = p.unique_col; b.obst_new_mask = p.obst_new; b.room_new_mask = p.room_new;
    b.counters = p.counters; b.tick = p.tick; b.obst_pos = p.obst_pos; b.ep_stats = p.ep_stats; b.ep_counters = p.ep_counters;
    b.run_sums = p.run_sums; b.ep_sums = p.ep_sums;
    b.obst_count = p.obst_count; b.obst_size_env = p.obst_size_env; b.obst_density_env = p.obst_density_env;
    b.error_flag = p.error_flag; b.scenario_id = p.scenario_id; b.ep_scenario = p.ep_scenario; b.obs_dim = h->obs_dim;
    b.real_size = sizeof(real);
    b.state_block_bytes = (int32_t)p.blk.block_bytes; b.envs_per_block = (int32_t)EPB; b.state_lane_major = (int32_t)p.blk.lane_major;
    // what a deep copy of one reference env carries (quad_experience_replay.py:99-104 deep-copies the whole env): every
    // per-drone and per-env array except the noise-stream position (step_ctr: a restored env draws fresh noise, as the
    // reference's does from the global numpy stream) and the per-step outputs
    auto &sa = h->snap_arrays;
    sa.clear();
#define SNAP_T(field, comps) sa.push_back({(char *)p.field, sizeof(*p.field), (size_t)(comps), T, N, 0, 0, 0})
    // wave-blocked state array: `comps` rows of 64 elements, or (lane-major) the N drones of an env as ONE contiguous piece of N * comps
    // elements
#define SNAP_B(field, comps) sa.push_back(p.blk.lane_major ? qs_handle::SnapArray{(char *)p.field, sizeof(*p.field), 1, 64 * (size_t)(comps), N * (size_t)(comps), 0, EPB, (size_t)p.blk.block_bytes} \
                                                           : qs_handle::SnapArray{(char *)p.field, sizeof(*p.field), (size_t)(comps), 64, N, 0, EPB, (size_t)p.blk.block_bytes})
#define SNAP_E(field, comps) sa.push_back({(char *)p.field, sizeof(*p.field), (size_t)(comps), E, 1, 0, 0, 0})
    SNAP_B(pos, 3); SNAP_B(vel, 3); SNAP_B(rot, 9); SNAP_B(omega, 3); SNAP_B(rot_damp, 4); SNAP_B(cmds_damp, 4); SNAP_B(ou, 4);
    SNAP_B(goal, 3);
    SNAP_B(flags, 1); SNAP_B(pair_mask, 1); SNAP_T(new_pair_mask, 1); SNAP_T(obst_hit_idx, 1); SNAP_B(dist_ring, 4); SNAP_B(dist_sums, 3);
    SNAP_T(run_sums, QS_SUM_COUNT); sa.back().kind = 2;
    sa.push_back({(char *)p.obs, sizeof(real), 1, T * D, N * D, 1, 0, 0});                     // the observation that goes with the state
    SNAP_E(unique_col, 1); SNAP_E(obst_new, 1); SNAP_E(room_new, 1); SNAP_E(counters, QS_CNT_COUNT); SNAP_E(tick, 1);
    SNAP_E(scen_real, SR_COUNT); SNAP_E(scen_int, SI_COUNT); SNAP_E(scen_omap, 4); SNAP_E(scenario_id, 1);
    SNAP_E(obst_count, 1); SNAP_E(obst_size_env, 1); SNAP_E(obst_density_env, 1);
    sa.push_back({(char *)p.obst_pos, sizeof(real), 2, E * (M_ ? M_ : 1), (M_ ? M_ : 1), 0, 0, 0});
#undef SNAP_T
#undef SNAP_B
#undef SNAP_E
    h->snap_bytes = 0;
    for (const auto &a : sa) h->snap_bytes += (a.elem * a.comps * a.per_env + 15) & ~(size_t)15;
    return QS_OK;
}

// ---- the generic kernels (qs_step_flavours.inc), named once: qs_create raises the dynamic-LDS limit on every entry, launch_step and
// launch_reset look theirs up.  A kernel that does not exist (the single-wave body has no gated mode) has fn == nullptr. ----
struct KernelEntry { const void *fn; int threads; };
enum { MODE_STEP = 0, MODE_ROLLOUT, MODE_GATED, MODE_COUNT };
#define QS_BOTH(KERNEL, THREADS) {{(const void *)KERNEL<float>, THREADS}, {(const void *)KERNEL<double>, THREADS}}
static const KernelEntry kStepKernels[2][2][MODE_COUNT][2] = {   // [team][full scenario set][mode][float64]
    {{QS_BOTH(qs_step_kernel, QS_WAVE), QS_BOTH(qs_rollout_kernel, QS_WAVE), {}},
     {QS_BOTH(qs_step_kernel_full, QS_WAVE), QS_BOTH(qs_rollout_kernel_full, QS_WAVE), {}}},
    {{QS_BOTH(qs_step_team, QS_TEAM_THREADS), QS_BOTH(qs_rollout_team, QS_TEAM_THREADS), QS_BOTH(qs_gated_team, QS_TEAM_THREADS)},
     {QS_BOTH(qs_step_team_full, QS_TEAM_THREADS), QS_BOTH(qs_rollout_team_full, QS_TEAM_THREADS), QS_BOTH(qs_gated_team_full, QS_TEAM_THREADS)}}};
#undef QS_BOTH
// the one-step team kernels with the fused exchange epilogue (qs_step_team_modes.inc; float32 only, like qs_set_obs_exchange): what
// launch_step takes instead of the table's entry while an exchange is attached
#if QS_XCHG_INLINE
static const KernelEntry kStepXchgKernels[2] = {{nullptr, 0}, {nullptr, 0}};   // (the run-time test lives in the table's kernels)
#else
static const KernelEntry kStepXchgKernels[2] = {   // [full scenario set]
    {(const void *)qs_step_team_x<float>, QS_TEAM_THREADS}, {(const void *)qs_step_team_full_x<float>, QS_TEAM_THREADS}};
#endif
static const KernelEntry kResetKernels[2][2] = {   // [full scenario set][float64]
    {{(const void *)qs_reset_kernel<float, false>, QS_WAVE}, {(const void *)qs_reset_kernel<double, false>, QS_WAVE}},
    {{(const void *)qs_reset_kernel<float, true>, QS_WAVE}, {(const void *)qs_reset_kernel<double, true>, QS_WAVE}}};
// every kernel of a table (`count` entries from its first) may ask for `bytes` of dynamic LDS, above the 64 KiB a kernel gets without asking
static bool raise_lds_limit(const KernelEntry *k, size_t count, int bytes) {
    for (; count--; ++k)
        if (k->fn && hipFuncSetAttribute(k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    return true;
}
static const char *const kNoXchgKernel = "qs_set_obs_exchange: this handle's kernels have no one-step kernel with the exchange epilogue (qs_spec_step_x / qs_step_team_x: float32 team kernels, not built with -DQS_XCHG_INLINE=1)";
static const char *const kGatedNeedsTeam = "resident-state stepping lives in the team kernels (batches up to ~8 waves per CU, see qs_kernel_flavor): larger batches are bandwidth-bound, not launch-bound";

extern "C" {

int qs_version(void) { return QS_VERSION; }
size_t qs_sizeof_config(void) { return sizeof(qs_config); }
const char *qs_last_error(void) { return g_last_error.c_str(); }

int qs_obs_dim(const qs_config *c) { return qs_self_dim(c->obs_repr) + 6 * c->num_neighbors + (c->use_obstacles ? 9 : 0); }

int qs_default_config(qs_config *c, int32_t num_envs, int32_t num_agents) {
    // Crazyflie constants as derived by the reference at construction time; the python
    // host layer (quad-swarm-rl_amd/airframe.py) re-derives them from the link geometry and overrides these.
    memset(c, 0, sizeof *c);
    c->num_envs = num_envs; c->num_agents = num_agents; c->precision = QS_PRECISION_F32; c->seed = 0;
    c->mass = 0.028000000000000008; c->arm = 0.04596194077712559;
    c->inertia[0] = 1.3669232142857143e-05; c->inertia[1] = 1.4356732142857143e-05; c->inertia[2] = 2.656158333333334e-05;
    const double pc[4][3] = {{-0.0325, -0.0325, 0}, {-0.0325, 0.0325, 0}, {0.0325, 0.0325, 0}, {0.0325, -0.0325, 0}};
    const double ccw[4] = {-1, 1, -1, 1};
    for (int m = 0; m < 4; ++m) {
        for (int q = 0; q < 3; ++q) c->prop_cross[m][q] = pc[m][q];
        c->prop_ccw[m] = ccw[m];
        c->thrust_max[m] = 9.81 * c->mass * 1.9 / 4.0;
        c->torque_max[m] = 0.006 * c->thrust_max[m];
    }
    c->dt = 1.0 / 200.0; c->sim_steps = 2;
    c->motor_tau_up = c->motor_tau_down = 4 * c->dt / (0.15 + 1e-6);
    c->motor_linearity = 1.0; c->vel_damp = 0; c->damp_omega_quadratic = 0; c->omega_max = 40.0; c->gravity = 9.81;
    // the numba path (floor_mode below): OUNoiseNumba keeps theta / sigma in float32 members (numba_utils.py:67-74) - the values the jitted
    // reference computes with are the float32 roundings widened back to double (config.make_config: numba_float32_ou)
    c->thrust_noise_sigma = (double)(float)(0.2 * 0.05); c->ou_theta = (double)(float)0.15;
    c->ep_len = (int)(15.0 / (c->dt * c->sim_steps));
    c->room_lo[0] = -5; c->room_lo[1] = -5; c->room_lo[2] = 0; c->room_hi[0] = 5; c->room_hi[1] = 5; c->room_hi[2] = 10;
    c->floor_mode = QS_FLOOR_NUMBA;
    { double s = 0; int n = 0; do { s += c->dt; ++n; } while (!(s > 0.5)); c->svd_period = n; }
    c->sense_noise = 1; c->obs_repr = QS_OBS_XYZ_VXYZ_R_OMEGA;
    c->pos_norm_std = 0.005; c->vel_norm_std = 0.01; c->gyro_noise_density = 0.000175;
    c->num_neighbors = num_agents > 6 ? 6 : num_agents - 1;
    c->use_downwash = 0; c->use_obstacles = 0; c->scenario = QS_SCENARIO_STATIC_SAME_GOAL;
    c->collision_threshold = 2.0 * c->arm; c->collision_falloff_threshold = 4.0 * c->arm;
    const double rc[QS_REW_COUNT] = {1.0, 0.05, 1.0, 1.0, 0.1, 5.0, 4.0, 5.0};
    for (int q = 0; q < QS_REW_COUNT; ++q) c->rew_coeff[q] = rc[q];
    c->spawn_box = 2.0; c->approach_goal_metric = 0.5;
    for (int q = 0; q < 3; ++q) { c->nbr_clip_pos[q] = 10.0; c->nbr_clip_vel[q] = 6.0; }
    c->obst_size = 1.0; c->obst_density = 0.2; c->obst_area[0] = 6; c->obst_area[1] = 6; c->num_obstacles = 0;
    c->write_rew_info = 1;
    c->episode_sums = 0;
    return QS_OK;
}

int qs_create(const qs_config *cfg, int device, qs_handle **out) {
    if (!cfg || !out) return fail(QS_ERR_INVALID, "null argument");
    int rc = validate(cfg);
    if (rc != QS_OK) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(QS_ERR_HIP, "no such HIP device");
    HIP_TRY(hipSetDevice(device));
    qs_handle *h = new qs_handle();
    h->cfg = *cfg;
    h->device = device;
    h->real_size = cfg->precision == QS_PRECISION_F64 ? 8 : 4;
    h->obs_dim = qs_obs_dim(cfg);
    h->epb = QS_WAVE / cfg->num_agents;
    h->blocks = (cfg->num_envs + h->epb - 1) / h->epb;
    // Kernel flavour: a team of 4 waves per workgroup shortens the per-step critical path when the batch cannot fill the
    // chip anyway (<= 8 waves per CU, team_default); the single-wave kernels do less total work per drone and win on throughput.
    // QS_TEAM=0/1 in the environment overrides the choice (both flavours produce the same results); 4 / 8 also name the specialised
    // team kernels' waves per workgroup.
    const char *const team_env = getenv("QS_TEAM");
    const char team_ch = team_env ? team_env[0] : 0;
    {
        hipDeviceProp_t prop;
        int cus = 256;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        h->team = team_default(h->blocks, cus, cfg->num_agents) ? QS_TEAM_WAVES : 0;
        h->cus = cus;
        if (team_ch == '0') h->team = 0;
        else if (team_ch == '1' || team_ch == '4' || team_ch == '8') h->team = QS_TEAM_WAVES;
    }
    // Config-specialised kernels.  QS_SPEC = "jit" (default): use the cached code object of this configuration, building it
    // first if needed (one hipcc run, ~5 s, cached next to the library); "cache": use it only if it is already there;
    // "off": always the generic kernels.  Any failure falls back to the generic kernels (same results, slower).
    {
        const char *ev = getenv("QS_SPEC");
        const std::string mode = (ev && ev[0]) ? ev : "jit";
        const int spec_team = h->team ? (team_ch == '4' ? 4 : (team_ch == '8' ? 8 : spec_team_waves(cfg->num_agents))) : 0;
        const LdsLayout sl = handle_layout(cfg, spec_team, true);
        const bool require = mode == "require";
        if (mode == "off" || mode == "0") h->spec_note = "QS_SPEC=off";
        else if (sl.total > 64 * 1024) h->spec_note = "LDS layout above the 64 KiB a module-loaded kernel gets";
        else {
            const std::string path = spec_ensure(cfg, spec_team, mode == "jit" || require);
            if (!path.empty()) {
                if (hipModuleLoad(&h->spec_mod, path.c_str()) == hipSuccess &&
                    hipModuleGetFunction(&h->spec_step, h->spec_mod, "qs_spec_step") == hipSuccess &&
                    hipModuleGetFunction(&h->spec_rollout, h->spec_mod, "qs_spec_rollout") == hipSuccess &&
                    hipModuleGetFunction(&h->spec_reset, h->spec_mod, "qs_spec_reset") == hipSuccess) {
                    h->team = spec_team;   // specialised kernels in use
                    if (spec_team > 0 && hipModuleGetFunction(&h->spec_gated, h->spec_mod, "qs_spec_gated") != hipSuccess) {
                        (void)hipGetLastError(); h->spec_gated = nullptr; }
                    // (absent from float64 objects and from -DQS_XCHG_INLINE=1 builds: qs_set_obs_exchange refuses those)
                    if (spec_team > 0 && hipModuleGetFunction(&h->spec_step_x, h->spec_mod, "qs_spec_step_x") != hipSuccess) {
                        (void)hipGetLastError(); h->spec_step_x = nullptr; }
                } else {
                    (void)hipGetLastError();
                    if (h->spec_mod) { (void)hipModuleUnload(h->spec_mod); h->spec_mod = nullptr; }
                    h->spec_step = h->spec_rollout = h->spec_reset = h->spec_gated = h->spec_step_x = nullptr;
                    h->spec_note = "cannot load " + path;
                }
            } else {
                h->spec_note = g_last_error;
            }
        }
        // The fallback is LOUD: one line on stderr, the reason kept for qs_spec_status(), and QS_SPEC=require turns it into an error
        // (the generic kernels give the same results - tests/test_fp32_parity_gpu.py - at ~1.3x the step time).
        if (!h->spec_step && mode != "off" && mode != "0") {
            if (require && sl.total <= 64 * 1024) { const std::string why = h->spec_note; delete h;
                return fail(QS_ERR_UNSUPPORTED, "QS_SPEC=require: no config-specialised kernels: " + why); }
            fprintf(stderr, "quadswarm_hip: WARNING: running the GENERIC step kernels (%s)\n", h->spec_note.c_str());
        }
    }
    h->lds = handle_layout(cfg, h->team, h->spec_step != nullptr);
    h->full = scenario_is_full(cfg->scenario);
    rc = (h->real_size == 8) ? create_typed<double>(h) : create_typed<float>(h);
    if (rc == QS_OK) {
        if (hipMalloc((void **)&h->d_state_buf, sizeof(double) * QS_MAX_AGENTS * QS_STATE_STRIDE) != hipSuccess ||
            hipMalloc((void **)&h->d_tick_io, sizeof(int32_t)) != hipSuccess ||
            hipHostMalloc((void **)&h->h_mask, (size_t)cfg->num_envs) != hipSuccess)
            rc = fail(QS_ERR_HIP, "allocation failed");
    }
    if (rc != QS_OK) { qs_destroy(h); return rc; }
    if (h->lds.total > 64 * 1024 && !(raise_lds_limit(&kStepKernels[0][0][0][0], sizeof kStepKernels / sizeof(KernelEntry), h->lds.total) &&
                                      raise_lds_limit(&kStepXchgKernels[0], sizeof kStepXchgKernels / sizeof(KernelEntry), h->lds.total) &&
                                      raise_lds_limit(&kResetKernels[0][0], sizeof kResetKernels / sizeof(KernelEntry), h->lds.total))) {
        qs_destroy(h);
        return fail(QS_ERR_HIP, "cannot raise dynamic LDS limit");
    }
    *out = h;
    return QS_OK;
}

// 1 if the handle runs config-specialised kernels, 0 if the generic ones
int qs_is_specialized(qs_handle *h) { return (h && h->spec_step) ? 1 : 0; }
int qs_spec_status(qs_handle *h, char *why_out, int cap) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    if (why_out && cap > 0) { snprintf(why_out, (size_t)cap, "%s", h->spec_note.c_str()); }
    return h->spec_step ? 1 : 0;
}
// bit 0: config-specialised code object, bit 1: team kernels, bit 2: full scenario set, bit 3: an exchange is attached (qs_step launches
// the `_x` kernel, see launch_step), bits 8..15: waves per workgroup
int qs_kernel_flavor(qs_handle *h) {
    return h ? ((h->spec_step ? 1 : 0) | (h->team ? 2 : 0) | (h->full ? 4 : 0) | (h->pf.xchg ? 8 : 0) | ((h->team ? h->team : 1) << 8)) : 0;
}

int qs_destroy(qs_handle *h) {
    if (!h) return QS_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->spec_mod) { (void)hipModuleUnload(h->spec_mod); h->spec_mod = nullptr; }
    if (h->snap_pool) (void)hipFree(h->snap_pool);
    for (void *q : h->allocs) (void)hipFree(q);
    if (h->d_state_buf) (void)hipFree(h->d_state_buf);
    if (h->d_tick_io) (void)hipFree(h->d_tick_io);
    if (h->h_mask) (void)hipHostFree(h->h_mask);
    if (h->d_tape) (void)hipFree(h->d_tape);
    if (h->d_tape_pos) (void)hipFree(h->d_tape_pos);
    if (h->d_gate) (void)hipFree(h->d_gate);
    if (h->gate_stream) (void)hipStreamDestroy(h->gate_stream);
    if (h->gate_ev_in) (void)hipEventDestroy(h->gate_ev_in);
    if (h->gate_ev_out) (void)hipEventDestroy(h->gate_ev_out);
    for (auto &ev : h->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    free(h->pilot);
    if (h->summary) (void)hipFree(h->summary);
    delete h;
    return QS_OK;
}

}  // extern "C"

static int launch_reset(qs_handle *h, hipStream_t s) {
    if (h->d_tape) {
        hipError_t e = (hipError_t)qs_tape_launch(0, &h->cfg, h->obs_dim, h->full ? 1 : 0, h->real_size,
                                                 h->real_size == 8 ? (const void *)&h->kd : (const void *)&h->kf, &h->pf, nullptr, s);
        if (e != hipSuccess) return fail(QS_ERR_HIP, std::string("tape reset kernel: ") + hipGetErrorString(e));
        return QS_OK;
    }
    Ptrs<float> pf = h->pf;   // this launch's pointers: the observation rows go to the target of qs_set_obs_target, if one is set
    if (h->obs_target) pf.obs = (float *)h->obs_target;
    void *args[] = {h->real_size == 8 ? (void *)&h->kd : (void *)&h->kf, &pf, &h->lds, &h->epb};   // (pf: as in launch_step)
    const KernelEntry &k = kResetKernels[h->full][h->real_size == 8];
    if (h->spec_reset) HIP_TRY(hipModuleLaunchKernel(h->spec_reset, h->blocks, 1, 1, QS_WAVE, 1, 1, h->lds.total, s, args, nullptr));
    else HIP_TRY(hipLaunchKernel(k.fn, dim3(h->blocks), dim3(k.threads), args, h->lds.total, s));
    return QS_OK;
}

static int launch_step(qs_handle *h, const void *actions, hipStream_t s, int ksteps = 1, bool gated = false) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (h->profiling) {
        if (h->events_used == h->events.size()) {
            hipEvent_t a, b;
            HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
            h->events.emplace_back(a, b);
        }
        e0 = h->events[h->events_used].first; e1 = h->events[h->events_used].second;
        ++h->events_used;
        HIP_TRY(hipEventRecord(e0, s));
    }
    if (h->d_tape) {   // noise-tape flavour: one launch per control step
        const size_t stride = (size_t)h->cfg.num_envs * h->cfg.num_agents * 4 * (size_t)h->real_size;
        for (int t = 0; t < ksteps; ++t) {
            hipError_t e = (hipError_t)qs_tape_launch(1, &h->cfg, h->obs_dim, h->full ? 1 : 0, h->real_size,
                                                     h->real_size == 8 ? (const void *)&h->kd : (const void *)&h->kf, &h->pf,
                                                     (const char *)actions + stride * t, s);
            if (e != hipSuccess) return fail(QS_ERR_HIP, std::string("tape step kernel: ") + hipGetErrorString(e));
        }
        if (h->profiling) HIP_TRY(hipEventRecord(e1, s));
        return QS_OK;
    }
    Ptrs<float> pf = h->pf;   // this launch's pointers (qs_set_obs_target)
    if (h->obs_target) pf.obs = (float *)h->obs_target;
    // the fused exchange epilogue exists in the one-step kernels only: a multi-step launch would advance the environments without sending
    // their rows and desynchronise push / wait sequence numbers (qs_step_many splits into single steps while an exchange is set)
    if (pf.xchg != nullptr && ksteps > 1)
        return fail(QS_ERR_UNSUPPORTED, "multi-step launches do not exchange observation rows: qs_set_obs_exchange is active");
    // the multi-step team kernels read the exchange slot as their gate (qs_step_team.inc)
    // An attached exchange selects the one-step kernel WITH the epilogue (`..._x`); without one the launch runs the kernel that has no
    // exchange code at all.  A captured graph freezes `pf` by value and with it this choice: attaching, detaching or replacing the exchange
    // means capturing again.
    const bool with_xchg = pf.xchg != nullptr && !gated;
    if (gated) pf.xchg = (const qsx::XchgDev *)h->d_gate;
    // (the one-step kernels have no `ksteps` parameter: a launch takes as many arguments as its kernel declares; Ptrs<float> and
    // Ptrs<double> are the same bytes)
    void *args[] = {h->real_size == 8 ? (void *)&h->kd : (void *)&h->kf, &pf, (void *)&actions, &h->lds, &h->epb, &ksteps};
    if (h->spec_step) {
        if (gated && !h->spec_gated)
            return fail(QS_ERR_UNSUPPORTED, "the specialised code object of this handle has no resident-state kernel");
        if (with_xchg && !h->spec_step_x) return fail(QS_ERR_UNSUPPORTED, kNoXchgKernel);
        HIP_TRY(hipModuleLaunchKernel(gated ? h->spec_gated : (ksteps == 1 ? (with_xchg ? h->spec_step_x : h->spec_step) : h->spec_rollout), h->blocks, 1, 1,
                                      h->team ? QS_WAVE * h->team : QS_WAVE, 1, 1, h->lds.total, s, args, nullptr));
    } else {
        const KernelEntry &k = with_xchg ? kStepXchgKernels[h->full]
                                         : kStepKernels[h->team != 0][h->full][gated ? MODE_GATED : (ksteps == 1 ? MODE_STEP : MODE_ROLLOUT)][h->real_size == 8];
        if (!k.fn) return fail(QS_ERR_UNSUPPORTED, with_xchg ? kNoXchgKernel : kGatedNeedsTeam);
        HIP_TRY(hipLaunchKernel(k.fn, dim3(h->blocks), dim3(k.threads), args, h->lds.total, s));
    }
    if (h->profiling) HIP_TRY(hipEventRecord(e1, s));
    return QS_OK;   // the auto-reset is the tail of the step kernel itself
}

// the replay wrapper's step() / new_episode() for every environment, behind each control step (qs_replay_enable)
static int launch_replay(qs_handle *h, hipStream_t s) {
    hipLaunchKernelGGL(qs_replay_kernel, dim3(h->cfg.num_envs), dim3(QS_WAVE), 0, s, h->rp);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

#include "qs_gate.inc"

extern "C" {

int qs_reset(qs_handle *h, const uint8_t *env_mask_host, void *stream) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    if (int jr = gate_join_stream(h, (hipStream_t)stream)) return jr;
    hipStream_t s = (hipStream_t)stream;
    const int E = h->cfg.num_envs;
    for (int e = 0; e < E; ++e) h->h_mask[e] = env_mask_host ? (env_mask_host[e] ? 1 : 0) : 1;
    HIP_TRY(hipMemcpyAsync(h->pf.reset_mask, h->h_mask, (size_t)E, hipMemcpyHostToDevice, s));
    // the replay wrapper's bookkeeping of an explicit reset (before the reset kernel zeroes the running sums); the reset that starts the
    // very first episode is already in the history (qs_replay_enable)
    if (h->replay_on && h->replay_stepped) {
        hipLaunchKernelGGL(qs_replay_reset_kernel, dim3((E + QS_WAVE - 1) / QS_WAVE), dim3(QS_WAVE), 0, s, h->rp,
                           (const uint8_t *)h->pf.reset_mask);
        HIP_TRY(hipGetLastError());
    }
    int rc = launch_reset(h, s);
    if (rc != QS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));   // h_mask is reused by the next call
    return QS_OK;
}

int qs_step(qs_handle *h, const void *actions_dev, void *stream) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    if (h->gate_pending) { if (int jr = gate_join_stream(h, (hipStream_t)stream)) return jr; }
    int rc = launch_step(h, actions_dev ? actions_dev : h->d_actions, (hipStream_t)stream);
    if (rc == QS_OK && h->replay_on) { rc = launch_replay(h, (hipStream_t)stream); h->replay_stepped = true; }
    return rc;
}

int qs_step_many(qs_handle *h, const void *actions_dev, int32_t k, void *stream) {
    if (!h || !actions_dev || k < 0) return fail(QS_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (h->gate_pending) { if (int jr = gate_join_stream(h, (hipStream_t)stream)) return jr; }
    const size_t stride = (size_t)h->cfg.num_envs * h->cfg.num_agents * 4 * h->real_size;
    // per-step HIP events / the replay kernel behind every step / the fused exchange epilogue: one launch per control step
    if (h->profiling || h->replay_on || h->pf.xchg) {
        for (int32_t t = 0; t < k; ++t) {
            int rc = launch_step(h, (const char *)actions_dev + stride * t, (hipStream_t)stream, 1);
            if (rc == QS_OK && h->replay_on) { rc = launch_replay(h, (hipStream_t)stream); h->replay_stepped = true; }
            if (rc != QS_OK) return rc;
        }
        return QS_OK;
    }
    // open-loop rollout: the step kernel keeps the state in registers across up to QS_STEPS_PER_LAUNCH control steps
    const int32_t per = 64;
    for (int32_t t = 0; t < k; t += per) {
        int rc = launch_step(h, (const char *)actions_dev + stride * t, (hipStream_t)stream, (k - t) < per ? (k - t) : per);
        if (rc != QS_OK) return rc;
    }
    return QS_OK;
}

int qs_sync(qs_handle *h, void *stream) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    if (int jr = gate_join_host(h)) return jr;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return QS_OK;
}

int qs_get_buffers(qs_handle *h, qs_buffers *out) {
    if (!h || !out) return fail(QS_ERR_INVALID, "null argument");
    *out = h->bufs;
    return QS_OK;
}

// what qs_pilot.hip (include/quadswarm_control.h) needs of this unit: the handle's struct and the error text are private here
int qs_pilot_fail(int code, const char *msg) { return fail(code, msg); }
int qs_pilot_view(qs_handle *h, QsPilotView *out) {
    if (!h || !out) return fail(QS_ERR_INVALID, "null handle");
    *out = {&h->cfg, h->pf.blk, h->device, h->real_size, h->cus, h->gate_pending ? 1 : 0, h->d_actions, &h->pilot};
    return QS_OK;
}

// what qs_episode_summary.hip (include/quadswarm_summary.h) needs of this unit
int qs_summary_fail(int code, const char *msg) { return fail(code, msg); }
int qs_summary_view(qs_handle *h, QsSummaryView *out) {
    if (!h || !out) return fail(QS_ERR_INVALID, "null handle");
    *out = {h->cfg.num_envs, h->cfg.num_agents, h->device, h->real_size, h->cfg.ep_len, h->cfg.episode_sums, h->gate_pending ? 1 : 0,
            h->pf.done, h->pf.ep_sums, h->pf.ep_stats, h->pf.ep_counters, h->pf.ep_scenario, h->pf.scenario_id,
            h->replay_on ? h->rp.ep_saved : nullptr, h->replay_on ? h->rp.last_steps : nullptr, &h->summary};
    return QS_OK;
}

// what qs_neighbor_ids.hip (include/quadswarm_neighbors.h) needs of this unit
int qs_neighbors_fail(int code, const char *msg) { return fail(code, msg); }
int qs_neighbors_view(qs_handle *h, QsNeighborsView *out) {
    if (!h || !out) return fail(QS_ERR_INVALID, "null handle");
    *out = {&h->cfg, h->pf.blk, h->device, h->real_size, h->cus, h->gate_pending ? 1 : 0, h->bufs.obs, h->obs_dim,
            qs_self_dim(h->cfg.obs_repr)};
    return QS_OK;
}

int qs_set_obs_target(qs_handle *h, void *obs_dev) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    if (obs_dev && h->replay_on)
        return fail(QS_ERR_UNSUPPORTED, "qs_set_obs_target: the device-side replay wrapper restores observations into qs_buffers.obs");
    if (obs_dev && h->d_tape) return fail(QS_ERR_UNSUPPORTED, "qs_set_obs_target: not available while a noise tape is set");
    h->obs_target = obs_dev;
    return QS_OK;
}

extern "C" void *qs_xchg_fused_desc(struct qs_xchg *x, int32_t blocks, int32_t auto_ack, int64_t *n_out);
extern "C" const char *qs_xchg_last_error(void);
extern "C" int qs_xchg_row_layout_is(struct qs_xchg *x, int32_t cols, int32_t q0, int32_t q1);
int qs_set_obs_exchange(qs_handle *h, struct qs_xchg *xchg, int32_t auto_ack) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    if (!xchg) { h->pf.xchg = nullptr; return QS_OK; }
    if (!h->team || h->real_size != 4)
        return fail(QS_ERR_UNSUPPORTED, "qs_set_obs_exchange: the fused exchange lives in the float32 team kernels (small batches); use qs_xchg_push for this handle");
    if (h->d_tape) return fail(QS_ERR_UNSUPPORTED, "qs_set_obs_exchange: not available while a noise tape is set");
    // the exchange runs in a kernel of its own: a handle without it says so here instead of stepping without exchanging
    if (h->spec_step ? !h->spec_step_x : !kStepXchgKernels[h->full].fn) return fail(QS_ERR_UNSUPPORTED, kNoXchgKernel);
    HIP_TRY(hipSetDevice(h->device));
    int64_t n = 0;
    void *desc = qs_xchg_fused_desc(xchg, h->blocks, auto_ack, &n);
    if (!desc) return fail(QS_ERR_INVALID, std::string("qs_set_obs_exchange: ") + qs_xchg_last_error());
    if (n != (int64_t)h->cfg.num_envs * h->cfg.num_agents * h->obs_dim)
        return fail(QS_ERR_INVALID, "qs_set_obs_exchange: the endpoint's rows * cols must be E*N * obs_dim");
    {   // the kernels rebuild a QS_WIRE_Q8 layout from their own constants: the neighbour block behind the self observation
        const int self_dim = qs_self_dim(h->cfg.obs_repr);
        if (!qs_xchg_row_layout_is(xchg, h->obs_dim, self_dim, self_dim + 6 * h->cfg.num_neighbors))
            return fail(QS_ERR_INVALID, "qs_set_obs_exchange: the endpoint's row layout is not this configuration's (QS_WIRE_Q8: q0 = self columns, q1 = q0 + 6 * visible neighbours)");
    }
    h->pf.xchg = (const qsx::XchgDev *)desc;
    return QS_OK;
}

int qs_set_reward_coeffs(qs_handle *h, const double *coeffs) {
    if (!h || !coeffs) return fail(QS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    for (int q = 0; q < QS_REW_COUNT; ++q) h->cfg.rew_coeff[q] = coeffs[q];
    fill_consts<float>(h->cfg, h->kf);
    fill_consts<double>(h->cfg, h->kd);
    // the kernels read the coefficients from this buffer on every launch - also launches replayed from a captured HIP graph
    return h->real_size == 8 ? upload_reward_coeffs(h->kd, h->pf.rew_rt) : upload_reward_coeffs(h->kf, h->pf.rew_rt);
}

int qs_check_errors(qs_handle *h) {
    if (!h) return fail(QS_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    // the gated kernel's stream is non-blocking: a null-stream copy does not wait for it by itself
    if (int jr = gate_join_host(h)) return jr;
    uint32_t f = 0;
    HIP_TRY(hipMemcpy(&f, h->pf.error_flag, sizeof f, hipMemcpyDeviceToHost));
    if (f) return fail(QS_ERR_NAN_REWARD, "QuadEnv: reward is Nan");
    return QS_OK;
}

}  // extern "C"

#include "qs_snapshot_replay.inc"
#include "qs_env_debug.inc"

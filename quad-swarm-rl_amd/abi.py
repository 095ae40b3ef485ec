"""The C ABI of the public headers (include/quadswarm.h, quadswarm_exchange.h, quadswarm_control.h, quadswarm_summary.h, quadswarm_neighbors.h, quadswarm_encoder.h,
quadswarm_valuemap.h, quadswarm_attention.h),
restated once: the constants under the headers' names, the structs with the headers' field names, one prototype table per header.  Written by
hand and checked against the headers compiled as C (tests/test_abi_layout.py; quadswarm_valuemap.h: tests/test_value_map_cpu.py; quadswarm_attention.h:
tests/test_attention_weights_cpu.py).  Plain ctypes: importing this loads no library and needs no GPU.
"""
import ctypes as C

# ---- include/quadswarm.h ----
QS_MAX_AGENTS = 64
QS_MAX_OBSTACLES = 64
QS_MAX_DR_CHOICES = 8
QS_STATE_STRIDE = 35
QS_OK, QS_ERR_INVALID, QS_ERR_HIP, QS_ERR_NAN_REWARD, QS_ERR_UNSUPPORTED = 0, -1, -2, -3, -4
QS_REW_COUNT = 8       # qs_config.rew_coeff (config.REW_COEFF_KEYS)
QS_RI_COUNT = 17       # rows of qs_buffers.rew_info (config.REW_INFO_KEYS)
QS_CNT_COUNT = 11      # rows of qs_buffers.counters / ep_counters (config.COUNTER_KEYS)
QS_EPS_COUNT = 6       # rows of qs_buffers.ep_stats (config.EPS_KEYS)
QS_SUM_ACT = QS_RI_COUNT            # rows of qs_buffers.run_sums / ep_sums: the reward terms, then sum a_k ...
QS_SUM_ACT2 = QS_RI_COUNT + 4       # ... and sum a_k^2 of the 4 raw actions
QS_SUM_COUNT = QS_RI_COUNT + 8
QS_REPLAY_STATS = 9
# ---- include/quadswarm_summary.h: rows = scenario id, columns of the double table `sums` and of the int64 table `counts` ----
QS_SUMM_SCENARIOS = 16
QS_SUMM_D_DIST_1S, QS_SUMM_D_DIST_3S, QS_SUMM_D_DIST_5S = 0, 1, 2                                           # row = ep_scenario, not replayed
QS_SUMM_D_SUCCESS, QS_SUMM_D_DEADLOCK, QS_SUMM_D_COL, QS_SUMM_D_NBR_COL, QS_SUMM_D_OBST_COL = 3, 4, 5, 6, 7   # row = ep_scenario, not replayed
QS_SUMM_D_REW = 8                                    # QS_RI_COUNT columns; row = ep_scenario, every episode (as the next three)
QS_SUMM_D_TRUE_REWARD = QS_SUMM_D_REW + QS_RI_COUNT
QS_SUMM_D_ACT_MEAN = QS_SUMM_D_TRUE_REWARD + 1       # 4 columns
QS_SUMM_D_ACT_STD = QS_SUMM_D_ACT_MEAN + 4           # 4 columns
QS_SUMM_D_START_REW_POS = QS_SUMM_D_ACT_STD + 4      # row = scenario_id (the scenario that starts), as the next
QS_SUMM_D_START_REW_CRASH = QS_SUMM_D_START_REW_POS + 1
QS_SUMM_D_COUNT = QS_SUMM_D_START_REW_CRASH + 1
QS_SUMM_I_EPISODES, QS_SUMM_I_REPLAYED = 0, 1        # row = ep_scenario
QS_SUMM_I_CNT = 2                                    # QS_CNT_COUNT columns; row = ep_scenario, not replayed
QS_SUMM_I_COL_REPLAY = QS_SUMM_I_CNT + QS_CNT_COUNT  # row = ep_scenario, replayed (as the next)
QS_SUMM_I_OBST_REPLAY = QS_SUMM_I_COL_REPLAY + 1
QS_SUMM_I_OVERRUN = QS_SUMM_I_OBST_REPLAY + 1        # row = ep_scenario
QS_SUMM_I_START_EPISODES = QS_SUMM_I_OVERRUN + 1     # row = scenario_id
QS_SUMM_I_COUNT = QS_SUMM_I_START_EPISODES + 1
# ---- include/quadswarm_exchange.h ----
QS_XCHG_HANDLE_BYTES = 64
QS_XCHG_EXPORT_BYTES = 2 * QS_XCHG_HANDLE_BYTES + 16
QS_WIRE_F32, QS_WIRE_BF16, QS_WIRE_Q8 = 0, 1, 2
# ---- include/quadswarm_encoder.h ----
QS_ENC_NBR_MEAN_EMBED, QS_ENC_NBR_ATTENTION, QS_ENC_NBR_MLP, QS_ENC_NBR_NONE, QS_ENC_MODEL_MHA, QS_ENC_MODEL_S2R = range(6)
# ---- include/quadswarm_valuemap.h (quadswarm_encoder.h includes it) ----
QS_VMAP_MAX_GRID = 64
QS_VMAP_MAX_SHIFTS = 64
QS_VMAP_MAX_OBS_DIM = 4096

i32, i64, u32, f32, f64, vp = C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_double, C.c_void_p


class QsConfig(C.Structure):
    """qs_config (include/quadswarm.h)"""
    _fields_ = [
        ("num_envs", i32), ("num_agents", i32), ("env_id_offset", i32), ("precision", i32), ("seed", C.c_uint64),
        ("mass", f64), ("inertia", f64 * 3), ("arm", f64), ("prop_cross", (f64 * 3) * 4), ("prop_ccw", f64 * 4),
        ("thrust_max", f64 * 4), ("torque_max", f64 * 4), ("motor_tau_up", f64), ("motor_tau_down", f64),
        ("motor_linearity", f64), ("vel_damp", f64), ("damp_omega_quadratic", f64), ("omega_max", f64), ("gravity", f64),
        ("thrust_noise_sigma", f64), ("ou_theta", f64),
        ("dt", f64), ("sim_steps", i32), ("ep_len", i32), ("room_lo", f64 * 3), ("room_hi", f64 * 3), ("floor_mode", i32), ("svd_period", i32),
        ("sense_noise", i32), ("obs_repr", i32),
        ("pos_norm_std", f64), ("pos_unif_range", f64), ("vel_norm_std", f64), ("vel_unif_range", f64), ("quat_norm_std", f64),
        ("quat_unif_range", f64), ("gyro_noise_density", f64),
        ("num_neighbors", i32), ("use_downwash", i32), ("use_obstacles", i32), ("scenario", i32),
        ("collision_threshold", f64), ("collision_falloff_threshold", f64), ("rew_coeff", f64 * QS_REW_COUNT),
        ("spawn_box", f64), ("approach_goal_metric", f64), ("nbr_clip_pos", f64 * 3), ("nbr_clip_vel", f64 * 3),
        ("obst_size", f64), ("obst_density", f64), ("obst_area", i32 * 2), ("num_obstacles", i32),
        ("write_rew_info", i32), ("episode_sums", i32),
        ("dr_num_density", i32), ("dr_num_size", i32), ("dr_obst_count", i32 * QS_MAX_DR_CHOICES),
        ("dr_density", f64 * QS_MAX_DR_CHOICES), ("dr_size", f64 * QS_MAX_DR_CHOICES)]


class QsBuffers(C.Structure):
    """qs_buffers (include/quadswarm.h): the device pointers native.Stepper turns into views"""
    _fields_ = [(name, vp) for name in (
        "obs", "reward", "done", "rew_info", "actions", "pos", "vel", "omega", "rot", "thrust_rot_damp",
        "thrust_cmds_damp", "ou_state", "goal", "flags", "obst_hit_idx", "col_pair_mask", "new_pair_mask",
        "unique_col_mask", "obst_new_mask", "room_new_mask", "counters", "tick", "obst_pos", "ep_stats",
        "ep_counters", "error_flag", "scenario_id", "ep_scenario", "run_sums", "ep_sums", "obst_count", "obst_size_env", "obst_density_env")] + [
        ("obs_dim", i32), ("real_size", i32), ("state_block_bytes", i32), ("envs_per_block", i32), ("state_lane_major", i32)]


class GateInfo(C.Structure):
    """qs_gate_info_t (include/quadswarm.h): the action ring and the sequence words of resident-state stepping"""
    _fields_ = [("action_ring", vp), ("action_stride_bytes", i64), ("ring_len", i32),
                ("groups", i32), ("wg_per_group", i32), ("workgroups", i32), ("envs_per_workgroup", i32),
                ("act_flag", vp), ("done_flag", vp), ("steps_launched", i64), ("steps_fed", i64)]


class PilotParams(C.Structure):
    """qs_pilot_params (include/quadswarm_control.h): gains, gravity, desired heading and inverse Jacobian of the position controller"""
    _fields_ = [(n, f64) for n in ("kp_p", "kd_p", "kp_a", "kd_a", "yaw_gain", "max_pos_err", "gravity")] + [
        ("x_des", f64 * 3), ("jinv", (f64 * 4) * 4)]


class WireQ8(C.Structure):
    """qs_wire_q8 (include/quadswarm_exchange.h): the 8-bit fixed-point block [q0, q1) of an observation row and its clip ranges"""
    _fields_ = [("q0", i32), ("q1", i32), ("clip", f32 * 6)]


class EncLayer(C.Structure):
    """qs_enc_layer (include/quadswarm_encoder.h): packed weights, padded bias"""
    _fields_ = [("w", vp), ("b", vp), ("M", i32), ("K", i32)]


class EncParams(C.Structure):
    """qs_enc_params (include/quadswarm_encoder.h)"""
    _fields_ = [("self_dim", i32), ("nbr_dim", i32), ("num_nbr", i32), ("obst_dim", i32), ("obs_dim", i32), ("nbr_encoder", i32),
                ("s1", EncLayer), ("s2", EncLayer), ("n1", EncLayer), ("n2", EncLayer), ("n3", EncLayer), ("o1", EncLayer), ("o2", EncLayer),
                ("v1", EncLayer), ("v2", EncLayer), ("a1e", EncLayer), ("a1m", EncLayer), ("a2", EncLayer), ("a3w", vp), ("a3b", f32), ("precision", i32),
                ("ebuf", vp), ("gbuf", vp), ("f", EncLayer),
                ("mq", EncLayer), ("mk", EncLayer), ("mv", EncLayer), ("mfc", EncLayer), ("ln_w", vp), ("ln_b", vp),
                ("head_w", vp), ("head_b", vp), ("head_out", vp), ("head_dim", i32),
                ("sample_step", u32), ("sample_log_std", vp), ("act_out", vp), ("sample_counter", vp), ("sample_seed_lo", u32), ("sample_seed_hi", u32),
                ("traj_rew_src", vp), ("traj_rew_dst", vp), ("traj_done_src", vp), ("traj_done_dst", vp)]


class RolloutTargetsParams(C.Structure):
    """qs_rollout_targets_params (include/quadswarm_encoder.h): a recorded segment -> log-probabilities, GAE advantages, returns"""
    _fields_ = [("T", i32), ("A", i32), ("rewards", vp), ("dones", vp), ("values", vp), ("means", vp), ("actions", vp), ("log_std", vp),
                ("act_dim", i32), ("gamma", f32), ("gae_lambda", f32), ("reward_scale", f32), ("reward_clip", f32),
                ("logp", vp), ("advantages", vp), ("returns", vp)]


class ValueMapParams(C.Structure):
    """qs_value_map_params (include/quadswarm_valuemap.h): observation rows -> rows over an offset grid -> critic values -> per-agent extrema"""
    _fields_ = [("A", i32), ("obs_dim", i32), ("nx", i32), ("ny", i32), ("obs", vp),
                ("off_x", f32 * QS_VMAP_MAX_GRID), ("off_y", f32 * QS_VMAP_MAX_GRID),
                ("n_shifts", i32), ("shift_col", i32 * QS_VMAP_MAX_SHIFTS), ("shift_axis", i32 * QS_VMAP_MAX_SHIFTS), ("shift_sign", i32 * QS_VMAP_MAX_SHIFTS),
                ("rows", vp), ("cap_rows", i32), ("values", vp), ("vmax", vp), ("vmin", vp), ("argmax", vp)]


# ---- prototypes: (name, restype, argtypes), one table per header, every function the header declares ----
cint, size_t, cstr, u8p, i32p, i64p, f64p = C.c_int, C.c_size_t, C.c_char_p, C.POINTER(C.c_uint8), C.POINTER(i32), C.POINTER(i64), C.POINTER(f64)
cfgp, q8p, pilotp, encp = C.POINTER(QsConfig), C.POINTER(WireQ8), C.POINTER(PilotParams), C.POINTER(EncParams)
vmapp = C.POINTER(ValueMapParams)

QUADSWARM_H = [
    ("qs_version", cint, []), ("qs_sizeof_config", size_t, []), ("qs_last_error", cstr, []),
    ("qs_default_config", cint, [cfgp, i32, i32]), ("qs_obs_dim", cint, [cfgp]),
    ("qs_create", cint, [cfgp, cint, C.POINTER(vp)]), ("qs_destroy", cint, [vp]),
    ("qs_reset", cint, [vp, u8p, vp]), ("qs_step", cint, [vp, vp, vp]), ("qs_step_many", cint, [vp, vp, i32, vp]),
    ("qs_gate_create", cint, [vp, i32, i32]), ("qs_gate_info", cint, [vp, C.POINTER(GateInfo)]),
    ("qs_step_gated", cint, [vp, i32, vp]), ("qs_gate_wait", cint, [vp, vp]),
    ("qs_gate_produce", cint, [vp, vp, i32, i32, i32, vp]), ("qs_gate_produce_verify", cint, [vp, vp, i32, i32, vp, vp]),
    ("qs_gate_status", cint, [vp, i64p]),
    ("qs_sync", cint, [vp, vp]), ("qs_get_buffers", cint, [vp, C.POINTER(QsBuffers)]),
    ("qs_set_obs_target", cint, [vp, vp]), ("qs_set_obs_exchange", cint, [vp, vp, i32]),
    ("qs_set_reward_coeffs", cint, [vp, f64p]), ("qs_get_state", cint, [vp, i32, f64p, i32p]), ("qs_set_state", cint, [vp, i32, f64p, i32]),
    ("qs_memcpy_d2h", cint, [vp, vp, vp, size_t]), ("qs_memcpy_h2d", cint, [vp, vp, vp, size_t]),
    ("qs_state_array_copy", cint, [vp, vp, vp, i32, i32, i32]), ("qs_check_errors", cint, [vp]),
    ("qs_set_profiling", cint, [vp, i32]), ("qs_get_kernel_time", cint, [vp, f64p, i64p]),
    ("qs_set_noise_tape", cint, [vp, f64p, i64]), ("qs_get_tape_pos", cint, [vp, i32p]), ("qs_set_tape_pos", cint, [vp, i32p]),
    ("qs_snapshot_pool", cint, [vp, i32]), ("qs_snapshot_save", cint, [vp, i32, i32, vp]), ("qs_snapshot_load", cint, [vp, i32, i32, vp]),
    ("qs_snapshot_copy", cint, [vp, i32, i32, vp]),
    ("qs_replay_enable", cint, [vp, f64]), ("qs_replay_stats", cint, [vp, i32p]), ("qs_replay_set_active", cint, [vp, u8p]),
    ("qs_spec_build", cint, [cfgp, cint, cstr, cint]), ("qs_spec_verify", cint, [cstr, cstr, cint]), ("qs_spec_repair", cint, [cstr, cstr, cint]),
    ("qs_is_specialized", cint, [vp]), ("qs_spec_status", cint, [vp, cstr, cint]), ("qs_kernel_flavor", cint, [vp])]

QUADSWARM_EXCHANGE_H = [
    ("qs_wire_row_bytes", i64, [i32, cint, q8p]), ("qs_xchg_set_fenced", cint, [vp, cint]), ("qs_xchg_get_fenced", cint, [vp]),
    ("qs_xchg_create", cint, [cint, cint, cint, i64, i32, cint, C.POINTER(vp)]),
    ("qs_xchg_create_q8", cint, [cint, cint, cint, i64, i32, q8p, C.POINTER(vp)]), ("qs_xchg_destroy", cint, [vp]),
    ("qs_xchg_export", cint, [vp, vp]), ("qs_xchg_attach", cint, [vp, vp]), ("qs_xchg_attach_local", cint, [vp, cint, vp]),
    ("qs_xchg_staging", vp, [vp, cint]), ("qs_xchg_gathered", vp, [vp, cint]),
    ("qs_xchg_push", cint, [vp, vp, vp]), ("qs_xchg_wait", cint, [vp, vp]), ("qs_xchg_release", cint, [vp, vp]), ("qs_xchg_wait_release", cint, [vp, vp]),
    ("qs_xchg_fused_desc", vp, [vp, i32, i32, i64p]), ("qs_xchg_status", cint, [vp, i64p]),
    ("qs_obs_pack", cint, [vp, vp, i64, cint, vp]), ("qs_obs_pack_rows", cint, [vp, vp, i64, i32, cint, q8p, vp]),
    ("qs_obs_unpack_rows", cint, [vp, vp, i64, i32, cint, q8p, vp]), ("qs_xchg_last_error", cstr, [])]

QUADSWARM_CONTROL_H = [
    ("qs_pilot_default_params", cint, [cfgp, pilotp]), ("qs_pilot_set_params", cint, [vp, pilotp]), ("qs_pilot_actions", cint, [vp, vp, vp, vp, i32, vp])]

QUADSWARM_SUMMARY_H = [
    ("qs_episode_summary_enable", cint, [vp]), ("qs_episode_summary_accumulate", cint, [vp, vp, i32, vp]),
    ("qs_episode_summary_read", cint, [vp, f64p, i64p, i32, vp])]

# include/quadswarm_neighbors.h (quadswarm_control.h includes it): no struct and no constant of its own
QUADSWARM_NEIGHBORS_H = [
    ("qs_neighbor_ids", cint, [vp, vp, vp, vp]), ("qs_neighbor_scatter", cint, [vp, vp, i32, i32, i32, vp, vp])]

QUADSWARM_ENCODER_H = [
    ("qs_enc_sizeof_params", size_t, []), ("qs_enc_lds_bytes", size_t, []), ("qs_enc_lds_bytes_of", size_t, [i32]), ("qs_enc_lds_bytes_split", size_t, [i32]),
    ("qs_enc_last_error", cstr, []), ("qs_enc_forward", cint, [vp, i32, encp, vp, vp]),
    ("qs_enc_set_wide_min", i32, [i32]), ("qs_enc_set_pingpong", i32, [i32]),
    ("qs_rollout_pre", cint, [vp, vp, i32, vp, vp, vp, i32, C.c_uint64, vp, vp]), ("qs_rollout_post", cint, [vp, vp, vp, vp, i32, vp, vp]),
    ("qs_rollout_sizeof_targets", size_t, []), ("qs_rollout_targets", cint, [C.POINTER(RolloutTargetsParams), vp]),
    ("qs_enc_benchmark", cint, [vp, i32, encp, vp, vp, i32, f64p])]
QUADSWARM_VALUEMAP_H = [
    ("qs_value_map_sizeof_params", size_t, []), ("qs_value_map_expand", cint, [vmapp, i64, i32, vp]), ("qs_value_map_reduce", cint, [vmapp, vp]),
    ("qs_value_map", cint, [vmapp, encp, vp])]
# include/quadswarm_attention.h (quadswarm_encoder.h includes it): no struct and no constant of its own
QUADSWARM_ATTENTION_H = [("qs_attn_row_elems", i32, [encp]), ("qs_attn_weights", cint, [vp, i32, encp, vp, vp])]
# exported by libquadswarm_encoder.so and bound by policy.lib(), declared by NO header: the bench-only switch of the targets scan
ENCODER_UNDECLARED = [("qs_rollout_set_targets_chunks", i32, [i32])]


def names(table):
    return [row[0] for row in table]


def bind(cdll, table):
    """give every function of `table` its prototype on the loaded library `cdll`"""
    for name, restype, argtypes in table:
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes

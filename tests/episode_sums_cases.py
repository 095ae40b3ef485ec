"""The inputs of the episode-sums tests, shared by tests/test_episode_sums_model_cpu.py (which checks on the oracle alone that they are
hard enough: every row moves, episodes end, actions leave [-1, 1], done flags differ inside a workgroup, every listed wrong model is
outside the bound) and tests/test_episode_sums_gpu.py (which runs the step kernels over them).  No GPU needed to import."""
import numpy as np

from tests import test_hip_parity as thp
from tests.episode_sums_model import EpisodeSums

# name -> (parity case, overrides, E): the smallest shapes at which the kernel paths differ
CASES = {
    "c2_n8_dw": ("c2_n8_dw", dict(ep_time=0.25), 11),             # N <= 8 team path: 8 environments per workgroup, the second holds 3
    "c3_n8_obst_short": ("c3_n8_obst_short", dict(ep_time=0.35), 3),   # obstacles: all 17 term rows move
    "c1_single": ("c1_single", dict(ep_time=0.1), 70),            # N = 1: 64 environments per workgroup, the second holds 6
    "e_n33_k8": ("e_n33_k8", dict(ep_time=0.1), 3),               # N > 8 team path, 31 idle lanes
    "e_n64_k6": ("e_n64_k6", dict(ep_time=0.1), 2),               # a full wave per environment
    "s_mix": ("s_mix", dict(), 5),                                # the `_full` scenario instantiations
}
STEPS = {name: 60 for name in CASES}
STEPS["c3_n8_obst_short"] = 75                                   # 36-step episodes: two of them
SUMS_KW = dict(episode_sums=True, write_rew_info=False)           # the production combination
RESETS = {7: (1, 4, 9), 31: (0, 9)}                               # staggered case: explicit resets in mid-episode (step -> environments)
COEFF_STEP = 12                                                   # annealing case: the step before which the coefficients change
NEW_COEFFS = dict(thp.REW, quadcol_bin=2.5, quadcol_bin_smooth_max=6.0, pos=0.8, effort=0.1, spin=0.2, crash=1.5, orient=0.6, quadcol_bin_obst=3.0)
MANY_K, MANY_LAUNCHES = 7, 9                                      # qs_step_many: steps per launch, launches
MANY_EVENT_T = {1: 6, 2: 14, 3: 22, 4: 30, 5: 31, 6: 15, 7: 16}   # launch -> the crafted state of force_events applied in front of it
RING_LEN = 8
# plain one-launch steps in front of the first multi-step launch: puts the end of s_mix's first 13-step episode on a launch's LAST step
MANY_LEAD = {"s_mix": 6}
# a float32 step that starts from the device's own state, not from a forced one: the free-running envelope the parity suite asserts before
# step 60, in units of the per-step bound (tests/test_fp32_parity_gpu.py, DRIFT[0] = 3; measured there: 2.0)
FREE_STEP_SCALE = 3.0


def many_steps(name):
    return MANY_LEAD.get(name, 0) + MANY_K * MANY_LAUNCHES


def many_event_t(name):
    """qs_step_many: states can only be forced between launches"""
    lead = MANY_LEAD.get(name, 0)
    return lambda t: MANY_EVENT_T.get((t - lead) // MANY_K) if t >= lead and (t - lead) % MANY_K == 0 else None


def config_of(name, precision="f64", E=None, seed=1234, env_id_offset=3, **over):
    from quad_swarm_rl_amd import config as qcfg
    case, case_over, case_E = CASES[name]
    kw = dict(thp.CASES[case], **dict(case_over, **dict(SUMS_KW, **over)))
    return qcfg.make_config(num_envs=E or case_E, seed=seed, env_id_offset=env_id_offset, precision=precision, **kw)


def coeff_vector(coeffs):
    from quad_swarm_rl_amd import config as qcfg
    full = dict(qcfg.REW_COEFF_DEFAULT, **coeffs)
    return [float(full[k]) for k in qcfg.REW_COEFF_KEYS]


def actions(rng, t, E, N, gentle_only=False):
    """The parity suite's schedule (ten wild steps, ten gentle ones) with the wild ones drawn from [-1.3, 1.3]: the sums take the RAW
    actions, the dynamics clip them.  float32-representable, so that every precision is given the same numbers."""
    gentle = gentle_only or (t // 10) % 2 == 1
    a = 0.06 + rng.uniform(-0.05, 0.05, size=(E, N, 4)) if gentle else rng.uniform(-1.3, 1.3, size=(E, N, 4))
    return a.astype(np.float32).astype(np.float64)


class NoDevice:
    """what oracle_rollout() tells a device twin; here: nobody"""
    teacher_forced = False

    def set_state(self, e, s, tick):
        pass

    def reset(self, mask):
        pass

    def set_reward_coeffs(self, vec):
        pass

    def note_lift(self, t, e, drones):
        pass


def make_scouts(cfg, oenvs):
    """one more oracle environment per environment, on the same draw counter: as many resets as the environment has had (no steps yet)"""
    from oracle import oracle as orc
    scouts = []
    for e, o in enumerate(oenvs):
        sc = orc.OracleEnv(cfg, env_global_id=cfg.env_id_offset + e)
        for _ in range(o.info().num_resets):
            sc.reset()
        scouts.append(sc)
    return scouts


def oracle_rollout(cfg, oenvs, steps, device=None, resets=None, coeff_step=None, event_t=None, seed=5, gentle_only=False, events=True, force_every=1):
    """Generator over `steps` control steps of the oracle environments `oenvs` with the crafted events of the parity suite
    (thp.force_events, obstacle positions from the oracle).  Yields ("reset", t, mask, model) after an explicit reset and
    ("step", t, actions [E, N, 4], done [E, N], rew_info [E, N, 17], model) after each step; `model` is the EpisodeSums fed with the oracle's
    reward terms and done flags.  `device` (NoDevice protocol) is told every state change, reset and coefficient update BEFORE the
    oracle steps, and - teacher_forced - is given the oracle's state in front of every force_every-th step (with the float32 margins of
    thp.float32_margins, and the floor margin applied one step earlier through a scout environment, below); the steps in between start
    from the device's own state and count FREE_STEP_SCALE times in the model's bound.  event_t: step -> the `t` handed to force_events
    (None: the step itself)."""
    device = device or NoDevice()
    E, N = len(oenvs), cfg.num_agents
    model = EpisodeSums(E, N)
    rng = np.random.RandomState(seed)
    thr = cfg.arm if cfg.floor_mode == 0 else 0.05
    M = cfg.num_obstacles
    scouts = make_scouts(cfg, oenvs) if device.teacher_forced else None
    for t in range(steps):
        if resets and t in resets:
            mask = np.zeros(E, dtype=np.uint8)
            mask[list(resets[t])] = 1
            for e in np.nonzero(mask)[0]:
                oenvs[e].reset()
                if scouts:
                    scouts[e].reset()
            device.reset(mask)
            model.reset(mask)
            yield ("reset", t, mask, model)
        if coeff_step is not None and t == coeff_step:
            vec = coeff_vector(NEW_COEFFS)
            for o in oenvs:
                o.set_reward_coeffs(vec)
            device.set_reward_coeffs(vec)
        te = t if event_t is None else event_t(t)
        forced = device.teacher_forced and t % force_every == 0
        act = actions(rng, t, E, N, gentle_only)
        for e, o in enumerate(oenvs):
            s, tick = o.get_state()
            changed = False
            if events and te is not None:
                oxy = np.array(o.info().obst_pos)[:M] if cfg.use_obstacles else None
                changed = thp.force_events(te, e, s, N, oxy, cfg.obst_size / 2)
            if forced:
                changed = thp.float32_margins(cfg, s) or changed
            if scouts:
                # The same floor margin one step earlier: a drone at REST on the floor that this step lifts by less than 1e-6 m (measured on the
                # full-length episode: 1.1e-9 and 5.2e-10 m; ulp(0.046) = 3.7e-9 in float32) leaves the floor in float64 and stays on it in
                # float32 - every term that depends on the floor flag then differs for this one step.  The scout (same Philox stream, same
                # state) takes the step first; such a drone starts a forced step from the representable margin, in BOTH states.
                scouts[e].set_state(s, tick)
                scouts[e].step(act[e])
                s1, _ = scouts[e].get_state()
                lift = (s[:, 30] != 0) & (s1[:, 30] == 0) & (s1[:, 2] - thr > 0) & (s1[:, 2] - thr < 1e-6)
                if forced and lift.any():
                    s[lift, 2], s[lift, 30] = thr + 1e-4, 0.0
                    changed = True
                    device.note_lift(t, e, np.nonzero(lift)[0].tolist())
            if changed:
                o.set_state(s, tick)
            if changed or forced:
                device.set_state(e, s, tick)
        out = [o.step(act[e]) for e, o in enumerate(oenvs)]
        done, ri = np.stack([x[2] for x in out]), np.stack([x[3] for x in out])
        model.step(act, ri, done, tol_scale=FREE_STEP_SCALE if device.teacher_forced and not forced else 1.0)
        yield ("step", t, act, done, ri, model)


def make_oracles(cfg, E=None):
    from oracle import oracle as orc
    oenvs = [orc.OracleEnv(cfg, env_global_id=cfg.env_id_offset + e) for e in range(E or cfg.num_envs)]
    for o in oenvs:
        o.reset()
    return oenvs

"""The device-side batched experience replay (qs_replay_enable: qs_replay_kernel behind every step) against its Python twin
tests/replay_model.py - which tests/test_replay_model_vs_reference.py pins against the REFERENCE wrapper's recorded behaviour.

test_replay_kernel_equals_the_model: 24 environments with different collision histories run for ~4500 control steps at 100 Hz: natural
activation of the replay buffers (10 episodes with a mean crash reward above -1), checkpoints every 0.5 s, collisions filed once per 5 s
from the checkpoint of 1.5 s ago, episodes restarted from events with probability 0.75.  After every step the kernel's
per-environment state must equal the model's (same Philox draws), the observation returned on a filing step must be the filed
checkpoint's, and a restored environment must equal the checkpoint bit for bit.

The tests below it run at 10 Hz control (sim_steps = 20: a checkpoint every 5 ticks, 15 ticks of grace, 50 ticks between the events of
an episode), which brings the branches of the kernel that the 100 Hz run never reaches within a few hundred steps: the wrapped
checkpoint ring, the full event buffer, the cleanup after ten replays, the obstacle trigger, the IndexError path - and compare the
restore array by array on every state layout.  Every comparison is integer or bit equality; the model is fed the device's own
collision masks, so the physics need not follow a script."""
import ctypes as C

import numpy as np
import pytest

from tests.replay_model import EVENTS, RING, ReplayModel

pytestmark = pytest.mark.gpu
SITE_REPLAY = 25
STAT_KEYS = ("episodes", "replayed", "buffer_len", "replayed_sum", "active", "checkpoints", "errors")
TEN_HZ = dict(sim_freq=200.0, sim_steps=20, episode_sums=True, write_rew_info=False)
ZEROED_COUNTERS = (0, 1, 7, 8)    # collisions, collisions_after_settle, obst, obst_after_settle (config.COUNTER_KEYS)


def philox_u(seed, env, ctr, slot):
    """u01 of word 0 of the Philox group the kernel draws: counter = {env, step_ctr, site | slot << 8, 0}"""
    from oracle import oracle as orc
    c = (C.c_uint32 * 4)(env, ctr, SITE_REPLAY | (slot << 8), 0)
    k = (C.c_uint32 * 2)(seed & 0xffffffff, seed >> 32)
    out = (C.c_uint32 * 4)()
    orc.lib().qso_philox4x32(c, k, out)
    return np.float32((np.float32(out[0] >> 9) + np.float32(0.5)) * np.float32(1.0 / 8388608.0))


def test_replay_kernel_equals_the_model():
    from quad_swarm_rl_amd import config as qcfg, native
    E, N, seed, prob = 24, 4, 5, 0.75
    cfg = qcfg.make_config(num_envs=E, num_agents=N, neighbor_visible_num=2, neighbor_obs_type="pos_vel", use_numba=True, ep_time=2.6, seed=seed,
                           env_id_offset=7, precision="f64", episode_sums=True, write_rew_info=False)
    st = native.Stepper(cfg, device=0)
    assert native.lib().qs_replay_enable(st._h, 2.0) != 0            # sample_prob outside [0, 1]
    st.replay_enable(prob)
    with pytest.raises(native.QsError):
        st.replay_enable(prob)                                       # once per handle
    st.reset()
    forced = np.array([e % 2 for e in range(E)], dtype=np.uint8)      # half of the buffers switched on by hand, the others by the rule
    st.replay_set_active(forced)
    models = [ReplayModel(prob, control_freq=100, use_obstacles=False, active=bool(forced[e])) for e in range(E)]
    D, T = st.obs_dim, E * N
    rng = np.random.RandomState(1)
    snaps = [dict() for _ in range(E)]                                # per env: pool slot -> (pos, vel, rot, tick, obs) of the snapshot
    ticks = np.zeros(E, dtype=np.int64)
    n_file = n_restore = n_save = 0
    steps = 4600
    for step in range(1, steps + 1):
        # a collision (two drones 3 cm apart) at tick 170 in a third of the envs, in episodes that are not replays
        for e in np.nonzero(ticks == 169)[0]:
            if e % 3 == 0 and not models[e].saved:
                s, tk = st.get_state(int(e))
                s[1, 0:3] = s[0, 0:3] + np.array([0.03, 0.0, 0.0]); s[1, 3:6] = s[0, 3:6]
                st.set_state(int(e), s, tk)
        act = 0.06 + rng.uniform(-0.02, 0.02, size=(T, 4))           # hovering: the drones stay in the air, crash rewards stay at zero
        st.from_host("actions", act)
        st.step()
        st.sync()
        done = st.to_host("done").reshape(E, N)[:, 0].astype(bool)
        ticks = st.to_host("tick").astype(np.int64)
        uq = st.to_host("unique_col_mask")
        ctr = 1 + step                                                # qs_reset took counter 1, step k takes 1 + k
        need_state = False
        acts = []
        crash = st.to_host("ep_sums")[3].reshape(E, N)[:, 0] if done.any() else None
        for e in range(E):
            a = models[e].step(bool(done[e]), int(ticks[e]), int(uq[e]), 0, float(crash[e]) if done[e] else 0.0,
                               lambda: philox_u(seed, 7 + e, ctr, 0),
                               lambda n: min(int(np.float32(philox_u(seed, 7 + e, ctr, 1)) * np.float32(n)), n - 1))
            a = [x for x in a if x[0] != "fresh"]
            acts.append(a)
            need_state |= bool(a)
        rs = st.replay_stats()
        for e in range(E):
            ms = models[e].stats()
            for k in ("episodes", "replayed", "buffer_len", "replayed_sum", "active", "checkpoints", "errors"):
                assert rs[k][e] == ms[k], (step, e, k, rs[k][e], ms[k])
        if need_state:
            pos, vel, rot = st.to_host("pos").reshape(3, E, N), st.to_host("vel").reshape(3, E, N), st.to_host("rot").reshape(9, E, N)
            obs = st.to_host("obs").reshape(E, N, D)
            for e, a in enumerate(acts):
                both = len(a) == 2     # a checkpoint saved AND an event filed on this step: the live observation was overwritten after the save
                for x in a:
                    if x[0] == "save":
                        snaps[e][x[1]] = (pos[:, e].copy(), vel[:, e].copy(), rot[:, e].copy(), int(ticks[e]), None if both else obs[e].copy())
                        n_save += 1
                    elif x[0] == "file":
                        snaps[e][x[2]] = snaps[e][x[1]]
                        if snaps[e][x[1]][4] is not None:
                            np.testing.assert_array_equal(obs[e], snaps[e][x[1]][4])  # the 1.5-s-old observation is returned on this step
                        assert ticks[e] - snaps[e][x[1]][3] >= 100
                        n_file += 1
                    else:
                        p0, v0, r0, t0, o0 = snaps[e][x[1]]
                        np.testing.assert_array_equal(pos[:, e], p0); np.testing.assert_array_equal(vel[:, e], v0)
                        np.testing.assert_array_equal(rot[:, e], r0)
                        if o0 is not None:
                            np.testing.assert_array_equal(obs[e], o0)
                        assert ticks[e] == t0 and rs["ep_steps"][e] >= 1
                        n_restore += 1
            cnt = st.to_host("counters")
            for e, a in enumerate(acts):
                if a and a[-1][0] == "restore":
                    assert cnt[0, e] == 0 and cnt[1, e] == 0                          # collision counters zeroed on the replayed env
    st.check_errors()
    assert all(m.active for m in models)                              # the rule switched the other half on after 10 clean episodes
    assert n_save > 500 and n_file >= 8 and n_restore >= 6, (n_save, n_file, n_restore)
    st.close()


def test_explicit_reset_feeds_the_crash_history():
    """qs_reset while the replay wrapper runs: every explicit reset of an environment records the running episode's crash reward, like
    the reference's reset() does (quadrotor_multi.py:356-359) - ten recorded episodes with a mean above -1 switch the buffer on.  The
    masked-out environments are untouched, and the action statistics of the next finished episode count its steps from tick 0."""
    from quad_swarm_rl_amd import config as qcfg, native
    E, N = 6, 4
    cfg = qcfg.make_config(num_envs=E, num_agents=N, neighbor_visible_num=2, neighbor_obs_type="pos_vel", use_numba=True, ep_time=0.5, seed=3,
                           precision="f32", episode_sums=True, write_rew_info=False)
    st = native.Stepper(cfg, device=0)
    st.replay_enable(0.5)
    st.reset()
    models = [ReplayModel(0.5, control_freq=100) for _ in range(E)]
    act = np.full((E * N, 4), 0.06, dtype=np.float32)
    mask = np.array([1, 0, 1, 1, 0, 0], dtype=np.uint8)
    for rnd in range(9):                                # 1 (first reset) + 9 explicit resets = 10 entries => active
        for _ in range(5):
            st.from_host("actions", act)
            st.step()
        st.sync()
        crash = st.to_host("run_sums")[3].reshape(E, N)[:, 0]
        assert not st.to_host("done").any()
        st.reset(mask)
        for e in np.nonzero(mask)[0]:
            models[e].explicit_reset(float(crash[e]))
        rs = st.replay_stats()
        assert rs["active"].tolist() == [int(m.active) for m in models], (rnd, rs["active"].tolist())
        assert (st.to_host("tick")[mask == 1] == 0).all() and (st.to_host("tick")[mask == 0] == 5 * (rnd + 1)).all()
    assert rs["active"].tolist() == [1, 0, 1, 1, 0, 0]
    # the reset environments finish their next episode after ep_len + 1 steps, counted from the reset
    for _ in range(cfg.ep_len + 1):
        st.from_host("actions", act)
        st.step()
    st.sync()
    rs = st.replay_stats()
    done = st.to_host("done").reshape(E, N)[:, 0]
    assert done[mask == 1].all() and (rs["ep_steps"][mask == 1] == cfg.ep_len + 1).all()
    st.close()


def test_domain_random_through_the_batched_env():
    """--quads_domain_random with the replay wrapper (quad_experience_replay.py:75-88,:106-118,:191-206): every new episode of every
    environment draws its obstacle density and size; the wrapper's statistics report them."""
    import argparse
    import torch
    from quad_swarm_rl_amd import sf_env
    p = argparse.ArgumentParser()
    p.add_argument("--with_pbt", default=False)
    sf_env.add_quadrotors_env_args("quadrotor_multi", p)
    cfg = p.parse_args(["--quads_num_agents=8", "--quads_neighbor_visible_num=2", "--quads_neighbor_obs_type=pos_vel", "--quads_use_numba=True",
                        "--quads_use_obstacles=True", "--quads_obstacle_obs_type=octomap", "--quads_obst_spawn_area", "8", "8", "--quads_obst_size=0.6",
                        "--quads_mode=o_random", "--quads_obs_repr=xyz_vxyz_R_omega_floor", "--quads_episode_duration=0.3", "--quads_num_envs=32",
                        "--replay_buffer_sample_prob=0.5", "--quads_domain_random=True", "--quads_obst_density_random=True", "--quads_obst_size_random=True",
                        "--quads_obst_density_min=0.05", "--quads_obst_density_max=0.2", "--quads_obst_size_min=0.3", "--quads_obst_size_max=0.6"])
    env = sf_env.make_quadrotor_env("quadrotor_multi", cfg=cfg)
    assert env.vec.cfg.dr_num_density == 4 and env.vec.cfg.dr_num_size == 3 and env.vec.cfg.num_obstacles == 12
    env.reset()
    seen_d, seen_s = set(), set()
    act = torch.full((env.num_agents, 4), 0.06, device="cuda")
    for t in range(100):
        obs, rew, term, trunc, infos = env.step(act)
        if term.any():
            for inf in infos:
                seen_d.add(round(inf["episode_extra_stats"]["replay/obst_density"], 6))
                seen_s.add(round(inf["episode_extra_stats"]["replay/obst_size"], 6))
    assert seen_d == {0.05, 0.1, 0.15, 0.2} and seen_s == {0.3, 0.4, 0.5}
    cnt = env.vec.stepper.to_host("obst_count")
    assert set(cnt.tolist()) <= {3, 6, 9, 12} and len(set(cnt.tolist())) > 1
    assert torch.isfinite(obs["obs"]).all()
    env.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 10 Hz control: the kernel's remaining branches against the model, the restore array by array
# ---------------------------------------------------------------------------------------------------------------------------------
# every array of one environment that Stepper exposes and the snapshot list (alloc_buffers) holds
EXPOSED = ("pos", "vel", "rot", "omega", "thrust_rot_damp", "thrust_cmds_damp", "ou_state", "goal", "flags", "col_pair_mask", "new_pair_mask",
           "obst_hit_idx", "run_sums", "obs", "unique_col_mask", "counters", "tick", "scenario_id", "obst_pos", "obst_new_mask", "room_new_mask",
           "obst_count", "obst_size_env", "obst_density_env")


def _env_part(st, a, name, e):
    """environment e's part of the host copy `a` of the library buffer `name`"""
    N, E, T = st.N, st.E, st.T
    if name == "obs":
        return a[e * N:(e + 1) * N].copy()
    if name == "obst_pos":
        M = a.shape[1] // E
        return a[:, e * M:(e + 1) * M].copy()
    if a.shape[-1] == T:
        return a[..., e * N:(e + 1) * N].copy()
    return a[..., e:e + 1].copy()


def _grab(st, names):
    return {n: st.to_host(n) for n in names}


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
        bad = np.nonzero((g.view(np.uint8).reshape(g.size, -1) != w.view(np.uint8).reshape(w.size, -1)).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ, first at flat index {int(bad[0])}: {g[bad[0]]!r} != {w[bad[0]]!r}")


def _plant_pair(st, e):
    """drone 1 placed 3 cm from drone 0: the pair collides on the next step"""
    s, tk = st.get_state(int(e))
    s[1, 0:3] = s[0, 0:3] + np.array([0.03, 0.0, 0.0]); s[1, 3:6] = s[0, 3:6]
    st.set_state(int(e), s, tk)


def _plant_obstacle_hit(st, e):
    """drone 0 put on the centre of the environment's first obstacle: it hits that obstacle on the next step"""
    M = max(st.cfg.num_obstacles, 1)
    centre = st.to_host("obst_pos")[:, int(e) * M].astype(np.float64)
    s, tk = st.get_state(int(e))
    s[0, 0:2] = centre; s[0, 3:6] = 0.0
    st.set_state(int(e), s, tk)


class ReplayRun:
    """One handle at 10 Hz control with the replay kernel behind every step and one ReplayModel per environment.  step() feeds the models
    the device's own done flags, ticks and collision masks and the kernel's Philox draws, requires the seven statistics of
    qs_replay_stats to equal the models' and returns what the models decided per environment."""

    def __init__(self, kw, E, prob, active, seed=5, env_id_offset=7, precision="f32"):
        from quad_swarm_rl_amd import config as qcfg, native
        self.cfg = qcfg.make_config(num_envs=E, seed=seed, env_id_offset=env_id_offset, precision=precision, **dict(kw, **TEN_HZ))
        self.st = st = native.Stepper(self.cfg, device=0)
        st.replay_enable(prob)
        st.reset()
        self.active = np.asarray(active, dtype=np.uint8)
        st.replay_set_active(self.active)          # by hand; the crash rule is test_replay_kernel_equals_the_model's
        self.models = [ReplayModel(prob, control_freq=10, use_obstacles=bool(self.cfg.use_obstacles), active=bool(a)) for a in self.active]
        assert (self.models[0].cp_every, self.models[0].grace, self.models[0].min_gap) == (5, 15, 50)
        self.E, self.N, self.seed, self.off, self.steps = E, st.N, seed, env_id_offset, 0
        self.ticks = np.zeros(E, dtype=np.int64)

    def step(self, act):
        st, E, N = self.st, self.E, self.N
        st.from_host("actions", act)
        st.step()
        st.sync()
        self.steps += 1
        ctr = 1 + self.steps                                         # qs_reset took counter 1, step k takes 1 + k
        self.done = done = st.to_host("done").reshape(E, N)[:, 0].astype(bool)
        self.ticks = ticks = st.to_host("tick").astype(np.int64)
        self.uq, self.on = uq, on = st.to_host("unique_col_mask"), st.to_host("obst_new_mask")
        crash = st.to_host("ep_sums")[3].reshape(E, N)[:, 0] if done.any() else None
        self.before = [(len(m.ev_slot), len(m.ck), m.saved) for m in self.models]   # events, checkpoints, replayed episode - before this step
        acts = []
        for e, m in enumerate(self.models):
            a = m.step(bool(done[e]), int(ticks[e]), int(uq[e]), int(on[e]), float(crash[e]) if done[e] else 0.0,
                       lambda: philox_u(self.seed, self.off + e, ctr, 0),
                       lambda n: min(int(np.float32(philox_u(self.seed, self.off + e, ctr, 1)) * np.float32(n)), n - 1))
            acts.append([x for x in a if x[0] != "fresh"])
        self.rs = rs = st.replay_stats()
        for e, m in enumerate(self.models):
            ms = m.stats()
            for k in STAT_KEYS:
                assert rs[k][e] == ms[k], (self.steps, e, k, rs[k][e], ms[k])
        return acts


def _follow_actions(run, acts, snaps, names, count):
    """The per-action checks of test_replay_kernel_equals_the_model over the arrays `names`: a filing step returns the filed checkpoint's
    observation, a restored environment equals the host copy made when its checkpoint was saved, bit for bit, with the four collision
    counters zeroed.  snaps: per environment, pool slot -> host copy."""
    if not any(acts):
        return
    st = run.st
    arrs = _grab(st, names + ("counters",))
    for e, a in enumerate(acts):
        both = len(a) == 2     # a checkpoint saved AND an event filed on this step: the live observation was overwritten after the save
        for x in a:
            if x[0] == "save":
                snaps[e][x[1]] = {n: _env_part(st, arrs[n], n, e) for n in names}
                if both:
                    snaps[e][x[1]]["obs"] = None
            elif x[0] == "file":
                snap = snaps[e][x[2]] = snaps[e][x[1]]
                if snap["obs"] is not None:
                    _same_bits(_env_part(st, arrs["obs"], "obs", e), snap["obs"], (run.steps, e, "observation returned on a filing step"))
                assert run.ticks[e] - int(snap["tick"][0]) >= 10
            else:
                snap = snaps[e][x[1]]
                for n in names:
                    if snap[n] is not None:
                        _same_bits(_env_part(st, arrs[n], n, e), snap[n], (run.steps, e, "restored", n))
                assert run.rs["ep_steps"][e] >= 1
                assert all(arrs["counters"][r, e] == 0 for r in ZEROED_COUNTERS), (run.steps, e, arrs["counters"][:, e])
            count[x[0]] += 1


def _c(name):
    from tests.test_hip_parity import CASES
    return CASES[name]


def test_ring_wrap_and_full_buffer_equal_the_model():
    """The C2 shape (8 drones, lane-major state blocks), 80-tick episodes, sample_prob 0.25, two planted pair collisions per fresh
    episode: every environment's 6-slot checkpoint ring wraps (the `dst = head; head = (head + 1) % RING` branch and the
    `(head + cnt - 3) % RING` source behind it), one buffer reaches 20 events and is overwritten at buffer_idx, and on some steps a
    checkpoint is saved and an event filed together (a collision on a tick that is a multiple of 5).  The run goes on until
    episodes were restored from slots that an overwrite had rewritten: only there does an overwrite of the wrong event show."""
    E = 8
    run = ReplayRun(dict(_c("c2_n8_dw"), ep_time=8.0), E, 0.25, np.ones(E))
    st = run.st
    assert st.bufs.state_lane_major == 1 and st.team
    names = ("pos", "vel", "rot", "tick", "obs")
    snaps, count = [dict() for _ in range(E)], dict(save=0, file=0, restore=0)
    wrapped, overwrites, both = np.zeros(E, dtype=bool), np.zeros(E, dtype=np.int64), 0
    overwritten, from_overwritten = [set() for _ in range(E)], 0      # pool slots rewritten by an overwrite; restores from such a slot
    first = [16 + e % 5 for e in range(E)]           # collision ticks 16...20 and 52 later: 20 and 70 are checkpoint ticks
    rng = np.random.RandomState(1)
    for _ in range(9000):
        for e in range(E):
            if not run.models[e].saved and run.ticks[e] + 1 in (first[e], first[e] + 52):
                _plant_pair(st, e)
        acts = run.step(0.06 + rng.uniform(-0.02, 0.02, size=(E * run.N, 4)))
        for e, a in enumerate(acts):
            kinds = [x[0] for x in a]
            wrapped[e] |= "save" in kinds and run.before[e][1] == RING
            both += kinds == ["save", "file"]
            for x in a:
                if x[0] == "file" and run.before[e][0] == EVENTS:
                    overwrites[e] += 1
                    overwritten[e].add(x[2])
                from_overwritten += x[0] == "restore" and x[1] in overwritten[e]
        _follow_actions(run, acts, snaps, names, count)
        if wrapped.all() and overwrites.max() >= 3 and both >= 1 and from_overwritten >= 3:
            break
    st.check_errors()
    print(f"ring wrap / full buffer: {run.steps} steps, {count}; wrapped {wrapped.tolist()}, overwrites of a full buffer {overwrites.tolist()}, "
          f"save and file on one step {both}, restores from an overwritten slot {from_overwritten}, buffer lengths {run.rs['buffer_len'].tolist()}")
    assert wrapped.all() and overwrites.max() >= 3 and both >= 1 and from_overwritten >= 3
    assert (run.rs["errors"] == 0).all()
    st.close()


def test_cleanup_after_ten_replays_equals_the_model():
    """The C3 shape (obstacles, floor representation), sample_prob 1.0: every fresh episode files one event - drone 0 alone put on an
    obstacle centre (the `use_obstacles && obst_new != 0` trigger: ids of drone 0 alone never pass the `.any()` test of the collision
    ids), in every third fresh episode a drone pair instead - which is then replayed until its tenth replay drops it from the buffer
    while buffer_idx keeps counting; the next fresh episode appends to the shrunken buffer.  A restored environment gets the obstacles
    of its checkpoint back, with the four collision counters zeroed."""
    E = 4
    run = ReplayRun(dict(_c("c3_n8_obst"), ep_time=8.0), E, 1.0, np.ones(E), seed=9)
    st = run.st
    assert st.bufs.state_lane_major == 1 and run.cfg.use_obstacles
    names = ("pos", "vel", "rot", "tick", "obs", "obst_pos", "obst_count", "obst_hit_idx", "obst_new_mask")
    snaps, count = [dict() for _ in range(E)], dict(save=0, file=0, restore=0)
    fresh_no, dropped, appended_after = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
    by_obstacle_alone = by_pair = 0
    rng = np.random.RandomState(2)
    for _ in range(3000):
        for e in range(E):
            if not run.models[e].saved and run.ticks[e] == 61:          # filed at tick 62 from the checkpoint of tick 50
                (_plant_pair if fresh_no[e] % 3 == 2 else _plant_obstacle_hit)(st, e)
        acts = run.step(0.06 + rng.uniform(-0.02, 0.02, size=(E * run.N, 4)))
        for e, a in enumerate(acts):
            for x in a:
                if x[0] == "restore":
                    dropped[e] += run.before[e][0] - len(run.models[e].ev_slot)
                elif x[0] == "file":
                    appended_after[e] += dropped[e] > 0
                    by_obstacle_alone += (int(run.uq[e]) & ~1) == 0 and int(run.on[e]) == 1
                    by_pair += (int(run.uq[e]) & ~1) != 0
            fresh_no[e] += bool(run.done[e]) and not a
        _follow_actions(run, acts, snaps, names, count)
        if ((dropped >= 2) & (appended_after >= 2)).any():
            break
    st.check_errors()
    print(f"cleanup: {run.steps} steps, {count}; events dropped after their tenth replay {dropped.tolist()}, appended afterwards "
          f"{appended_after.tolist()}, filed by drone 0's obstacle hit alone {by_obstacle_alone}, by a drone pair {by_pair}")
    assert ((dropped >= 2) & (appended_after >= 2)).any() and by_obstacle_alone >= 2
    assert (run.rs["errors"] == 0).all()
    st.close()


def test_collision_before_three_checkpoints_counts_an_error():
    """A buffer switched on at tick 12 has one checkpoint (tick 15) when a collision comes at tick 17: the reference raises IndexError
    there (quad_experience_replay.py:155-157); the kernel counts an error and files nothing."""
    E = 3
    run = ReplayRun(dict(_c("c2_n8_dw"), ep_time=8.0), E, 0.5, np.zeros(E))
    st = run.st
    filed = 0
    for _ in range(25):
        if run.ticks[0] == 12:
            st.replay_set_active(np.ones(E))
            for m in run.models:
                m.active = True
        if run.ticks[0] == 16:
            _plant_pair(st, 0); _plant_pair(st, 2)
        acts = run.step(np.full((E * run.N, 4), 0.06))
        filed += sum(x[0] == "file" for a in acts for x in a)
        if run.ticks[0] == 17:
            assert (int(run.uq[0]) & ~1) and (int(run.uq[2]) & ~1) and not int(run.uq[1]), run.uq    # the planted collisions happened
    print(f"errors path: errors {run.rs['errors'].tolist()}, checkpoints {run.rs['checkpoints'].tolist()}, events {run.rs['buffer_len'].tolist()}")
    assert run.rs["errors"].tolist() == [1, 0, 1] and run.rs["buffer_len"].tolist() == [0, 0, 0] and filed == 0
    assert run.rs["checkpoints"].tolist() == [3, 3, 3] and run.ticks.tolist() == [25, 25, 25]
    st.check_errors()
    st.close()


NOISE_FREE = dict(ep_time=4.0, sense_noise=None, thrust_noise_ratio=0.0, use_downwash=False)


def _hover_table(ticks, N):
    """actions per tick and drone: a little more than hover thrust, the same for the four motors but for a thousandth of the range - the drones drift
    and tilt a little (position, velocity, rotation and angular velocity all move) and stay away from floor, walls and ceiling, whose
    collision responses draw random numbers"""
    rng = np.random.RandomState(2)
    return 0.08 + rng.uniform(-0.015, 0.015, size=(ticks, N, 1)) + rng.uniform(-0.002, 0.002, size=(ticks, N, 4))


def _layouts():
    from tests.test_hip_parity import REW
    c2, c3, c4 = _c("c2_n8_dw"), _c("c3_n8_obst"), _c("c4_n32_svs")
    n5 = dict(num_agents=5, neighbor_visible_num=-1, neighbor_obs_type="pos_vel", use_downwash=True, use_numba=True, collision_falloff_radius=4.0,
              rew_coeff=REW, quads_mode="dynamic_formations")
    # name: (configuration, environments, precision, QS_TEAM, seed, envs per state block, lane-major)
    return {"c2_team": (c2, 6, "f32", None, 5, 8, 1), "c2_rows": (c2, 6, "f32", "0", 5, 8, 0), "c4_two_envs_per_block": (c4, 4, "f32", None, 12, 2, None),
            "n5_partial_last_block": (n5, 13, "f32", None, 5, 12, None),
            "c3_domain_random": (dict(c3, domain_random=True, obst_density_random=True, obst_size_random=True), 6, "f32", None, 5, 8, 1),
            "c2_lissajous_f64": (dict(c2, quads_mode="ep_lissajous3D"), 6, "f64", None, 3, 8, None)}


LAYOUT_NAMES = ("c2_team", "c2_rows", "c4_two_envs_per_block", "n5_partial_last_block", "c3_domain_random", "c2_lissajous_f64")


def spec_jobs():
    """(make_config keywords, precision, QS_TEAM) of the handles the 10 Hz tests create, for __graft_entry__._spec_jobs: build() compiles
    their config-specialised code objects ahead of time"""
    run = dict(TEN_HZ, env_id_offset=7)
    jobs = [(dict(_c("c2_n8_dw"), ep_time=8.0, num_envs=8, seed=5, **run), "f32"), (dict(_c("c2_n8_dw"), ep_time=8.0, num_envs=3, seed=5, **run), "f32"),
            (dict(_c("c3_n8_obst"), ep_time=8.0, num_envs=4, seed=9, **run), "f32"),
            (dict(_c("c3_n8_obst"), ep_time=4.0, domain_random=True, obst_density_random=True, obst_size_random=True, num_envs=16, seed=3, **TEN_HZ), "f32")]
    for kw, E, precision, team, seed, _, _ in _layouts().values():
        jobs.append((dict(kw, num_envs=E, seed=seed, **NOISE_FREE, **run), precision, -1 if team is None else int(team)))
    return jobs


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_restore_is_complete_and_leaves_the_other_environments_alone(layout, monkeypatch):
    """replay_copy's addressing on every state layout: the team kernel's lane-major blocks, the single-wave kernels' row blocks, two
    environments per block (32 drones), a partial last block (13 environments of 5 drones, the tested one alone in block 1), the
    per-environment obstacle fields of --quads_domain_random, float64.

    Noise-free dynamics (no sensor noise, no thrust noise, no downwash: a drone in another one's downwash draws random numbers), 40-tick episodes, sample_prob 1.0, every other environment active (the last one always), actions from a table
    indexed by the environment's own tick.  A pair collision planted at tick 22 files the checkpoint of tick 10; the episode end
    restores it.  Then (1) every exposed array of the restored environment equals the host copy made when tick 10 was saved - except
    the four collision counters, which the kernel zeroes, and run_sums, which is NOT restored: the reward-shaping wrapper sits outside
    the replay wrapper, its sums restart with the episode (alloc_buffers: kind 2), so they are all zero after the restore; (2) the next
    ten steps reproduce observation, reward, done and exposed state of ticks 11...20 of the first pass bit for bit (run_sums apart:
    sums that start at tick 10 instead of 0) - which they only can if the arrays qs_buffers does not expose (scen_real / scen_int /
    scen_omap) came back too: in the dynamic_formations case the goals are regenerated on every step from the formation's size,
    speed and direction kept there (ep_lissajous3D, the float64 case, only keeps constants there: its goals follow the tick); (3) a twin handle without replay, given the same actions and
    plants, equals the replay handle bit for bit in every exposed array and output of the inactive environments on every step, and of
    the active ones up to their restore (but for the observation on the filing step, which is the filed checkpoint's).
    Premise, asserted from the device's masks: no collision with a drone, an obstacle or the room in ticks 1...21 of the tested
    environments, nor in the continuation (a collision response draws
    random numbers; a restored environment does not get the noise-stream position back) - the seeds were picked with the CPU oracle
    (seed 5 has such a collision in the 32-drone and in the float64 Lissajous case, seeds 12 and 3 have none).  The Lissajous and static-goal scenarios draw
    no goals inside an episode, dynamic_formations only when the formation's size reaches its bound; swarm_vs_swarm swaps goals after 4 s at the earliest, the end of these episodes."""
    from quad_swarm_rl_amd import native
    kw, E, precision, team, seed, epb, lane_major = _layouts()[layout]
    if team is not None:
        monkeypatch.setenv("QS_TEAM", team)
    active = np.array([(E - 1 - e) % 2 == 0 for e in range(E)], dtype=np.uint8)
    run = ReplayRun(dict(kw, **NOISE_FREE), E, 1.0, active, seed=seed, precision=precision)
    st, N, ep_len = run.st, run.N, run.cfg.ep_len
    twin = native.Stepper(run.cfg, device=0)
    twin.reset()
    assert st.bufs.envs_per_block == epb and (lane_major is None or st.bufs.state_lane_major == lane_major), (st.bufs.envs_per_block, st.bufs.state_lane_major)
    assert twin.team == st.team and st.team == (team is None if layout.startswith("c2") else st.team) and st.real_size == (8 if precision == "f64" else 4)
    table = _hover_table(ep_len + 2, N)
    tested = [e for e in range(E) if active[e]]
    outputs = EXPOSED + ("reward", "done")
    saved, first, restored, continued = {}, {e: {} for e in tested}, set(), dict.fromkeys(tested, 0)
    for step in range(ep_len + 1 + 10):
        for e in tested:
            if e not in restored and run.ticks[e] == 21:
                _plant_pair(st, e); _plant_pair(twin, e)
        act = table[run.ticks].reshape(E * N, 4)
        acts = run.step(act)
        twin.from_host("actions", act)
        twin.step()
        twin.sync()
        a, b = _grab(st, outputs), _grab(twin, outputs)
        for e in range(E):
            kinds = [x[0] for x in acts[e]]
            part = {n: _env_part(st, a[n], n, e) for n in outputs}
            t = int(run.ticks[e])
            if e in restored:                        # (2) the continuation from the restored checkpoint
                assert int(run.uq[e]) == 0 and int(run.on[e]) == 0 and int(a["room_new_mask"][e]) == 0, ("premise: a collision in the continuation", layout, e, t)
                differ = [n for n in outputs if n != "run_sums" and part[n].tobytes() != first[e][t][n].tobytes()]
                if differ:
                    _same_bits(part[differ[0]], first[e][t][differ[0]], (layout, "continuation", e, t, differ))
                continued[e] += 1
                continue
            if "restore" in kinds:                   # (1) the restore
                assert t == 10 and step == ep_len, (t, step)
                for n in EXPOSED:
                    want = saved[e][n].copy()
                    if n == "counters":
                        want[list(ZEROED_COUNTERS)] = 0
                    if n == "run_sums":
                        want[:] = 0
                    _same_bits(part[n], want, (layout, "restored", e, n))
                restored.add(e)
                continue
            for n in outputs:                        # (3) the twin
                if not (n == "obs" and "file" in kinds):
                    _same_bits(part[n], _env_part(twin, b[n], n, e), (layout, "twin", step, e, n))
            if e in tested:
                if t <= 21 and not run.done[e]:
                    assert int(run.uq[e]) == 0 and int(run.on[e]) == 0 and int(a["room_new_mask"][e]) == 0, ("premise: a collision before the planted one", layout, e, t)
                if t == 10:
                    assert kinds == ["save"]
                    saved[e] = part
                if 10 <= t <= 20:
                    first[e][t] = part
                if t == 22:
                    assert kinds == ["file"], ("premise: the planted collision files the checkpoint of tick 10", layout, e, kinds)
    print(f"{layout}: restored {sorted(restored)} of {E} environments ({st.bufs.envs_per_block} per block, lane-major {st.bufs.state_lane_major}, "
          f"team {st.team}), continuation steps checked {continued}, {len(EXPOSED)} arrays compared")
    assert sorted(restored) == tested and all(v == 10 for v in continued.values())
    assert (run.rs["errors"] == 0).all() and (run.rs["replayed"] == active).all()
    st.check_errors()
    twin.check_errors()
    st.close()
    twin.close()


def test_a_replayed_start_reports_the_obstacle_size_of_the_last_fresh_start():
    """replay/obst_size through the batched env with --quads_domain_random: the reference reports the wrapper's curr_obst_size, which only
    a fresh episode start assigns (quad_experience_replay.py:114-116, :202-204; pinned by
    tests/golden/wrapper_experience_replay_domain_random.json) - so after a replayed start it is the size reported at the environment's
    last fresh start, whatever size the restored checkpoint runs with; replay/obst_density follows the restored environment (:184).
    sample_prob 0.5, so that fresh episodes come between an event and its replays."""
    import torch
    from quad_swarm_rl_amd import sf_env
    E = 16
    env = sf_env.BatchedQuadSwarm(E, seed=3, replay_buffer_sample_prob=0.5, sim_freq=200.0, sim_steps=20,
                                  **dict(_c("c3_n8_obst"), ep_time=4.0, domain_random=True, obst_density_random=True, obst_size_random=True))
    st, N = env.vec.stepper, env.agents_per_env
    env.reset()
    st.replay_set_active(None)
    last_fresh = st.to_host("obst_size_env").astype(np.float64)
    seen = st.replay_stats()["replayed"].copy()
    planted = np.zeros(E, dtype=bool)
    act = torch.full((env.num_agents, 4), 0.06, device="cuda")
    replayed_starts = differs = fresh_starts = 0
    for _ in range(330):
        ticks = st.to_host("tick")
        for e in np.nonzero((ticks == 21) & ~planted)[0]:      # one event per environment, filed in its first episode
            _plant_pair(st, e)
            planted[e] = True
        obs, rew, term, trunc, infos = env.step(act)
        if len(infos):
            rs = st.replay_stats()
            size_env, density_env = st.to_host("obst_size_env").astype(np.float64), st.to_host("obst_density_env").astype(np.float64)
            for e in np.nonzero(term.view(E, N)[:, 0].cpu().numpy())[0]:
                stats = infos[e * N]["episode_extra_stats"]
                assert stats["replay/obst_density"] == density_env[e]
                if rs["replayed"][e] > seen[e]:
                    assert stats["replay/obst_size"] == last_fresh[e], (e, stats["replay/obst_size"], last_fresh[e], size_env[e])
                    replayed_starts += 1
                    differs += size_env[e] != last_fresh[e]
                else:
                    assert stats["replay/obst_size"] == size_env[e]
                    last_fresh[e] = size_env[e]
                    fresh_starts += 1
                seen[e] = rs["replayed"][e]
    print(f"replay/obst_size: {replayed_starts} replayed starts, {differs} of them from a checkpoint of another obstacle size than the last "
          f"fresh start's; {fresh_starts} fresh starts")
    assert replayed_starts >= 10 and differs >= 3 and fresh_starts >= 10
    env.close()

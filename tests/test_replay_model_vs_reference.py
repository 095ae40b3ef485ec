"""The replay kernel's decision logic (tests/replay_model.py, the Python twin of qs_replay_kernel) against the REFERENCE wrapper.

tests/golden/wrapper_experience_replay*.json hold what the reference's ExperienceReplayWrapper
(gym_art/quadrotor_multi/quad_experience_replay.py:66-209) did over the scripted env of tests/fake_env.py, one fixture per
schedule of fake_env.REPLAY_SCHEDULES, together with the random draws it made (oracle/ref_harness/capture_replay_wrapper.py):
  base           100 Hz, 9000 steps, 18 episodes, 14 replays - pair collisions only, never more than 4 events;
  full           10 Hz, a hit every ~23 steps of four kinds (drone pair, id 0 alone, obstacle hit by one drone): the 20-event buffer
                 fills up and is overwritten at buffer_idx, checkpoints are saved and filed on one step, the ring wraps all the time;
  cleanup        sample_prob 0.9 with rare hits - events reach their tenth replay and are dropped, buffer_idx runs ahead of the shrunken
                 deque - then frequent hits refill the buffer to 20 and overwrite at the stale buffer_idx;
  domain_random  the wrapper draws obstacle density and size per fresh episode and reports replay/obst_density, replay/obst_size.
Here the model makes the decisions, a small harness carries them out on the same scripted env (checkpoint = the env's copyable
core), and the trajectory and the replay statistics at every episode end must equal the reference's.  The harness counts which
branches the schedule drove; the floors below are conditions on the fixture, not measurements.  CPU only; tests/test_replay_gpu.py then
requires the device kernel to equal the model.

What domain_random settles: the reference reports replay/obst_size from curr_obst_size, which only a FRESH episode start assigns
(:114-116, :202-204), while replay/obst_density follows the replayed env (:184).  The harness below reports exactly that and equals the
fixture; reporting the restored env's size instead differs at the episode ends counted in `size_differs`."""
import json
import os

import numpy as np
import pytest

from tests.fake_env import REPLAY_SCHEDULES, FakeReplayEnv, unpack_trace
from tests.replay_model import EVENTS, RING, ReplayModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOORS = {
    "base": {},
    "full": {"overwrites_at_20": 10, "save_and_file": 3, "obstacle_of_drone0_alone": 5, "id0_only_no_filing": 1, "ring_wraps": 1},
    "cleanup": {"dropped": 5, "appends_with_stale_idx": 5, "overwrites_after_refill": 1},
    "domain_random": {"size_differs": 1, "replays": 10},
}


def run_model(name, report_restored_size=False):
    sched = REPLAY_SCHEDULES[name]
    want = json.load(open(os.path.join(GOLDEN, sched["file"])))
    if sched["compact"]:
        want["trajectory"] = unpack_trace(want["trajectory"], want["steps"])
    u, idx, choice = list(want["draws"]["uniform"]), list(want["draws"]["randint"]), list(want["draws"].get("choice", []))
    env = FakeReplayEnv(**sched["env"])
    freq = env.envs[0].control_freq
    model = ReplayModel(sched["sample_prob"], control_freq=freq, use_obstacles=env.use_obstacles, active=True)   # the scripted env's buffer is active from the start
    pool = [None] * (RING + EVENTS)
    dr = sched["wrapper"]
    n = dict.fromkeys(("overwrites_at_20", "save_and_file", "obstacle_of_drone0_alone", "id0_only_no_filing", "ring_wraps", "dropped",
                       "appends_with_stale_idx", "overwrites_after_refill", "size_differs", "replays", "max_len"), 0)

    def draw_idx(k):
        v = idx.pop(0)
        assert 0 <= v < k
        return v

    def fresh_draws():     # ExperienceReplayWrapper.reset / new_episode: one np.random.choice per randomised quantity
        nonlocal density, size
        d = s = None
        if dr:
            density = d = choice.pop(0)
            size = s = choice.pop(0)
        return d, s

    density, size = (0.0, 0.0) if dr else (0.2, 0.6)
    rec = {"x": {} if sched["compact"] else [], "tick": [], "episode": [], "ends": {}}
    obs = env.reset(*fresh_draws())
    for t in range(want["steps"]):
        obs, rewards, dones, infos = env.step(None)     # (the scripted env resets itself at done, like QuadrotorEnvMulti.step)
        ids, quad_col = env.last_step_unique_collisions, env.curr_quad_col
        mask, omask = sum(1 << int(i) for i in ids), sum(1 << int(i) for i in quad_col)
        before = (len(model.ev_slot), model.ev_idx, len(model.ck), model.saved)
        could_file = not dones[0] and not model.saved and env.envs[0].tick > model.grace and env.envs[0].tick - model.last_added > model.min_gap
        # `.any()` on the id array [0, 1] is True: the mask test (mask & ~1) != 0 sees id 1
        acts = model.step(bool(dones[0]), env.envs[0].tick, mask, omask, 0.0, lambda: u.pop(0), draw_idx)
        for act in acts:
            if act[0] == "save":
                pool[act[1]] = (env.core(), [o.copy() for o in obs])
                n["ring_wraps"] += before[2] == RING
            elif act[0] == "file":
                pool[act[2]] = pool[act[1]]
                obs = [o.copy() for o in pool[act[1]][1]]           # the reference returns the filed checkpoint's observation
                n["overwrites_at_20"] += before[0] == EVENTS
                n["overwrites_after_refill"] += before[0] == EVENTS and n["dropped"] > 0
                n["appends_with_stale_idx"] += before[0] < EVENTS and before[1] != before[0]
                n["save_and_file"] += len(acts) == 2
                n["obstacle_of_drone0_alone"] += (mask & ~1) == 0 and omask == 1
            elif act[0] == "fresh":
                obs = env.reset(*fresh_draws())                     # the wrapper's own reset() of a non-replayed episode
            else:
                core, ck_obs = pool[act[1]]
                env.set_core(core)
                env.collisions_per_episode = env.collisions_after_settle = 0
                obs = [o.copy() for o in ck_obs]
                density = env.obst_density                          # :184 - and curr_obst_size stays what the last fresh start drew
                n["dropped"] += before[0] - len(model.ev_slot)
                n["replays"] += 1
                n["size_differs"] += env.obst_size != size
                if report_restored_size:
                    size = env.obst_size
        n["id0_only_no_filing"] += could_file and mask == 1 and omask == 0 and before[2] >= 3 and not any(a[0] == "file" for a in acts)
        n["max_len"] = max(n["max_len"], len(model.ev_slot))
        rec["tick"].append(int(obs[0][1])); rec["episode"].append(int(obs[0][2]))
        if not sched["compact"]:
            rec["x"].append(float(obs[0][0]))
        if dones[0]:
            s = model.stats()
            stats = dict(infos[0]["episode_extra_stats"])
            stats.update({"replay/replay_rate": s["replayed"] / s["episodes"], "replay/new_episode_rate": (s["episodes"] - s["replayed"]) / s["episodes"],
                          "replay/replay_buffer_size": s["buffer_len"], "replay/avg_replayed": (s["replayed_sum"] / s["buffer_len"]) if s["buffer_len"] else 0,
                          "replay/obst_density": density, "replay/obst_size": size})
            rec["ends"][str(t)] = {k: float(v) for k, v in sorted(stats.items())}
            if sched["compact"]:
                rec["x"][str(t)] = float(obs[0][0])
    return want, rec, n, (u, idx, choice), model


@pytest.mark.parametrize("name", list(REPLAY_SCHEDULES))
def test_model_reproduces_the_reference_wrapper(name):
    want, rec, n, left, model = run_model(name)
    ref = want["trajectory"]
    assert rec["tick"] == ref["tick"] and rec["episode"] == ref["episode"]
    assert rec["x"] == ref["x"]                                      # bit for bit: the same arithmetic on the same state
    assert sorted(rec["ends"]) == sorted(ref["ends"]) and len(ref["ends"]) >= 15
    for t in ref["ends"]:
        assert rec["ends"][t] == pytest.approx(ref["ends"][t]), (t, rec["ends"][t], ref["ends"][t])
    assert not any(left)                # every draw of the reference was asked for, in order
    assert model.errors == 0
    print(name, "branches reached:", {k: int(v) for k, v in n.items()})
    for k, floor in FLOORS[name].items():
        assert n[k] >= floor, (k, n[k], floor)
    if name == "full":
        assert n["max_len"] == EVENTS


def test_obst_size_of_a_replayed_start_is_the_last_fresh_draw():
    """the other reading - replay/obst_size follows the restored env like replay/obst_density does - does not reproduce the fixture"""
    want, rec, n, _, _ = run_model("domain_random", report_restored_size=True)
    ref = want["trajectory"]["ends"]
    differ = [t for t in ref if rec["ends"][t]["replay/obst_size"] != pytest.approx(ref[t]["replay/obst_size"])]
    assert differ and all(rec["ends"][t]["replay/obst_density"] == pytest.approx(ref[t]["replay/obst_density"]) for t in ref)
    sizes = {ref[t]["replay/obst_size"] for t in ref}
    assert len(sizes) >= 3 and len({ref[t]["replay/obst_density"] for t in ref}) >= 3, sizes
    assert np.isfinite(list(sizes)).all()

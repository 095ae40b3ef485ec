#!/usr/bin/env python
"""Build-container only (needs /root/reference): runs the reference's ExperienceReplayWrapper
(gym_art/quadrotor_multi/quad_experience_replay.py:66-209) over the scripted env of tests/fake_env.py (FakeReplayEnv) and writes the
trajectory it produces - which episodes were replays, from which checkpoint, the replay statistics - together with the random
draws it made (one U(0,1) per new episode, one index per sampled event, the np.random.choice draws of --quads_domain_random) to
tests/golden/.  One fixture per schedule of tests/fake_env.py: REPLAY_SCHEDULES;

    capture_replay_wrapper.py [schedule ...]      (default: all of them; `base` rewrites wrapper_experience_replay.json byte for byte)"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "stubs"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, REPO)

import gymnasium as gym                                                             # noqa: E402  (the stub)
from gym_art.quadrotor_multi import quad_experience_replay as ref                    # noqa: E402
from tests.fake_env import REPLAY_SCHEDULES, FakeReplayEnv, drive_replay, pack_trace             # noqa: E402

if not hasattr(gym.Wrapper, "__getattr__"):
    gym.Wrapper.__getattr__ = lambda self, name: getattr(self.__dict__["env"], name)
ref.print = lambda *a, **k: None


def capture(name):
    sched = REPLAY_SCHEDULES[name]
    draws = {"uniform": [], "randint": []}
    if sched["wrapper"]:
        draws["choice"] = []
    _uniform, _randint, _choice = np.random.uniform, random.randint, np.random.choice

    def rec_uniform(*a, **k):
        v = float(_uniform(*a, **k))
        draws["uniform"].append(v)
        return v

    def rec_randint(a, b):
        v = _randint(a, b)
        draws["randint"].append(int(v))
        return v

    def rec_choice(a):
        v = _choice(a)
        draws["choice"].append(float(v))
        return v

    ref.np.random.uniform, ref.random.randint, ref.np.random.choice = rec_uniform, rec_randint, rec_choice
    np.random.seed(7)
    random.seed(7)
    try:
        env = FakeReplayEnv(**sched["env"])
        w = ref.ExperienceReplayWrapper(env, sched["sample_prob"], 0.2, 0.6, **sched["wrapper"])
        rec = drive_replay(w, sched["steps"], compact=sched["compact"])
    finally:
        ref.np.random.uniform, ref.random.randint, ref.np.random.choice = _uniform, _randint, _choice
    out = {"steps": sched["steps"], "draws": draws, "trajectory": pack_trace(rec) if sched["compact"] else rec}
    path = os.path.join(REPO, "tests", "golden", sched["file"])
    json.dump(out, open(path, "w"), sort_keys=True, separators=(", ", ": ") if not sched["compact"] else (",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes; episodes", len(rec["ends"]), "uniform draws", len(draws["uniform"]), "sampled events",
          len(draws["randint"]), "resets", len(env.scenes))


for schedule in sys.argv[1:] or list(REPLAY_SCHEDULES):
    capture(schedule)

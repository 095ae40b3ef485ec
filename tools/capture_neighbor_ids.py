#!/usr/bin/env python
"""Fixtures of the neighbour identities: the reference environment's own `neighborhood_indices` results, as step() and reset() used them.

Runs the reference the way oracle/ref_harness/capture.py runs its cases (same recorders, same file format: tests/golden_util.py and the
tape replay of tests/test_hip_vs_reference.py read the result unchanged) and adds two arrays:

    nbr_idx0 [N, K]       the indices behind the rows reset() returned
    nbr_idx  [T, N, K]    the indices behind the rows step t returned - at an episode end those of the reset inside the step

The method is wrapped, not called afterwards: at a reset the reference ranks with the previous episode's velocities (the dynamics objects
are reset later), so a call after the fact would re-rank with fresh ones.

Every ranking that was used must be decided by a margin: consecutive entries among the first K + 1 of the sorted metric differ by at least
GAP.  The float64 tape kernels meet the reference to 1e-9, so with that margin their ranking cannot differ and a GPU replay needs no excused
rows.  A condition on the inputs, not a tolerance: seeds are tried until one holds.  TEST INFRASTRUCTURE - needs the reference checkout that
oracle/ref_harness/capture.py imports.

Usage:  python tools/capture_neighbor_ids.py [case ...]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.ref_harness import capture as cap  # noqa: E402

GAP = 1e-6
STEPS = 64
CASES = {
    # N = 8, K = 2 among obstacles, 0.25-s episodes: ends at steps 25 and 51
    "nbr_n8_k2_obst": dict(cfg=dict(cap.OBST, quads_mode="o_static_same_goal", ep_time=0.25), seed=91),
    # N = 12, K = 6, two swarms, 0.2-s episodes: three ends
    "nbr_n12_k6_svs": dict(cfg=dict(num_agents=12, neighbor_visible_num=6, quads_mode="swarm_vs_swarm", ep_time=0.2), seed=92),
}


class Recorder:
    """wraps QuadrotorEnvMulti.neighborhood_indices and .step on the class for the length of one run"""

    def __init__(self):
        self.calls, self.per_step, self.min_gap = [], [], np.inf
        self.cls = cap.QuadrotorEnvMulti
        self.orig_idx, self.orig_step = self.cls.neighborhood_indices, self.cls.step

    def __enter__(self):
        rec = self

        def neighborhood_indices(env):
            out = rec.orig_idx(env)
            K, N = env.num_use_neighbor_obs, env.num_agents
            if 1 <= K < N - 1:   # the metric as quadrotor_multi.py:258-268 forms it, from what the environment holds at THIS moment
                for i in range(N):
                    others = [j for j in range(N) if j != i]
                    rel_pos, rel_vel = env.get_rel_pos_vel_item(env_id=i, indices=others)
                    rel_dist = np.maximum(np.linalg.norm(rel_pos, axis=1), 0.01)
                    metric = np.sort(rel_dist + np.sum(rel_pos / rel_dist[:, None] * rel_vel, axis=1))
                    rec.min_gap = min(rec.min_gap, float(np.diff(metric[:K + 1]).min()))
            rec.calls.append(np.array([np.asarray(r) for r in out], dtype=np.int32))
            return out

        def step(env, actions):
            out = rec.orig_step(env, actions)
            rec.per_step.append(rec.calls[-1])   # a step that ends the episode calls twice: the reset's ranking is behind the rows it returns
            return out

        self.cls.neighborhood_indices, self.cls.step = neighborhood_indices, step
        return self

    def __exit__(self, *exc):
        self.cls.neighborhood_indices, self.cls.step = self.orig_idx, self.orig_step


def capture(name, tries=50):
    spec = CASES[name]
    path = os.path.join(cap.GOLDEN_DIR, name + ".npz")
    for seed in range(spec["seed"], spec["seed"] + tries):
        with Recorder() as rec:
            cap.run_case(name, cap.default_cfg(**spec["cfg"]), steps=STEPS, seed=seed, slim=True)
        g = dict(np.load(path))
        ends = int(g["done"].any(axis=1).sum())
        if rec.min_gap < GAP or ends < 2:
            print(f"{name}: seed {seed} has a ranking decided by {rec.min_gap:.3g} (< {GAP:g}) or {ends} < 2 episode ends - next seed")
            os.remove(path)
            continue
        assert len(rec.per_step) == STEPS and len(rec.calls) == 1 + STEPS + ends
        g["nbr_idx0"], g["nbr_idx"] = rec.calls[0], np.stack(rec.per_step)
        np.savez_compressed(path, **g)
        print(f"{name}: seed {seed}, {ends} episode ends, smallest gap among the first K + 1 metrics {rec.min_gap:.3g}, nbr_idx {g['nbr_idx'].shape} "
              f"-> {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
        return
    raise SystemExit(f"{name}: no seed of {tries} gives rankings decided by {GAP:g}")


if __name__ == "__main__":
    cap.install_recorders()
    for nm in sys.argv[1:] or list(CASES):
        capture(nm)

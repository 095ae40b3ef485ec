#!/usr/bin/env python
"""The position controller's launch (include/quadswarm_control.h) timed beside the step it feeds, and what the controller achieves as a baseline.
Recorded, not gated.

  python tools/bench_pilot.py --prebuild     (no GPU) compile the config-specialised code objects of the shapes below into spec_cache/
  python tools/bench_pilot.py                (GPU)    -> profiles/pilot_kernel_times.txt, profiles/pilot_baseline.txt (--out-dir: elsewhere)

Times: float32, the C2 configuration of bench.py at 8 x 1024 and at 2^20 drones, both element orders of the state blocks (QS_TEAM picks the
kernel flavour and with it the order).  Each figure is device-event time around `--launches` back-to-back launches on one stream, divided
by their number, after a warm-up: at the small shape that is the launch cadence of the queue rather than the kernel's own duration.  Byte
floor of the pilot launch: 100 B per drone in float32 (21 state elements read, one 16-byte row written) at the 6.29 TB/s copy rate.

Baseline: one episode at E = 1024 flown by step_pilot alone - static_diff_goal (8 drones) and swarm_vs_swarm (32 drones): mean distance to the
goal over the last second (the step kernel's own episode statistic, distance_to_goal_1s) and drone-drone collisions per episode.  The
controller knows nothing of neighbours: the collisions are the point of the record."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from quad_swarm_rl_amd import config as qcfg, native  # noqa: E402

C2 = bench.WORKLOADS["c2"]["kw"]
SHAPES = [(1024, None), (1024, "0"), (131072, None), (131072, "1")]    # (environments of 8 drones, QS_TEAM)
BASELINES = [("static_diff_goal", dict(C2, quads_mode="static_diff_goal")), ("swarm_vs_swarm", bench.WORKLOADS["c4"]["kw"])]
COPY_RATE, FLOOR_BYTES = 6.29e12, 100


def with_team(team, fn):
    saved = os.environ.get("QS_TEAM")
    if team is not None:
        os.environ["QS_TEAM"] = team
    try:
        return fn()
    finally:
        if team is not None:
            os.environ.pop("QS_TEAM", None)
            if saved is not None:
                os.environ["QS_TEAM"] = saved


def prebuild():
    for E, team in SHAPES:
        print(native.spec_build(qcfg.make_config(num_envs=E, precision="f32", write_rew_info=False, **C2), -1 if team is None else int(team)))
    for _, kw in BASELINES:
        print(native.spec_build(qcfg.make_config(num_envs=1024, precision="f32", write_rew_info=False, **kw)))


def timed(torch, fn, launches, warmup=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches    # us per launch


def kernel_times(torch, launches):
    lines = ["# us per launch, float32, device events around %d back-to-back launches (tools/bench_pilot.py)" % launches,
             "# drones  lane_major  kernel            pilot_us  step_us  pilot_floor_us  pilot/floor"]
    for E, team in SHAPES:
        cfg = qcfg.make_config(num_envs=E, seed=0, precision="f32", write_rew_info=False, **C2)
        st = with_team(team, lambda: native.Stepper(cfg, device=0))
        st.reset()
        stream = torch.cuda.current_stream()
        st.pilot_actions(stream=stream)
        for _ in range(20):                       # a state in flight, not the spawn
            st.step(stream=stream)
        n = 3 if E > 4096 else 1                  # best of n windows: other work shares the machine
        pilot = min(timed(torch, lambda: st.pilot_actions(stream=stream), launches) for _ in range(n))
        step = min(timed(torch, lambda: st.step(stream=stream), launches) for _ in range(n))
        st.check_errors()
        floor = st.T * FLOOR_BYTES / COPY_RATE * 1e6
        lines.append(f"{st.T:8d}  {st.bufs.state_lane_major:10d}  {st.kernel_name:16s}  {pilot:8.2f}  {step:7.2f}  {floor:14.2f}  {pilot / floor:11.1f}"
                     + ("   # FINDING: the pilot launch is slower than the step it feeds" if pilot > step else ""))
        print(lines[-1], flush=True)
        st.close()
    return lines


def baselines(torch):
    from quad_swarm_rl_amd import env as qenv
    lines = ["# one episode flown by step_pilot alone, E = 1024, float32 (tools/bench_pilot.py)",
             "# scenario  drones_per_env  steps  mean_distance_to_goal_last_1s_m  worst_m  collisions_per_episode  floor_crashes_per_episode"]
    for name, kw in BASELINES:
        venv = qenv.QuadSwarmVecEnv(1024, seed=0, precision="f32", write_rew_info=False, **kw)
        venv.reset()
        steps, done = 0, None
        while steps < venv.cfg.ep_len + 8:
            _, _, done, _ = venv.step_pilot()
            steps += 1
            if steps > venv.cfg.ep_len - 2 and bool(done.any()):
                break
        torch.cuda.synchronize()
        venv.stepper.check_errors()
        assert bool(done.all()), "the episode did not end"
        eps, cnt = venv.stepper.to_host("ep_stats").astype(np.float64), venv.stepper.to_host("ep_counters")
        k = qcfg.COUNTER_KEYS
        lines.append(f"{name}  {venv.cfg.num_agents}  {steps}  {eps[0].mean():.4f}  {eps[0].max():.4f}  {cnt[k.index('collisions')].mean():.3f}  "
                     f"{cnt[k.index('floor')].mean():.3f}")
        print(lines[-1], flush=True)
        venv.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prebuild", action="store_true")
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    if args.prebuild:
        return prebuild()
    import torch
    if not torch.cuda.is_available():
        raise native.QsError("tools/bench_pilot.py measures on a GPU (--prebuild is the part that needs none)")
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "pilot_kernel_times.txt"), "w") as f:
        f.write("\n".join(kernel_times(torch, args.launches)) + "\n")
    if not args.no_baseline:
        with open(os.path.join(args.out_dir, "pilot_baseline.txt"), "w") as f:
            f.write("\n".join(baselines(torch)) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What the neighbour-identity launch (include/quadswarm_neighbors.h: qs_neighbor_ids) costs, beside the step of the same handle.  Recorded, not
gated: a diagnostic has no roofline target.  The one expectation is that it takes no longer than the qs_step it is measured beside - it reads
24 (1 + K) bytes and writes 4 K bytes per drone in float32, a fraction of what a step moves; a line where it does carries a FINDING mark.

  python tools/bench_neighbor_ids.py --prebuild     (no GPU) compile the config-specialised code objects of the shapes below into spec_cache/
  python tools/bench_neighbor_ids.py                (GPU)    -> profiles/r18_bench_neighbor_ids.txt (--out: elsewhere)

Shapes, float32: the C2 handle of bench.py (1024 environments of 8 drones, K = 6) and 2^17 drones as 16384 x 8 and as 4096 x 32 (the C4
configuration), K = 6.  Method: 50 calls recorded into one HIP graph per launch kind; device events around 20 replays of a graph; 5 rounds
that alternate the two kinds in one process; the median round and the rounds' spread (min .. max) per kind, in us per call.  At the small
shape that is the launch cadence inside a graph rather than the kernel's own duration, for both kinds alike."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from quad_swarm_rl_amd import config as qcfg, native  # noqa: E402

SHAPES = [("c2", 1024), ("c2", 16384), ("c4", 4096)]      # (workload of bench.py, environments)
CALLS, REPLAYS, ROUNDS = 50, 20, 5


def config(workload, E):
    return qcfg.make_config(num_envs=E, seed=0, precision="f32", write_rew_info=False, **bench.WORKLOADS[workload]["kw"])


def prebuild():
    for workload, E in SHAPES:
        print(native.spec_build(config(workload, E)))


def captured(torch, fn):
    """CALLS calls of fn recorded into one graph (one eager call on a side stream first: library warm-up outside the capture)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    torch.cuda.synchronize()
    return g


def us_per_call(torch, g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPLAYS):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (REPLAYS * CALLS)


def measure(torch):
    lines = [f"# us per call, float32: {CALLS} calls per HIP graph, device events around {REPLAYS} replays, {ROUNDS} rounds alternating the two launch kinds in one",
             "# process; median round (min .. max of the rounds)   (tools/bench_neighbor_ids.py)",
             "# drones  N   K  lane_major  step kernel       neighbor_ids_us (spread)        qs_step_us (spread)             ids/step  slots without a drone"]
    for workload, E in SHAPES:
        st = native.Stepper(config(workload, E), device=0)
        st.reset()
        st.from_host("actions", torch.rand((st.T, 4), generator=torch.Generator().manual_seed(1)).numpy() * 2 - 1)
        for _ in range(20):                                   # a state in flight, not the spawn
            st.step(stream=torch.cuda.current_stream())
        out = torch.empty((st.T, int(st.cfg.num_neighbors)), device="cuda", dtype=torch.int32)
        g_ids = captured(torch, lambda: st.neighbor_ids(out=out))
        g_step = captured(torch, lambda: st.step(stream=torch.cuda.current_stream()))
        for g in (g_ids, g_step):                             # both graphs once, untimed
            g.replay()
        torch.cuda.synchronize()
        ids_us, step_us = [], []
        for _ in range(ROUNDS):
            ids_us.append(us_per_call(torch, g_ids))
            step_us.append(us_per_call(torch, g_step))
        st.check_errors()
        missing = int((st.neighbor_ids() < 0).sum().item())   # rows and state of one moment: none
        mi, ms = statistics.median(ids_us), statistics.median(step_us)
        lines.append(f"{st.T:8d}  {st.N:2d}  {int(st.cfg.num_neighbors):2d}  {st.bufs.state_lane_major:10d}  {st.kernel_name:16s}  "
                     f"{mi:8.2f} ({min(ids_us):.2f} .. {max(ids_us):.2f})   {ms:8.2f} ({min(step_us):.2f} .. {max(step_us):.2f})   {mi / ms:8.2f}  {missing}"
                     + ("   # FINDING: the launch is slower than the step it is measured beside" if mi > ms else ""))
        print(lines[-1], flush=True)
        st.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prebuild", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r18_bench_neighbor_ids.txt"))
    args = ap.parse_args()
    if args.prebuild:
        return prebuild()
    import torch
    if not torch.cuda.is_available():
        raise native.QsError("tools/bench_neighbor_ids.py measures on a GPU (--prebuild is the part that needs none)")
    lines = measure(torch)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

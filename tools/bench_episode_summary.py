#!/usr/bin/env python
"""What the learning-curve numbers of a step on which EVERY environment finishes cost, both ways in ONE process on one device, at 1024
environments x 8 drones under `mix` (6-step episodes, so that all end together on every sixth step):

  (a) the host path: step() + infos.materialize() (one dict per finished agent) + a key-by-key host average of the dicts
  (b) the device path: step() of an env created with episode_summary=True (the two summary launches ride behind the step) +
      episode_summary() (two small copies, one pure function)

(a) and (b) alternate on two envs of the same seed; each timed window is a host clock around work that ends in a device synchronise; medians
of --reps windows after a warm-up.  Beside them, from device events in the same run: one step() call and the two summary launches
(qs_summary_partial_kernel + qs_summary_fold_kernel) on an all-ended step, and on a step on which nothing ended.  One JSON line; --out writes
a text record as well.

    python tools/bench_episode_summary.py
    python tools/bench_episode_summary.py --envs 16384 --reps 11
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EP_TIME, EP_STEPS = 0.055, 6


def host_average(infos):
    """what a consumer of the dicts does today: the mean of every key over the dicts that have it"""
    vals = {}
    for d in infos.materialize():
        if d:
            vals.setdefault("true_reward", []).append(d["true_reward"])
            for k, v in d["episode_extra_stats"].items():
                vals.setdefault(k, []).append(v)
    return {k: math.fsum(v) / len(v) for k, v in vals.items()}


def event_us(torch, fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=1024)
    p.add_argument("--agents", type=int, default=8)
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", type=str, default="")
    a = p.parse_args(argv)
    import torch
    from quad_swarm_rl_amd import sf_env
    if not torch.cuda.is_available():
        raise SystemExit("bench_episode_summary: needs the GPU (nothing here is a measurement without one)")
    kw = dict(seed=1, num_agents=a.agents, neighbor_visible_num=min(6, a.agents - 1), neighbor_obs_type="pos_vel" if a.agents > 1 else "none",
              use_downwash=True, use_numba=True, collision_falloff_radius=4.0, ep_time=EP_TIME, quads_mode="mix")
    host, dev = sf_env.BatchedQuadSwarm(a.envs, **kw), sf_env.BatchedQuadSwarm(a.envs, episode_summary=True, **kw)
    gen = torch.Generator().manual_seed(3)
    acts = [(torch.rand((host.num_agents, 4), generator=gen) * 2 - 1).cuda() for _ in range(EP_STEPS)]
    host.reset(); dev.reset()
    stream = torch.cuda.current_stream()
    st = dev.vec.stepper
    t_host, t_dev, t_lazy, ev_step, ev_summ, ev_summ_idle, keys = [], [], [], [], [], [], (0, 0)
    for rep in range(a.warmup + a.reps):
        for t in range(EP_STEPS - 1):   # the steps on which nothing ends: not timed, but for the summary launches on such a step
            host.step(acts[t]); dev.step(acts[t])
        idle = event_us(torch, lambda: st.episode_summary_accumulate(stream=stream), stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        infos = host.step(acts[-1])[4]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        avg = host_average(infos)
        t2 = time.perf_counter()
        dev.step(acts[-1])
        summary = dev.episode_summary(clear=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert len(infos.finished_agents()) == host.num_agents and summary["episodes"] == a.envs
        # device events: the summary launches repeated on the buffers of the step that just ended everything (the window is cleared after), and
        # one step() call - the next episode's first step: the same kernel, the same work but for the auto-reset tail
        summ_us = event_us(torch, lambda: st.episode_summary_accumulate(stream=stream), stream)
        dev.episode_summary(clear=True)
        step_us = event_us(torch, lambda: dev.step(acts[0]), stream)
        host.step(acts[0])
        for t in range(1, EP_STEPS):   # finish that episode outside the timed windows, keep both envs in step
            host.step(acts[t]); dev.step(acts[t])
        dev.episode_summary(clear=True)
        if rep >= a.warmup:
            t_lazy.append((t1 - t0) * 1e3); t_host.append((t2 - t0) * 1e3); t_dev.append((t3 - t2) * 1e3)
            ev_step.append(step_us); ev_summ.append(summ_us); ev_summ_idle.append(idle)
            keys = (len(avg), len(summary))
    med = statistics.median
    rec = dict(tool="bench_episode_summary", envs=a.envs, agents=a.agents, scenario="mix", reps=a.reps, warmup=a.warmup,
               host_path_ms=dict(median=round(med(t_host), 3), min=round(min(t_host), 3), max=round(max(t_host), 3),
                                 of_which_step_with_lazy_infos=round(med(t_lazy), 3)),
               device_path_ms=dict(median=round(med(t_dev), 3), min=round(min(t_dev), 3), max=round(max(t_dev), 3)),
               speedup=round(med(t_host) / med(t_dev), 1),
               device_events_us=dict(step_call=round(med(ev_step), 1), summary_two_launches_all_ended=round(med(ev_summ), 1),
                                     summary_two_launches_nothing_ended=round(med(ev_summ_idle), 1)),
               keys=dict(host_average=keys[0], summary=keys[1]), step_kernel=st.kernel_name, device=torch.cuda.get_device_name(0))
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    host.close(); dev.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

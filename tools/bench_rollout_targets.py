#!/usr/bin/env python
"""What it costs to turn a recorded rollout segment into what PPO consumes (values, log-probabilities, GAE advantages, returns), at the
config-5 shape (1024 envs x 8 drones, 128-step segments), both ways in ONE process on one device, timed with device events:

  (a) the framework way (tools/ppo_c5.py without --device_targets): the float32 torch critic over all (T + 1) * A observation rows in
      65536-row slices, gaussian_logp as elementwise torch kernels, the Python GAE loop of T iterations;
  (b) inside the segment (rollout.GraphedRollout critic= / targets=): us per control step of the captured graph with and without them, the
      fused critic pass alone, and the finishing kernel (qs_rollout_targets) alone - both forms of its scan (qs_rollout_set_targets_chunks),
      launches back to back inside a HIP graph, on one buffer set (cache-warm) and rotating over more sets than the 256 MiB last-level
      cache holds, with the achieved bytes/s next to the measured float4-copy rate of the device (MI355X: 6.29 TB/s).

Medians of repeated runs after a warm-up.  One JSON line per encoder; --out appends them to a file as well.

    python tools/bench_rollout_targets.py                       # mean_embed and attention
    python tools/bench_rollout_targets.py --encoders mean_embed --envs 256 --steps 32
"""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COPY_RATE = 6.29e12          # bytes/s, float4 copy measured on MI355X: the ceiling of a streaming kernel
ROW_READ, ROW_WRITE = 4 + 1 + 4 + 16 + 16, 12   # reward, done flag, value, mean row, action row -> logp, advantage, return


def timed(torch, fn, reps, inner=1):
    """median over `reps` of the device time of `inner` back-to-back calls of fn, in us per call"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(out), min(out), max(out)


def graph_timed(torch, fns, reps):
    """the calls of `fns` recorded back to back into one HIP graph (no host cost between the launches): median us per call over `reps` replays"""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for fn in fns:
            fn()
    g.replay()
    torch.cuda.synchronize()
    med, lo, hi = timed(torch, g.replay, reps)
    return med / len(fns), lo / len(fns), hi / len(fns)


def bench(nbr_encoder, E, T, precision, reps):
    import torch
    import ppo_c5
    from quad_swarm_rl_amd import policy, rollout
    from quad_swarm_rl_amd.env import QuadSwarmVecEnv
    kw = dict(num_agents=8, neighbor_visible_num=6, neighbor_obs_type="pos_vel", use_numba=True, collision_falloff_radius=4.0, write_rew_info=False)
    targets = dict(gamma=0.99, gae_lambda=1.0, reward_scale=1.0, reward_clip=10.0)      # train_local.sh / Sample Factory defaults
    res = {"workload": f"config-5 shape: {E} envs x 8 drones, {T}-step segments, {nbr_encoder} encoders, {precision} operands", "reps": reps}

    def make(with_critic):
        env = QuadSwarmVecEnv(E, seed=0, **kw)
        env.reset()
        enc = policy.FusedQuadEncoder(policy.make_reference_encoder(seed=0, nbr_encoder=nbr_encoder).cuda(), precision=precision)
        head = rollout.GaussianActionHead(sample=True)
        module = policy.make_reference_encoder(seed=1, nbr_encoder=nbr_encoder).cuda()
        torch.manual_seed(2)
        value = torch.nn.Linear(512, 1).cuda()
        extra = {}
        if with_critic:
            critic = policy.FusedQuadEncoder(module, precision=precision)
            critic.set_head(value.weight, value.bias)
            extra = dict(critic=critic, targets=targets)
        return env, rollout.GraphedRollout(env, enc, head, steps=T, **extra), head, module, value, extra.get("critic")

    env_a, seg_a, _, _, _, _ = make(False)
    env_b, seg_b, head, module, value, critic = make(True)
    for _ in range(3):
        seg_a.run(); seg_b.run()
    torch.cuda.synchronize()
    # (b) the segment with and without critic + targets, alternating
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(torch, seg_a.run, 1)[0])
        tb.append(timed(torch, seg_b.run, 1)[0])
    res["segment_us_per_control_step"] = {"plain": statistics.median(ta) / T, "with_critic_and_targets": statistics.median(tb) / T,
                                          "plain_min_max": [min(ta) / T, max(ta) / T], "with_min_max": [min(tb) / T, max(tb) / T]}
    res["segment_added_us"] = statistics.median(tb) - statistics.median(ta)
    out = seg_b.run()
    torch.cuda.synchronize()
    A, D = out["last_obs"].shape
    rows = (T + 1) * A

    # (a) the framework way on the same recorded buffers
    obs = torch.cat((out["obs"].reshape(T * A, D), out["last_obs"]))
    vals = torch.empty(rows, device="cuda")

    def torch_values():   # tools/ppo_c5.py collect_fused: the flat (T + 1) * A rows in 65536-row slices
        with torch.no_grad():
            for s0 in range(0, rows, 65536):
                vals[s0:s0 + 65536] = value(module(obs[s0:s0 + 65536])).squeeze(-1)

    logp_buf = torch.empty((T, A), device="cuda")

    def torch_logp():
        logp_buf.copy_(ppo_c5.gaussian_logp(out["means"], head.log_std, out["actions"]))

    me = types.SimpleNamespace(torch=torch, cfg=types.SimpleNamespace(rollout=T, **targets), rew=out["rewards"], done=out["dones"].float(),
                               val=out["values"])

    def torch_gae():
        ppo_c5.Learner.advantages(me)

    for fn in (torch_values, torch_logp, torch_gae):
        fn(); fn()
    torch.cuda.synchronize()
    a = {"critic_torch_fp32_65536_row_slices": timed(torch, torch_values, max(3, reps // 2))[0], "gaussian_logp_torch": timed(torch, torch_logp, reps)[0],
         "gae_python_loop": timed(torch, torch_gae, reps)[0]}
    a["total"] = sum(a.values())
    res["framework_way_us"] = a
    res["critic_torch_us_per_8192_rows"] = a["critic_torch_fp32_65536_row_slices"] * 8192 / rows

    # (b) the pieces: the fused critic pass, the finishing kernel
    v2 = torch.empty((rows, 1), device="cuda")

    def fused_values():
        for s0 in range(0, T * A, 65536):
            critic.forward_head(obs[s0:min(T * A, s0 + 65536)], head_out=v2[s0:min(T * A, s0 + 65536)])
        critic.forward_head(obs[T * A:], head_out=v2[T * A:])

    fused_values(); fused_values()
    torch.cuda.synchronize()
    res["critic_fused_us"] = timed(torch, fused_values, reps)[0]
    res["critic_fused_us_per_8192_rows"] = res["critic_fused_us"] * 8192 / rows
    # (the `attention` encoder pairs rows across a batch, so the two sides compute the same function only where their slices coincide: T * A a
    # multiple of 65536, as at the config-5 shape, or mean_embed)
    if nbr_encoder != "attention" or (T * A) % 65536 == 0:
        res["critic_fused_vs_torch_max_abs_diff"] = float((v2.reshape(-1) - vals).abs().max())

    nbytes = T * A * (ROW_READ + ROW_WRITE) + 4 * A
    sets = min(16, max(2, -(-(300 << 20) // nbytes)))   # at the config-5 shape: more than the last-level cache holds
    names = ("rewards", "dones", "values", "means", "actions")
    bufs = [{k: out[k].clone() for k in names} for _ in range(sets)]
    outs = [[torch.empty((T, A), device="cuda") for _ in range(3)] for _ in range(sets)]

    def kernel(i):
        b, o = bufs[i], outs[i]
        policy.rollout_targets(b["rewards"], b["dones"], b["values"], means=b["means"], actions=b["actions"], log_std=head.log_std, logp=o[0],
                               advantages=o[1], returns=o[2], **targets)

    L = policy.lib()
    forms = {}
    for chunks in (0, 1, 16):   # the default rule, the plain form, the chunked form
        prev = L.qs_rollout_set_targets_chunks(chunks)
        for i in range(sets):
            kernel(i)
        torch.cuda.synchronize()
        warm = graph_timed(torch, [lambda: kernel(0)] * 48, reps)
        cold = graph_timed(torch, [lambda i=i: kernel(i % sets) for i in range(8 * sets)], reps)
        forms["default" if chunks == 0 else f"chunks_{chunks}"] = {
            "warm_us": warm[0], "rotating_us": cold[0], "rotating_min_max_us": [cold[1], cold[2]], "rotating_bytes_per_s": nbytes / (cold[0] * 1e-6),
            "rotating_share_of_copy_rate": nbytes / (cold[0] * 1e-6) / COPY_RATE, "warm_bytes_per_s": nbytes / (warm[0] * 1e-6)}
        L.qs_rollout_set_targets_chunks(prev)
    res["finishing_kernel"] = {"bytes_per_launch": nbytes, "buffer_sets_rotated": sets, "copy_rate_ceiling_bytes_per_s": COPY_RATE, "forms": forms}
    res["device_way_us"] = {"critic_fused": res["critic_fused_us"], "qs_rollout_targets": forms["default"]["rotating_us"],
                            "total": res["critic_fused_us"] + forms["default"]["rotating_us"], "segment_added": res["segment_added_us"]}
    env_a.close(); env_b.close()
    return res


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--encoders", nargs="+", default=["mean_embed", "attention"])
    p.add_argument("--envs", type=int, default=1024)
    p.add_argument("--steps", type=int, default=128)
    p.add_argument("--precision", choices=("bf16", "fp32"), default="fp32", help="operands of the fused actor and critic (tools/ppo_c5.py --sampler_precision)")
    p.add_argument("--reps", type=int, default=11)
    p.add_argument("--out", default=None)
    cfg = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_targets needs a GPU: there is nothing to time without one")
    for enc in cfg.encoders:
        line = json.dumps(bench(enc, cfg.envs, cfg.steps, cfg.precision, cfg.reps))
        print(line, flush=True)
        if cfg.out:
            with open(cfg.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""What the attention weights cost (quad_swarm_rl_amd/attention.py, include/quadswarm_attention.h) at 8192 agents, per encoder class, in one process:

  * the probe (qs_attn_weights: one launch, two for the attention neighbour encoder);
  * the full forward pass of the same class in reference precision (qs_enc_forward, FusedQuadEncoder(precision="fp32")): the probe runs a strict
    subset of its work and must not be slower;
  * the torch module in fp32 with the forward hooks that are the only other way to the weights (eager; host clock around a synchronise).

The probe and the forward pass are timed the same way: CALLS back-to-back calls recorded into one HIP graph (no host cost between the launches),
device events around REPLAYS replays, ROUNDS rounds alternating between the two so that both see the same machine; the median round and the
spread (max - min over the rounds) are reported.  The probe's weights are compared with the float64 module at the size that is timed.

Prints its lines and one JSON line at the end (profiles/r17_bench_attention_weights.txt is this output).

    python tools/bench_attention_weights.py [agents] [rounds]"""
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from quad_swarm_rl_amd import attention, policy

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
CALLS, REPLAYS = 50, 20

CLASSES = [  # name, module
    ("attention K=6", lambda: policy.make_reference_encoder(seed=0, nbr_encoder="attention", num_nbr=6, self_dim=18, obst_dim=0)),
    ("mha K=2", lambda: policy.make_reference_mha_encoder(seed=0, num_nbr=2)),
    ("sim2real 256 K=2", lambda: policy.make_reference_sim2real_encoder(seed=0, num_nbr=2)),
    ("sim2real 16 K=6", lambda: policy.make_reference_sim2real_encoder(seed=0, hidden=16, num_nbr=6, self_dim=18)),
]


def graph_timed_us(fn):
    """us per call of fn: CALLS calls in one graph, events around REPLAYS replays"""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * CALLS)


def hooked_weights(module, obs):
    """the weights out of the torch module's own forward pass, the way the fixtures were taken (tools/capture_attention_weights.py)"""
    taken = {}
    if module.nbr_encoder == "attention":
        h = module.attention_mlp.register_forward_hook(lambda m, i, o: taken.__setitem__("w", torch.softmax(o.view(obs.shape[0], -1), dim=1)))
        module(obs)
    else:   # the restatements' attention blocks return the tokens only: the block's inputs, and the weights from its projections
        h = module.attention_layer.register_forward_hook(lambda m, i, o: taken.__setitem__("x", i[0]))
        module(obs)
        att, x = module.attention_layer, taken["x"]
        d = att.w_qs.in_features
        q, k = att.w_qs(x), att.w_ks(x)
        if q.shape[-1] != d:
            q, k = q.view(x.shape[0], 2, -1, d).transpose(1, 2), k.view(x.shape[0], 2, -1, d).transpose(1, 2)
        taken["w"] = torch.softmax(torch.matmul(q / d ** 0.5, k.transpose(-1, -2)), dim=-1)
    h.remove()
    return taken["w"]


def host_timed_us(fn, iters=50):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


res = {"agents": B, "rounds": ROUNDS, "calls_per_graph": CALLS, "replays": REPLAYS, "classes": {}}
slower = []
with torch.no_grad():
    for name, make in CLASSES:
        ref = make().cuda()
        probe, fused = attention.AttentionProbe(ref), policy.FusedQuadEncoder(ref, precision="fp32")
        obs = torch.rand((B, probe.params.obs_dim), device="cuda") * 2 - 1
        w, feats = torch.empty((B,) + probe.row_shape, device="cuda"), torch.empty((B, fused.out_dim), device="cuda")
        probe.weights(obs, out=w)          # warm-up outside any capture: scratch, LDS attributes
        fused(obs, out=feats)
        torch.cuda.synchronize()
        err = (w.double() - attention.attention_weights_reference(copy.deepcopy(ref).double(), obs.double())).abs().max().item()
        hooked = hooked_weights(ref, obs)
        err_hooked = (w - hooked).abs().max().item()
        tp, tf = [], []
        for r in range(ROUNDS):
            tp.append(graph_timed_us(lambda: probe.weights(obs, out=w)))
            tf.append(graph_timed_us(lambda: fused(obs, out=feats)))
        th = sorted(host_timed_us(lambda: hooked_weights(ref, obs)) for _ in range(3))
        mp, mf = sorted(tp)[ROUNDS // 2], sorted(tf)[ROUNDS // 2]
        spread = max(max(tp) - min(tp), max(tf) - min(tf))
        ok = mp <= mf + spread
        if not ok:
            slower.append(name)
        print(f"{name}, {B} agents, us per call over {ROUNDS} rounds of {REPLAYS} x {CALLS}:")
        print("    probe (qs_attn_weights)        " + " ".join(f"{t:8.2f}" for t in tp) + f"   median {mp:8.2f}")
        print("    forward (qs_enc_forward, fp32) " + " ".join(f"{t:8.2f}" for t in tf) + f"   median {mf:8.2f}")
        print(f"    hooked torch fp32 module, eager " + " ".join(f"{t:8.1f}" for t in th) + f"   median {th[1]:8.1f}")
        print(f"    probe / forward = {mp / mf:.3f} (spread of a round {spread:.2f} us: {'not slower' if ok else 'SLOWER than the forward pass'}), "
              f"hooked module / probe = {th[1] / mp:.1f}; |probe - module float64| = {err:.2e}, |probe - hooked fp32| = {err_hooked:.2e}")
        res["classes"][name] = {"probe_us": mp, "forward_fp32_us": mf, "round_spread_us": spread, "hooked_torch_fp32_us": th[1], "probe_over_forward": mp / mf,
                                "hooked_over_probe": th[1] / mp, "probe_not_slower_than_forward": ok, "max_abs_error_vs_float64_module": err}
res["slower_than_forward"] = slower
print(json.dumps(res))

#!/usr/bin/env python
"""The deployable Sim2Real encoder (rnn_size 16, 6 neighbours, obs 18 + 36 + 9 = 63; csrc/qs_enc_narrow.inc) at 8192 agents, one process:

  * the fused forward pass: device events around back-to-back launches (qs_enc_benchmark), several rounds so that the spread is visible.  With
    a second build of the library as the third argument the two are timed alternately in the same process and their features compared bit
    for bit - how the workgroup size was chosen (waves per workgroup are a build-time constant):
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -DENC_NW_WAVES=4 -o build_exp/libquadswarm_encoder_w4.so \\
            quad-swarm-rl_amd/csrc/qs_policy_encoder.hip
  * the fp32 torch module, eager;
  * one control step of a graphed segment (encoder + head + Gaussian sampling -> environment step) on 1024 environments x 8 drones with
    obstacles, with the narrow encoder and with the 256-wide `mean_embed` encoder on the same environments.

Prints its lines and one JSON line at the end (profiles/r16_bench_narrow_encoder.txt is this output).

    python tools/bench_narrow_encoder.py [agents] [rounds] [second library]"""
import ctypes as C
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from quad_swarm_rl_amd import abi, policy, rollout
from quad_swarm_rl_amd.env import QuadSwarmVecEnv

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
H, K = 16, 6
OTHER = sys.argv[3] if len(sys.argv) > 3 else None
libs = {"the library": policy.lib()}
if OTHER:
    libs[os.path.basename(OTHER)] = C.CDLL(OTHER)
    abi.bind(libs[os.path.basename(OTHER)], abi.QUADSWARM_ENCODER_H)

ref = policy.make_reference_sim2real_encoder(seed=0, hidden=H, num_nbr=K, self_dim=18).cuda()
fused = policy.FusedQuadEncoder(ref)
D = fused.params.obs_dim
obs = torch.rand((B, D), device="cuda") * 2 - 1
out = torch.empty((B, H), device="cuda")
macs = (18 + 6 * K + 9) * H + 2 * 3 * H * H + 2 * H * H + 2 * 2 * 2 * H + 3 * H * H      # per agent, unpadded
res = {"agents": B, "obs_dim": D, "rnn_size": H, "num_nbr": K, "algorithmic_kflop_per_agent": 2 * macs / 1e3}


def timeit(fn, iters):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def passes_us(lib, iters=10000):
    ms = C.c_double(0)
    rc = lib.qs_enc_benchmark(obs.data_ptr(), B, C.byref(fused.params), out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream), iters, C.byref(ms))
    assert rc == 0, lib.qs_enc_last_error()
    return ms.value * 1e3


with torch.no_grad():
    want64 = copy.deepcopy(ref).double()(obs.double())
    feats, times = {}, {name: [] for name in libs}
    for r in range(ROUNDS):
        for name, lib in libs.items():
            times[name].append(passes_us(lib))
            feats[name] = out.clone()
    res["fused_us"] = {}
    for name in libs:
        print(f"narrow forward, {name}: us per pass over {ROUNDS} rounds of 10000: " + " ".join(f"{t:.2f}" for t in times[name])
              + f"   median {sorted(times[name])[ROUNDS // 2]:.2f}")
        res["fused_us"][name] = sorted(times[name])[ROUNDS // 2]
        assert torch.equal(feats[name], feats["the library"]), "the workgroup size is a launch shape: same features bit for bit"
    t_fused = res["fused_us"]["the library"]
    res["max_abs_error_vs_float64_module"] = (feats["the library"].double() - want64).abs().max().item()
    res["fused_us_one_python_call_per_pass"] = timeit(lambda: fused(obs, out=out), 500) * 1e6
    t_torch = [timeit(lambda: ref(obs), 200) * 1e6 for _ in range(3)]
    res["torch_fp32_eager_us"] = sorted(t_torch)[1]
    res["torch_fp32_error_vs_float64_module"] = (ref(obs).double() - want64).abs().max().item()
    print(f"torch fp32 module, eager: us per pass {' '.join(f'{t:.1f}' for t in t_torch)}   (fused: {res['max_abs_error_vs_float64_module']:.2e} from the "
          f"float64 module, torch fp32: {res['torch_fp32_error_vs_float64_module']:.2e})")
    res["speedup_vs_torch_fp32"] = res["torch_fp32_eager_us"] / t_fused

# ---- one graphed control step: encoder + head + sampling -> step, on environments whose rows are the deployed shape ----
E, T = B // 8, 32
env = QuadSwarmVecEnv(E, seed=0, num_agents=8, neighbor_visible_num=K, neighbor_obs_type="pos_vel", use_numba=True, collision_falloff_radius=4.0,
                      use_obstacles=True, obst_density=0.2, obst_size=0.6, obst_spawn_area=(8.0, 8.0), quads_mode="o_random", obs_repr="xyz_vxyz_R_omega",
                      write_rew_info=False)
env.reset()
wide = policy.FusedQuadEncoder(policy.make_reference_encoder(seed=0, nbr_encoder="mean_embed", num_nbr=K, obst_dim=9, self_dim=18).cuda())


def control_step_us(enc, in_features):
    seg = rollout.GraphedRollout(env, enc, rollout.GaussianActionHead(in_features=in_features, sample=True), steps=T)
    for _ in range(3):
        seg.run()
    torch.cuda.synchronize()
    reps = 30
    t0 = time.perf_counter()
    for _ in range(reps):
        seg.run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * T) * 1e6


steps = {"narrow_16": [], "mean_embed_256": []}
for r in range(3):
    steps["narrow_16"].append(control_step_us(fused, H))
    steps["mean_embed_256"].append(control_step_us(wide, 512))
for name, ts in steps.items():
    print(f"graphed control step, {E} envs x 8 drones with obstacles, {name}: us per step " + " ".join(f"{t:.2f}" for t in ts))
    res[f"control_step_us_{name}"] = sorted(ts)[1]
env.close()
print(json.dumps(res))
assert t_fused < res["torch_fp32_eager_us"], "the fused pass has to beat the eager module"

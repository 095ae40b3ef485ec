#!/usr/bin/env python
"""What a value map of every agent costs (quad_swarm_rl_amd/value_map.py, include/quadswarm_valuemap.h): 8192 agents x 21 x 21 cells = 3.6 M
hypothetical rows, `mean_embed` and `attention` critics (6 neighbours, 54 columns), both precisions, in ONE process on one device, timed with
device events, medians of repeated runs after a warm-up:

  full        ValueMap(obs): expand + fused critic per 65536-row chunk, then the reduction
  expand      the expansion launches of all chunks alone (qs_value_map_expand), with the bytes they write per second next to the measured
              float4-copy rate of the device (MI355X: 6.29 TB/s) - the kernel reads almost nothing, so its traffic is half a copy's
  reduce      the reduction alone (qs_value_map_reduce)
  torch       the float32 torch module + value layer over the same rows in the same chunks (rows expanded by the same kernel, included)

Nothing is asserted; one JSON line per (encoder, precision), --out appends them to a file as well.

    python tools/bench_value_map.py --out profiles/r09_bench_value_map.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12          # bytes/s, float4 copy measured on MI355X: read + write of a streaming kernel


def timed(torch, fn, reps):
    """median, min, max over `reps` of the device time of one call of fn, in ms"""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def bench(nbr_encoder, precision, A, chunk, reps):
    import torch
    from quad_swarm_rl_amd import policy, value_map
    module = policy.make_reference_encoder(seed=3, nbr_encoder=nbr_encoder).cuda()
    torch.manual_seed(4)
    value = torch.nn.Linear(512, 1).cuda()
    critic = policy.FusedQuadEncoder(module, precision=precision)
    critic.set_head(value.weight, value.bias)
    m = value_map.ValueMap(critic, chunk_rows=chunk)
    D = critic.params.obs_dim
    obs = torch.rand((A, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 2 - 1
    lib, stream = policy.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    total = A * m.nx * m.ny
    out = m(obs)                                                      # warm-up: allocations, code objects, LDS attributes
    values = out["values"].clone()
    torch.cuda.synchronize()

    def expand_all():
        for row0 in range(0, total, chunk):
            assert lib.qs_value_map_expand(C.byref(m._P), row0, min(chunk, total - row0), stream) == 0

    def reduce_only():
        assert lib.qs_value_map_reduce(C.byref(m._P), stream) == 0

    def torch_all():
        with torch.no_grad():
            for row0 in range(0, total, chunk):
                n = min(chunk, total - row0)
                assert lib.qs_value_map_expand(C.byref(m._P), row0, n, stream) == 0
                tvalues[row0:row0 + n] = value(module(m._rows[:n]))[:, 0]

    tvalues = torch.empty(total, device="cuda")
    for fn in (expand_all, reduce_only, torch_all):
        fn()
    torch.cuda.synchronize()
    full = timed(torch, lambda: m(obs), reps)
    expand = timed(torch, expand_all, reps)
    reduce_ = timed(torch, reduce_only, reps)
    torch_ms = timed(torch, torch_all, max(3, reps // 2))
    written = total * D * 4
    line = dict(tool="bench_value_map", encoder=nbr_encoder, precision=precision, agents=A, grid=[m.nx, m.ny], rows=total, obs_dim=D, chunk_rows=chunk,
                reps=reps, full_ms=round(full[0], 3), full_ms_min_max=[round(full[1], 3), round(full[2], 3)],
                expand_ms=round(expand[0], 4), expand_ms_min_max=[round(expand[1], 4), round(expand[2], 4)], expand_launches=-(-total // chunk),
                expand_written_bytes=written, expand_written_bytes_per_s=round(written / (expand[0] * 1e-3), -9), copy_rate_bytes_per_s=COPY_RATE,
                reduce_ms=round(reduce_[0], 4), reduce_ms_min_max=[round(reduce_[1], 4), round(reduce_[2], 4)],
                torch_fp32_ms=round(torch_ms[0], 3), torch_over_full=round(torch_ms[0] / full[0], 2),
                us_per_8192_rows=round(full[0] * 1e3 * 8192 / total, 2),
                max_abs_diff_vs_torch_fp32=float((values.reshape(-1) - tvalues).abs().max()))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=8192)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--encoders", nargs="+", default=["mean_embed", "attention"])
    ap.add_argument("--precisions", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_value_map: needs a GPU (a CPU run says nothing about the device)")
    for enc in args.encoders:
        for prec in args.precisions:
            line = json.dumps(bench(enc, prec, args.agents, args.chunk, args.reps))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()

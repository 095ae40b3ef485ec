"""Test model of the value map (include/quadswarm_valuemap.h), written from the header's semantics in numpy, not from the kernels:

    rows[a * nx * ny + i * ny + j, c] = obs[a, c], except rows[r, col] = obs[a, col] + sign * off_axis[i or j] for a shift entry (col, axis, sign)
    vmax / vmin / argmax per agent as numpy's max / min / argmax answer (first index on ties, the first NaN if there is one)

and the helpers the fixtures tests/golden/value_map_<case>.npz are read with (tools/capture_value_map.py writes them from the reference's
V_ValueMapWrapper): the critic module of a case, rebuilt from its seed."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {  # name: (builder, neighbour encoder, neighbours, obstacles, obs_dim)
    "mean_embed": ("multi", "mean_embed", 6, False, 54),
    "attention_obst": ("multi", "attention", 2, True, 40),
    "none_obst": ("multi", "no_encoder", 2, True, 40),
    "mha_k6": ("mha", None, 6, True, 64),
}
DEFAULT_SHIFTS = [(0, 0, 1), (1, 1, 1)]


def offset_table(n, step):
    """float32(k * step), k * step in double, k centred on 0 (the reference: k = -10..10, step 0.2)"""
    return np.array([np.float32(float(k) * float(step)) for k in range(-(n // 2), n - n // 2)], dtype=np.float32)


def expand(obs, off_x, off_y, shifts=DEFAULT_SHIFTS):
    """obs [A, D] float32 -> rows [A * nx * ny, D] float32"""
    obs, off_x, off_y = np.asarray(obs, dtype=np.float32), np.asarray(off_x, dtype=np.float32), np.asarray(off_y, dtype=np.float32)
    A, D = obs.shape
    nx, ny = len(off_x), len(off_y)
    rows = np.repeat(obs, nx * ny, axis=0).reshape(A, nx, ny, D).copy()
    for col, axis, sign in shifts:
        off = off_x[:, None] if axis == 0 else off_y[None, :]
        rows[:, :, :, col] = obs[:, None, None, col] + np.float32(sign) * off[None]      # float32 + float32: one rounding
    return rows.reshape(A * nx * ny, D)


def reduce(values):
    """values [A, n] -> (vmax [A], vmin [A], argmax [A] int32)"""
    values = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return values.max(axis=1), values.min(axis=1), values.argmax(axis=1).astype(np.int32)


def load(case):
    return np.load(os.path.join(GOLDEN, f"value_map_{case}.npz"))


def reference_critic(case, seed):
    """(encoder module, value layer) of a case: policy.make_reference_* under the fixture's seed, then nn.Linear(out, 1) on the same
    generator - the order in which tools/capture_value_map.py creates the reference's (it asserts both carry the same weights)."""
    import torch
    from quad_swarm_rl_amd import policy
    cls, enc, K, obst, _ = CASES[case]
    if cls == "multi":
        module = policy.make_reference_encoder(seed=int(seed), nbr_encoder=enc, num_nbr=K, obst_dim=9 if obst else 0, self_dim=19 if obst else 18)
    else:
        module = policy.make_reference_mha_encoder(seed=int(seed), num_nbr=K)
    value = torch.nn.Linear(module.feed_forward[0].out_features, 1)
    return module, value


def weight_sums(module, value):
    """[sum, sum of |w|] per tensor, encoder first (sorted by name), then the value layer: the fixtures' checksum"""
    tensors = [v for _, v in sorted(module.state_dict().items())] + [value.weight.detach(), value.bias.detach()]
    return np.array([[float(v.double().sum()), float(v.double().abs().sum())] for v in tensors])

#!/usr/bin/env python
"""Golden fixtures of the reference's value map.  Build container only (imports the reference checkout at /root/reference).

The reference's V_ValueMapWrapper (swarm_rl/env_wrappers/v_value_map.py) is built over a trivial env and asked for its map:
get_v_value_map_2d overwrites columns 0 and 1 of its current observation row with init + i * 0.2, init + j * 0.2 (i, j in -10..10) and calls
model.forward once per cell.  The model here is {"values": value_layer(reference_encoder(obs))}: the REFERENCE encoder class under a fixed
seed, as oracle/ref_harness/capture_encoders.py builds it, and nn.Linear(out, 1) created next on the same generator.  The script ASSERTS
that tests/value_map_model.reference_critic (policy.make_reference_* + the same Linear) under the same seed carries the same weights bit for
bit, so the fixture needs none.  The reference's `.item()` works on a batch of one only, so the wrapper is asked once per agent with
curr_obs = [row].  plot_v_value_2d is replaced in the wrapper module's namespace by a recorder of (idx, idy, tmp_score).

Sample Factory is not installed: its modules are stubbed as in capture_encoders.py, plus sample_factory.algo.utils.rl_utils with
prepare_and_normalize_obs = float32 tensor of the observation (--normalize_input=False, the recipe's setting); plotly.express is stubbed if absent.

tests/golden/value_map_<case>.npz: seed, case shapes, obs [3, D] (uniform in [-1, 1]), values [3, 21, 21] float32 (the reference's tmp_score),
idx / idy [441], values64 [3, 21, 21] (the same module in float64 on the rows the reference built, a batch of one each), weight_sums.
Two conditions the tests rest on are checked here, and a case that misses one gets another seed (--seed-base), never a wider bound:
max |values - values64| <= 1e-5, and at most one agent over all cases whose two largest values lie within 2e-5 of each other.

Usage: python tools/capture_value_map.py [--seed-base 2200]
"""
import argparse
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "ref_harness", "stubs"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def mod(name, **kw):
    m = types.ModuleType(name)
    m.__dict__.update(kw)
    sys.modules[name] = m


for name in ("sample_factory", "sample_factory.algo", "sample_factory.algo.utils", "sample_factory.model"):
    mod(name)
mod("sample_factory.algo.utils.context", global_model_factory=lambda: None)
mod("sample_factory.algo.utils.torch_utils", calc_num_elements=lambda module, shape: module(torch.zeros(1, *shape)).numel())
mod("sample_factory.algo.utils.rl_utils", prepare_and_normalize_obs=lambda model, obs: {"obs": torch.as_tensor(obs["obs"], dtype=torch.float32)})


class _Encoder(nn.Module):   # sample_factory.model.encoder.Encoder: an nn.Module that takes cfg
    def __init__(self, cfg=None):
        super().__init__()


mod("sample_factory.model.encoder", Encoder=_Encoder)
mod("sample_factory.model.model_utils", fc_layer=lambda i, o, **k: nn.Linear(i, o), nonlinearity=lambda cfg: nn.Tanh())
if importlib.util.find_spec("plotly") is None:   # gym_art/quadrotor_multi/tests/plot_v_value_2d.py imports it at module level and never uses it here
    mod("plotly")
    mod("plotly.express")

import gymnasium                                                  # noqa: E402  (the stub)
from swarm_rl.models import quad_multi_model as ref_model        # noqa: E402
from swarm_rl.env_wrappers import v_value_map as ref_vmap        # noqa: E402
import value_map_model as vm                                      # noqa: E402
from quad_swarm_rl_amd import policy                              # noqa: E402

VALUE_TOL, ARGMAX_GAP = 1e-5, 2e-5


class TrivialEnv(gymnasium.Env):
    def reset(self, **kw):
        return None, {}


class Critic:
    """what the reference wrapper calls: forward(normalized_obs, rnn_states, values_only=True) -> {"values": ...}; keeps the rows it was given"""

    def __init__(self, encoder, value):
        self.encoder, self.value, self.rows = encoder, value, []

    def forward(self, normalized_obs, rnn_states, values_only=True):
        self.rows.append(normalized_obs["obs"].clone())
        with torch.no_grad():
            return {"values": self.value(self.encoder({"obs": normalized_obs["obs"]}))}


def capture(case, seed):
    cls, enc, K, obst, D = vm.CASES[case]
    cfg = types.SimpleNamespace(quads_obs_repr="xyz_vxyz_R_omega_floor" if obst else "xyz_vxyz_R_omega", quads_neighbor_hidden_size=256,
                                quads_use_obstacles=obst, quads_neighbor_visible_num=K, quads_num_agents=8, quads_neighbor_obs_type="pos_vel",
                                quads_obstacle_obs_type="octomap", quads_obst_hidden_size=256, quads_neighbor_encoder_type=enc, rnn_size=256)
    torch.manual_seed(seed)
    theirs = {"multi": ref_model.QuadMultiEncoder, "mha": ref_model.QuadMultiHeadAttentionEncoder}[cls](cfg, None)
    their_value = nn.Linear(512, 1)
    mine, my_value = vm.reference_critic(case, seed)
    loaded = policy.encoder_from_state_dict({"actor_critic.encoder." + k: v for k, v in theirs.state_dict().items()}, num_nbr=K)
    for (ka, va), (kb, vb) in zip(sorted(mine.state_dict().items()), sorted(loaded.state_dict().items())):
        assert ka == kb and torch.equal(va, vb), f"{case}: seed-built restatement differs from the reference weights at {ka}"
    assert torch.equal(their_value.weight, my_value.weight) and torch.equal(their_value.bias, my_value.bias), f"{case}: value layer"

    g = torch.Generator().manual_seed(seed + 1)
    obs = (torch.rand((3, D), generator=g) * 2 - 1).numpy()
    recorded = []
    ref_vmap.plot_v_value_2d = lambda idx, idy, tmp_score, width=None, height=None: recorded.append((idx, idy, tmp_score)) or tmp_score
    critic = Critic(theirs, their_value)
    wrapper = ref_vmap.V_ValueMapWrapper(TrivialEnv(), critic)
    for a in range(3):
        wrapper.curr_obs = [obs[a]]
        wrapper.get_v_value_map_2d()
    idx, idy = recorded[0][0], recorded[0][1]
    assert all(np.array_equal(r[0], idx) and np.array_equal(r[1], idy) for r in recorded)
    values = np.stack([r[2] for r in recorded]).astype(np.float32)            # .item() of float32 values: exact in float32
    assert np.array_equal(values.astype(np.float64), np.stack([r[2] for r in recorded]))
    rows = torch.cat(critic.rows)                                              # [3 * 441, D]: what the reference fed its model
    assert np.array_equal(rows.numpy(), vm.expand(obs, vm.offset_table(21, 0.2), vm.offset_table(21, 0.2))), f"{case}: the model's rows"
    enc64, val64 = copy.deepcopy(theirs).double(), copy.deepcopy(their_value).double()
    with torch.no_grad():
        values64 = torch.cat([val64(enc64({"obs": r[None].double()})) for r in rows]).reshape(3, 21, 21).numpy()
    err = float(np.abs(values - values64).max())
    top = np.sort(values64.reshape(3, -1), axis=1)
    close = int(((top[:, -1] - top[:, -2]) <= ARGMAX_GAP).sum())
    np.savez_compressed(os.path.join(vm.GOLDEN, f"value_map_{case}.npz"), seed=seed, case=case, num_nbr=K, obst_dim=9 if obst else 0,
                        self_dim=19 if obst else 18, obs=obs, values=values, idx=idx, idy=idy, values64=values64, weight_sums=vm.weight_sums(mine, my_value))
    print(f"value_map_{case}.npz: seed {seed}, obs {obs.shape}, max |fp32 reference - float64| = {err:.2e}, agents with a top-two gap <= {ARGMAX_GAP}: {close}")
    return err, close


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed-base", type=int, default=2200)
    args = ap.parse_args()
    results = [capture(case, args.seed_base + i) for i, case in enumerate(vm.CASES)]
    assert max(r[0] for r in results) <= VALUE_TOL, "a case's fp32 reference lies outside VALUE_TOL of float64: capture with another seed"
    assert sum(r[1] for r in results) <= 1, "more than one agent with a near-tie at the top: capture with another seed"


if __name__ == "__main__":
    main()

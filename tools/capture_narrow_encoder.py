#!/usr/bin/env python
"""Golden fixtures of the reference's QuadSingleHeadAttentionEncoder_Sim2Real at the widths that are deployed (--rnn_size 16 / 32).
Build container only: it needs the reference checkout that oracle/ref_harness/capture_encoders.py imports.

Like that script (whose Sample Factory stubs and import path it reuses by importing it) the reference CLASS is instantiated under a fixed torch
seed and run on a fixed observation batch.  At these sizes the fixture carries the whole state dict under the reference's key names (a few
thousand floats, keys "w:<name>"), the observations and the class's output:

    tests/golden/narrow_sim2real_h16_k6.npz   the deployed shape: rnn_size 16, 6 neighbours, xyz_vxyz_R_omega, obs 18 + 36 + 9 = 63, batch 37
    tests/golden/narrow_sim2real_h32_k2.npz   rnn_size 32, 2 neighbours, xyz_vxyz_R_omega_floor, obs 19 + 12 + 9 = 40, batch 19

(not encoder_*.npz: tests/test_encoder_fixtures.py builds everything of that name at width 256).  tests/test_narrow_fixtures.py reads them.
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "ref_harness"))
import capture_encoders as ce  # noqa: E402  (stubs the four Sample Factory imports, imports the reference's model file)

CASES = [  # name, rnn_size, neighbours, observation representation, self columns, batch
    ("h16_k6", 16, 6, "xyz_vxyz_R_omega", 18, 37),
    ("h32_k2", 32, 2, "xyz_vxyz_R_omega_floor", 19, 19),
]


def main():
    out_dir = os.path.join(REPO, "tests", "golden")
    for idx, (name, H, K, repr_, self_dim, B) in enumerate(CASES):
        seed = 2000 + idx
        cfg = types.SimpleNamespace(quads_obs_repr=repr_, quads_neighbor_hidden_size=H, quads_use_obstacles=True, quads_neighbor_visible_num=K,
                                    quads_num_agents=8, quads_neighbor_obs_type="pos_vel", quads_obstacle_obs_type="octomap", quads_obst_hidden_size=H,
                                    quads_neighbor_encoder_type=None, rnn_size=H)
        torch.manual_seed(seed)
        theirs = ce.ref_model.QuadSingleHeadAttentionEncoder_Sim2Real(cfg, None)
        with torch.no_grad():   # LayerNorm starts at (1, 0): make the affine part visible
            g = torch.Generator().manual_seed(seed + 7)
            theirs.attention_layer.layer_norm.weight.copy_(0.5 + torch.rand(H, generator=g))
            theirs.attention_layer.layer_norm.bias.copy_(-0.3 + 0.6 * torch.rand(H, generator=g))
        g = torch.Generator().manual_seed(seed + 1)
        obs = torch.rand((B, self_dim + 6 * K + 9), generator=g) * 2 - 1
        with torch.no_grad():
            want = theirs({"obs": obs})
        assert want.shape == (B, H)
        sd = {k: v.detach().numpy() for k, v in theirs.state_dict().items()}
        mine = ce.policy.encoder_from_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, num_nbr=K)
        with torch.no_grad():
            err = (mine(obs) - want).abs().max().item()
        assert err <= 1e-6, f"{name}: restatement vs reference class {err}"
        path = os.path.join(out_dir, f"narrow_sim2real_{name}.npz")
        np.savez_compressed(path, rnn_size=H, num_nbr=K, self_dim=self_dim, obst_dim=9, obs=obs.numpy(), out=want.numpy(), **{"w:" + k: v for k, v in sd.items()})
        print(f"{os.path.basename(path)}: seed {seed}, obs {tuple(obs.shape)}, {sum(v.size for v in sd.values())} weights, "
              f"max |restatement - reference class| = {err:.1e}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

"""What the two attention-weight test files share: the fixtures of tools/capture_attention_weights.py (tests/golden/attnw_<case>.npz) and the
restatement module each one describes.  No test in here."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("attnw_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "attnw_*.npz")))
EXPECTED = {"attention_k6": ("multi", 256, 6, 0, 37), "attention_k2_obst": ("multi", 256, 2, 9, 19), "mha_k6": ("mha", 256, 6, 9, 21),
            "sim2real_k2": ("s2r", 256, 2, 9, 21), "sim2real_h16_k6": ("s2r", 16, 6, 9, 37)}   # class, rnn_size, neighbours, obstacle columns, batch
RESTATEMENT_TOL = 1e-6    # tests/test_encoder_fixtures.py: restatement vs reference class
ROW_SUM_TOL = 1e-6


def load(case):
    """(fixture, restatement module carrying the reference class's weights): from the seed at width 256 (the fixture's checksums prove the seed
    reproduces them), from the state dict the narrow fixture carries"""
    import torch
    from quad_swarm_rl_amd import policy
    g = np.load(os.path.join(GOLDEN, f"attnw_{case}.npz"))
    seed, K, cls = int(g["seed"]), int(g["num_nbr"]), str(g["cls"])
    if int(g["rnn_size"]) != policy.HIDDEN:
        sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
        return g, policy.encoder_from_state_dict(sd, num_nbr=K)
    if cls == "multi":
        return g, policy.make_reference_encoder(seed=seed, nbr_encoder="attention", num_nbr=K, obst_dim=int(g["obst_dim"]), self_dim=int(g["self_dim"]))
    return g, (policy.make_reference_mha_encoder if cls == "mha" else policy.make_reference_sim2real_encoder)(seed=seed, num_nbr=K)


def row_sum_error(w):
    """max |sum over the keys - 1| of float32 weights (numpy), summed in float64"""
    return float(np.abs(np.asarray(w, dtype=np.float64).sum(axis=-1) - 1.0).max())

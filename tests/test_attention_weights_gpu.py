"""The attention probe on the GPU (include/quadswarm_attention.h, csrc/qs_attn_weights.inc, quad_swarm_rl_amd/attention.py): the weights against
the torch module in float64, the reference classes' own weights (tests/golden/attnw_*.npz), and the launch rules - nothing behind row B, rows that
sum to 1, run-to-run identity, HIP-graph capture, refresh(), and a forward pass that is not disturbed by a probe on its scratch.

Shapes.  attention: 16 agents per workgroup, the K slots in groups of ENC_ANH = 3 row tiles - B = 1, 15, 16, 17, 37 are a single row, a tile less
one, a full tile, a one-row second workgroup and three workgroups with a partial last tile; K = 1, 3, 4, 7, 8 are one partial group, one full
group, a full group and a one-slot tail, two groups and a tail, and the maximum; every B < 16 K makes the (a*K + k) mod B pairing wrap.  The
multi-head classes: B = 1, 17, 37 with one and two K-steps of neighbour columns (K = 2, 6).  Narrow: every width, one wave per 16 agents.

Bound: 1e-5 absolute, the project's bound for reference-precision features (tests/test_policy_encoder_gpu.py REFERENCE_PRECISION_TOL).  Weights
are scaled as that file scales each class, so that the softmaxes are far from uniform.  With QS_ATTN_ERRORS_FILE=<path> in the environment the
worst errors per class - the kernel's, and torch's own fp32 forward on the same cases, both against float64 - are written there when the module
is done (profiles/r17_attention_weights_errors.txt is that file from an MI355X)."""
import copy
import os

import numpy as np
import pytest

from tests import attention_weights_cases as awc

pytestmark = pytest.mark.gpu

TOL = 1e-5
ATT_B, ATT_K = (1, 15, 16, 17, 37), (1, 3, 4, 7, 8)
MHA_B, MHA_K = (1, 17, 37), (2, 6)
NARROW_H = (16, 32, 64)

_built = {}
RECORD = {}     # class -> [cases, worst |kernel - float64|, worst |torch fp32 - float64|]


def built(kind, K, H=256, self_dim=19):
    """(fp32 module on the GPU, its float64 copy, AttentionProbe), once per shape"""
    import torch
    from quad_swarm_rl_amd import attention, policy
    key = (kind, K, H, self_dim)
    if key not in _built:
        if kind == "attention":
            ref = policy.make_reference_encoder(seed=3, nbr_encoder="attention", num_nbr=K, self_dim=18, obst_dim=0).cuda()
            with torch.no_grad():
                for p in ref.parameters():
                    p.mul_(2.5)
                ref.attention_mlp[4].weight.mul_(4.0)   # spread the scores so that the softmax is far from uniform
        else:
            make = policy.make_reference_mha_encoder if kind == "mha" else policy.make_reference_sim2real_encoder
            ref = make(seed=11, hidden=H, num_nbr=K, self_dim=self_dim).cuda()
            with torch.no_grad():
                for p in ref.parameters():
                    p.mul_(2.0)
                ref.attention_layer.w_qs.weight.mul_(1.5)   # scores of a few units: the 2-way softmax weights spread over 0.04 .. 0.96
        _built[key] = (ref, copy.deepcopy(ref).double(), attention.AttentionProbe(ref))
    return _built[key]


def observations(B, D, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((B, D), device="cuda", generator=g) * 2 - 1


def check_parity(label, ref, ref64, probe, obs):
    """probe vs float64 module under TOL (and vs the fp32 module), sentinel rows behind B, row sums, a second call bit-identical"""
    import torch
    from quad_swarm_rl_amd import attention
    B = obs.shape[0]
    out = torch.full((B + 3,) + probe.row_shape, 7.0, device="cuda")
    got = probe.weights(obs, out=out[:B]).clone()
    again = probe.weights(obs)
    torch.cuda.synchronize()
    want64, want32 = attention.attention_weights_reference(ref64, obs.double()), attention.attention_weights_reference(ref, obs)
    e64, e32 = (got.double() - want64).abs().max().item(), (got - want32).abs().max().item()
    t32 = (want32.double() - want64).abs().max().item()
    rs = awc.row_sum_error(got.cpu().numpy())
    print(f"\n{label} B={B}: |probe - module64| = {e64:.3e}, |probe - module32| = {e32:.3e}, |module32 - module64| = {t32:.3e}, row sums off by {rs:.2e}, "
          f"weights in [{got.min().item():.4f}, {got.max().item():.4f}]")
    rec = RECORD.setdefault(label.split()[0], [0, 0.0, 0.0])
    rec[0], rec[1], rec[2] = rec[0] + 1, max(rec[1], e64), max(rec[2], t32)
    assert tuple(got.shape) == (B,) + probe.row_shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    assert bool((out[B:] == 7.0).all())                      # rows >= B are never written
    assert torch.equal(got, again)
    assert rs <= awc.ROW_SUM_TOL
    assert e64 <= TOL and e32 <= TOL, (e64, e32)
    return got


@pytest.fixture(scope="module", autouse=True)
def error_record():
    yield
    path = os.environ.get("QS_ATTN_ERRORS_FILE")
    if path and RECORD:
        with open(path, "w") as f:
            f.write("attention weights, worst absolute error per encoder class over the parity cases of tests/test_attention_weights_gpu.py (bound 1e-5)\n")
            f.write(f"{'class':<12} {'cases':>5} {'|probe - module float64|':>26} {'|torch fp32 module - float64|':>30}\n")
            for cls in sorted(RECORD):
                n, e, t = RECORD[cls]
                f.write(f"{cls:<12} {n:>5} {e:>26.3e} {t:>30.3e}\n")


@pytest.mark.parametrize("B", ATT_B)
@pytest.mark.parametrize("K", ATT_K)
def test_attention_neighbour_encoder(K, B):
    ref, ref64, probe = built("attention", K)
    assert probe.row_shape == (K,) and probe.params.obs_dim == 18 + 6 * K
    got = check_parity(f"attention K={K}", ref, ref64, probe, observations(B, 18 + 6 * K, 100 * K + B))
    if K > 1 and B > 1:
        assert (got.max(dim=1).values - got.min(dim=1).values).max().item() > 0.05      # not the uniform softmax


def test_attention_weights_depend_on_the_batch_as_the_modules_do():
    """the (a*K + k) mod B pairing is part of the function: the first 16 rows of a batch of 37 are not the weights of those 16 rows alone, and the
    module says the same"""
    import torch
    from quad_swarm_rl_amd import attention
    ref, ref64, probe = built("attention", 3)
    obs = observations(37, 36, 9)
    whole, part = probe.weights(obs)[:16].clone(), probe.weights(obs[:16].contiguous()).clone()
    torch.cuda.synchronize()
    assert (whole - part).abs().max().item() > 1e-3
    assert (part.double() - attention.attention_weights_reference(ref64, obs[:16].double())).abs().max().item() <= TOL


@pytest.mark.parametrize("B", MHA_B)
@pytest.mark.parametrize("K", MHA_K)
@pytest.mark.parametrize("kind", ["mha", "sim2real"])
def test_multi_head_classes(kind, K, B):
    ref, ref64, probe = built(kind, K)
    assert probe.row_shape == ((4, 2, 2) if kind == "mha" else (2, 2))
    got = check_parity(f"{kind} K={K}", ref, ref64, probe, observations(B, 19 + 6 * K + 9, 1000 + 10 * K + B))
    if kind == "mha" and B > 1:
        assert (got[:, 0] - got[:, 3]).abs().max().item() > 1e-3                         # the heads are not copies of one another


@pytest.mark.parametrize("B", MHA_B)
@pytest.mark.parametrize("H", NARROW_H)
def test_narrow_sim2real(H, B):
    ref, ref64, probe = built("sim2real", 6, H=H, self_dim=18)                           # the deployed row: 18 + 36 + 9 = 63 floats
    assert probe.row_shape == (2, 2) and probe.params.n1.M == H and probe.params.obs_dim == 63
    check_parity(f"narrow H={H}", ref, ref64, probe, observations(B, 63, 7 * H + B))


@pytest.mark.parametrize("case", sorted(awc.EXPECTED))
def test_fixtures_through_the_kernel(case):
    """the reference classes' own weights (forward hooks, tools/capture_attention_weights.py), at the same bound"""
    import torch
    from quad_swarm_rl_amd import attention
    g, m = awc.load(case)
    probe = attention.AttentionProbe(m.cuda())
    got = probe.weights(torch.from_numpy(g["obs"]).cuda().contiguous()).cpu().numpy()
    err = float(np.abs(got - g["weights"]).max())
    print(f"\n{case}: max |probe - reference class| = {err:.3e}, row sums off by {awc.row_sum_error(got):.2e}")
    assert got.shape == g["weights"].shape and err <= TOL and awc.row_sum_error(got) <= awc.ROW_SUM_TOL


@pytest.mark.parametrize("shape", [("attention", 7, 256), ("mha", 2, 256), ("sim2real", 2, 256), ("sim2real", 6, 16)], ids=lambda s: f"{s[0]}-K{s[1]}-H{s[2]}")
def test_a_batch_larger_than_the_chip_is_run_to_run_identical(shape):
    """16 * 256 + 5 agents: more workgroups than CUs, a partial last tile"""
    import torch
    kind, K, H = shape
    _, _, probe = built(kind, K, H=H, self_dim=18 if H != 256 else 19)
    obs = observations(16 * 256 + 5, probe.params.obs_dim, 5)
    a = probe.weights(obs).clone()
    b = probe.weights(obs)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b) and awc.row_sum_error(a.cpu().numpy()) <= awc.ROW_SUM_TOL
    if kind != "attention":                                  # these classes treat every row on its own
        assert torch.equal(a[:100], probe.weights(obs[:100].contiguous()))


@pytest.mark.parametrize("shape", [("attention", 4, 256), ("mha", 6, 256), ("sim2real", 6, 32)], ids=lambda s: f"{s[0]}-K{s[1]}-H{s[2]}")
def test_a_captured_call_replays_on_new_observations(shape):
    import torch
    kind, K, H = shape
    _, _, probe = built(kind, K, H=H, self_dim=18 if H != 256 else 19)
    B, D = 37, probe.params.obs_dim
    obs_a, obs_b = observations(B, D, 21), observations(B, D, 22)
    static_obs, static_out = obs_a.clone(), torch.zeros((B,) + probe.row_shape, device="cuda")
    probe.weights(static_obs, out=static_out)                # outside the capture: scratch allocated, LDS attributes set
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        probe.weights(static_obs, out=static_out)
    static_obs.copy_(obs_b)
    graph.replay()
    torch.cuda.synchronize()
    replayed = static_out.clone()
    eager = probe.weights(obs_b)
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager) and not torch.equal(replayed, probe.weights(obs_a))


@pytest.mark.parametrize("shape", [("attention", 3, 256), ("mha", 2, 256), ("sim2real", 6, 16)], ids=lambda s: f"{s[0]}-K{s[1]}-H{s[2]}")
def test_refresh_follows_the_module(shape):
    import torch
    from quad_swarm_rl_amd import attention
    kind, K, H = shape
    ref = copy.deepcopy(built(kind, K, H=H, self_dim=18 if H != 256 else 19)[0])
    probe = attention.AttentionProbe(ref)
    obs = observations(33, probe.params.obs_dim, 9)
    before = probe.weights(obs).clone()
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(23)
        for p in ref.parameters():
            p.add_(torch.randn(p.shape, device="cuda", generator=g) * 0.05)
    stale = probe.weights(obs).clone()
    probe.refresh()
    after = probe.weights(obs)
    torch.cuda.synchronize()
    want = attention.attention_weights_reference(copy.deepcopy(ref).double(), obs.double())
    assert torch.equal(stale, before)                        # the probe holds its own packed copy until it is told
    assert (after.double() - want).abs().max().item() <= TOL and (after - before).abs().max().item() > 1e-3


def test_the_forward_pass_is_not_disturbed_by_a_probe_on_its_scratch():
    """FusedQuadEncoder.forward before and after a probe call that uses the encoder's own ebuf / gbuf: identical bits (a forward pass fills the
    scratch again before it reads it), and the probe's weights are those of a probe with buffers of its own"""
    import torch
    from quad_swarm_rl_amd import attention, policy
    ref, _, own = built("attention", 6)
    fused = policy.FusedQuadEncoder(ref, precision="fp32")
    probe = attention.AttentionProbe(ref, scratch=fused)
    obs = observations(37, 54, 31)
    before = fused(obs).clone()
    w = probe.weights(obs).clone()
    assert probe.params.ebuf == fused.params.ebuf and probe.params.gbuf == fused.params.gbuf and fused.params.ebuf
    after = fused(obs).clone()
    w2 = probe.weights(obs)
    torch.cuda.synchronize()
    assert torch.equal(before, after) and torch.equal(w, w2) and torch.equal(w, own.weights(obs))
    with pytest.raises(ValueError):
        attention.AttentionProbe(ref, scratch=policy.FusedQuadEncoder(ref, precision="bf16"))

"""The Sim2Real encoder's narrow kernels (csrc/qs_enc_narrow.inc; rnn_size 16, 32, 64) on the GPU: features against the torch module, run-to-run
identity, and the three fused epilogues - linear head, Gaussian sampling, trajectory copy - with the checks tests/test_encoder_epilogues_gpu.py
makes for the 256-wide kernels (its sampler model and sentinel-framed buffers are imported from there).

Shapes: one wave owns 16 agents, so B = 1, 16, 17 are a single row, a full tile and a one-row tail in a second wave; B = 100 is more than one
four-wave workgroup with a partial last tile.  K = 1, 2, 6 give the neighbour embedding one or two K-steps (6, 12, 36 columns); self_dim 18 at
K = 6 is the deployed row of 63 floats - no row but the first 16-byte aligned."""
import copy
import ctypes as C

import pytest

from tests import encoder_epilogue_cases as cases
from tests import test_encoder_epilogues_gpu as epi

pytestmark = pytest.mark.gpu

TOL = 1e-5        # the project's bound for the reference-precision kernels (tests/test_policy_encoder_gpu.py REFERENCE_PRECISION_TOL)
WIDTHS = (16, 32, 64)
SHAPES = [(1, 19), (2, 19), (6, 19), (6, 18)]          # (neighbours, self columns)
BATCHES = (1, 16, 17, 100)

_built = {}


def built(H, K, self_dim=19):
    """(fp32 module on the GPU, its float64 copy, FusedQuadEncoder), built once per shape; weights scaled as tests/test_policy_encoder_gpu.py
    scales this class (tanh layers out of their linear regime, softmax weights spread, LayerNorm's affine part visible)"""
    import torch
    from quad_swarm_rl_amd import policy
    key = (H, K, self_dim)
    if key not in _built:
        ref = policy.make_reference_sim2real_encoder(seed=11, hidden=H, num_nbr=K, self_dim=self_dim).cuda()
        with torch.no_grad():
            for p in ref.parameters():
                p.mul_(2.0)
            a = ref.attention_layer
            a.w_qs.weight.mul_(1.5)
            g = torch.Generator(device="cuda").manual_seed(17)
            a.layer_norm.weight.copy_(torch.rand(a.layer_norm.weight.shape, device="cuda", generator=g) + 0.5)
            a.layer_norm.bias.copy_(torch.rand(a.layer_norm.bias.shape, device="cuda", generator=g) * 0.6 - 0.3)
        fused = policy.FusedQuadEncoder(ref, precision="bf16")     # for a narrow module the argument is an upper bound on the error
        assert fused.params.nbr_encoder == cases.S2R and fused.params.precision == 1 and fused.precision == "fp32" and fused.out_dim == H
        assert not hasattr(fused, "_ebuf") and not fused.params.ebuf and not fused.params.gbuf
        _built[key] = (ref, copy.deepcopy(ref).double(), fused)
    return _built[key]


def observations(B, D, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((B, D), device="cuda", generator=g) * 2 - 1


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"K{s[0]}-self{s[1]}")
@pytest.mark.parametrize("H", WIDTHS)
def test_features_match_the_module(H, shape, B):
    import torch
    K, self_dim = shape
    ref, ref64, fused = built(H, K, self_dim)
    obs = observations(B, fused.params.obs_dim, 1000 * H + 10 * K + B)
    assert obs.shape[1] == self_dim + 6 * K + 9
    out = torch.full((B + 3, H), 7.0, device="cuda")
    got = fused(obs, out=out[:B]).clone()
    again = fused(obs)
    torch.cuda.synchronize()
    with torch.no_grad():
        want64, want32 = ref64(obs.double()), ref(obs)
    e64, e32 = (got.double() - want64).abs().max().item(), (got - want32).abs().max().item()
    print(f"narrow H={H} K={K} self={self_dim} B={B}: |fused - module64| = {e64:.3e}, |fused - module32| = {e32:.3e}, "
          f"|module32 - module64| = {(want32.double() - want64).abs().max().item():.3e}")
    assert got.shape == (B, H) and torch.isfinite(got).all()
    assert bool((out[B:] == 7.0).all())                      # nothing behind the batch's rows
    assert torch.equal(got, again)
    assert e64 <= TOL and e32 <= TOL, (e64, e32)


def test_a_grid_larger_than_the_chip_is_run_to_run_identical():
    """16401 agents = 1026 tiles: more workgroups than CUs at either workgroup size, a one-row tail; the rows do not depend on the batch"""
    import torch
    _, _, fused = built(16, 6, 18)
    obs = observations(16401, 63, 5)
    a, b = fused(obs), fused(obs)
    small = fused(obs[:100].contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(a[:100], small)


@pytest.mark.parametrize("hd", [1, 4])
@pytest.mark.parametrize("H", WIDTHS)
def test_head_sampling_and_trajectory_copy_in_one_pass(H, hd):
    """all three epilogues in ONE pass over B = 17 agents (a one-row second tile), each output framed by sentinel rows; then the head alone,
    with and without a feature tensor"""
    import torch
    from quad_swarm_rl_amd import policy
    B, K = 17, 2
    _, ref64, fused = built(H, K)
    g = torch.Generator(device="cuda").manual_seed(100 * H + hd)
    obs = observations(B, fused.params.obs_dim, 31 * H + hd)
    W = torch.randn((hd, H), device="cuda", generator=g) * 0.1
    b = torch.randn((hd,), device="cuda", generator=g)
    seed, counter0, step = 0x9E3779B97F4A7C15 ^ (H * 0x10001 + hd), 1000 + H + hd, 3
    sigma = cases.SIGMAS[:hd]
    log_std = torch.log(torch.tensor(sigma, device="cuda"))
    counter = torch.tensor([counter0], device="cuda", dtype=torch.int32)
    fused.set_head(W, b)
    full, again, head_only, no_feats = (epi.Pass(fused, B, hd, g) for _ in range(4))
    again.rew_src, again.done_src = full.rew_src, full.done_src
    for p in (full, again):
        fused.forward_head(obs, head_out=p.head[:B], features=p.feats[:B], sample=(log_std, p.act[:B], counter, step, seed),
                           traj=(p.rew_src, p.rew_dst[:B], p.done_src, p.done_dst[:B]))
    fused.forward_head(obs, head_out=head_only.head[:B], features=head_only.feats[:B])
    fused.forward_head(obs, head_out=no_feats.head[:B])               # out == NULL: the poisoned feature buffer next to it stays poisoned
    plain = fused(obs).clone()
    torch.cuda.synchronize()
    feats, head, act = full.feats[:B], full.head[:B], full.act[:B]
    assert torch.isfinite(feats).all() and torch.isfinite(head).all() and torch.isfinite(act).all()
    assert all(p.sentinels_intact() for p in (full, again, head_only, no_feats))
    assert torch.equal(head_only.feats[:B], feats) and torch.equal(plain, feats)
    assert torch.equal(head_only.head[:B], head) and torch.equal(no_feats.head[:B], head)
    assert bool((no_feats.feats == epi.SENT).all())
    for p in (head_only, no_feats):
        assert bool((p.act == epi.SENT).all()) and bool((p.rew_dst == epi.SENT).all()) and bool((p.done_dst == epi.SENT_BYTE).all())
    for x, y in zip(full.outputs(), again.outputs()):
        assert torch.equal(x, y)
    assert int(counter.item()) == counter0
    # head: Linear on the features the kernel wrote, and end to end against the float64 module
    err = (head.double() - (feats.double() @ W.double().T + b.double())).abs().max().item()
    with torch.no_grad():
        e64 = (head.double() - (ref64(obs.double()) @ W.double().T + b.double())).abs()
    print(f"narrow head H={H} h={hd}: |head_out - Linear64(features)| = {err:.3e}, |head_out - module64| = {e64.max().item():.3e}")
    assert err <= TOL, err
    assert (e64 <= (TOL * W.double().abs().sum(dim=1) + TOL)[None, :]).all()
    # sampler: the model's draws, under the bound of the 256-wide kernels
    epi.check_sampler("epilogue, narrow Sim2Real", f"H{H}-h{hd}", act, head, sigma, seed & 0xFFFFFFFFFFFFFFFF, counter0, step)
    if hd == 4:   # ... and what qs_rollout_pre draws from the same means at the summed counter value, bit for bit
        act2 = torch.empty((B, 4), device="cuda")
        summed = torch.tensor([counter0 + step], device="cuda", dtype=torch.int32)
        rc = policy.lib().qs_rollout_pre(None, None, 0, C.c_void_p(head.contiguous().data_ptr()), C.c_void_p(log_std.data_ptr()), C.c_void_p(act2.data_ptr()), B,
                                         C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), C.c_void_p(summed.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        print(f"narrow sampler H={H}: max |act_out - qs_rollout_pre| = {(act - act2).abs().max().item():.3e}")
        assert torch.equal(act, act2)
        assert (act - head).abs().max().item() > 0.1
    # trajectory copy
    assert torch.equal(full.rew_dst[:B], full.rew_src) and torch.equal(full.done_dst[:B], full.done_src)


def test_refresh_picks_up_the_modules_new_weights():
    import torch
    from quad_swarm_rl_amd import policy
    ref = copy.deepcopy(built(16, 6, 18)[0])
    fused = policy.FusedQuadEncoder(ref)
    obs = observations(33, 63, 9)
    W = torch.randn((1, 16), device="cuda") * 0.1
    bias = torch.zeros(1, device="cuda")
    fused.set_head(W, bias)
    before, head_before = fused(obs).clone(), fused.forward_head(obs).clone()
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(23)
        for p in ref.parameters():
            p.add_(torch.randn(p.shape, device="cuda", generator=g) * 0.05)
        W.mul_(-2.0)
    fused.refresh()
    after, head_after = fused(obs), fused.forward_head(obs)
    torch.cuda.synchronize()
    with torch.no_grad():
        want = copy.deepcopy(ref).double()(obs.double())
    assert (after.double() - want).abs().max().item() <= TOL
    assert (after - before).abs().max().item() > 1e-3
    assert (head_after.double() - (after.double() @ W.double().T + bias.double())).abs().max().item() <= TOL
    assert (head_after - head_before).abs().max().item() > 1e-3


def test_narrow_modules_take_one_kernel_whatever_precision_is_asked():
    import torch
    from quad_swarm_rl_amd import policy
    ref, _, fused = built(32, 2)
    other = policy.FusedQuadEncoder(ref, precision="fp32")
    obs = observations(17, fused.params.obs_dim, 3)
    assert other.precision == fused.precision == "fp32" and torch.equal(other(obs), fused(obs))

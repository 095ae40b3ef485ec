"""What sits behind the policy encoder's features, on every kernel of its table (tests/encoder_epilogue_cases.py: 23 configurations that
tests/test_sampler_model_cpu.py shows to select all 25 kernels): the linear head fused into the last kernel's epilogue, the Gaussian sampling
behind it, the reward / done trajectory copy on the first kernel - each against a model that shares no code with the library
(tests/sampler_model.py, float64 matrix products) and all three in ONE forward pass, so that one duty overwriting another's scratch or output
shows.  Then the two glue launches qs_rollout_pre / qs_rollout_post by themselves, and the closed loop: every action of three replays of a
captured segment is the model's draw at (seed, counter, agent), so no (counter, agent) pair is drawn twice.

QS_SAMPLER_REPORT=<path>: the worst sampler error per kernel family (see SAMPLER_Z_TOL) is also written there as JSON."""
import contextlib
import copy
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_model as sm  # noqa: E402
from tests import encoder_epilogue_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

HEAD_TOL = 1e-4                     # tests/test_policy_encoder_gpu.py::test_fused_linear_head, same scale of W
REFERENCE_PRECISION_TOL = 1e-5      # tests/test_policy_encoder_gpu.py: features of the reference-precision kernels against the module in float64
# The sampler's bound is sm.bound(head_out, sigma, z_model, SAMPLER_Z_TOL) = sigma * SAMPLER_Z_TOL + 2^-23 (|head_out| + sigma |z_model|).  The second
# term is derived (rounding of the product and of the final add).  SAMPLER_Z_TOL covers z itself as float32 with the fast log / sincos / exp
# intrinsics: 4 x the worst (|act - want| - derived term) / sigma the kernels show against the float64 model over every case of this file on an
# MI355X - MEASURED_WORST_Z, profiles/r11_sampler_z_tol.txt: 1.588e-6 in qs_rollout_pre at 524291 agents; the encoders' epilogues 1.31e-6 (16-agent
# kernels), 1.50e-6 (32-agent), 0.90e-6 (reference precision), the replayed segments 1.03e-6.  The factor 4: the 1e5 - 1e6 draws of these cases
# do not reach the far tail of ua, where dr/du is largest.  Not a measurement but a condition: the constant may not exceed SAMPLER_Z_TOL_CAP, and
# every mutant of the model stays above the bound at that cap (tests/test_sampler_model_cpu.py).
SAMPLER_Z_TOL_CAP = 1e-4
MEASURED_WORST_Z = 1.589e-6
SAMPLER_Z_TOL = 4 * MEASURED_WORST_Z    # 6.356e-6

SENT, SENT_BYTE = 7.0, 0xA5
PAD = cases.SENTINEL_ROWS

_worst = {}     # kernel family -> (worst (|act - want| - derived term) / sigma, where)


@pytest.fixture(scope="module", autouse=True)
def sampler_report():
    yield
    for family, (x, where) in sorted(_worst.items()):
        print(f"\nsampler, {family}: worst (|act - want| - derived term) / sigma = {x:.3e} at {where}; SAMPLER_Z_TOL = {SAMPLER_Z_TOL:.3e}")
    path = os.environ.get("QS_SAMPLER_REPORT")
    if path and _worst:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump({k: {"worst_z_error": v[0], "where": v[1]} for k, v in sorted(_worst.items())}, f, indent=1)


def check_sampler(family, where, act, head, sigma, seed, counter, step):
    """act [B, h] float32 against head + sigma * z_model: records the z error of the family, then asserts the bound"""
    act, head = act.detach().cpu().double().numpy(), head.detach().cpu().double().numpy()
    sigma = np.asarray(sigma, dtype=np.float64)[None, :]
    assert np.abs(head).max() <= cases.HEAD_ABS_MAX                 # (what the CPU test of the mutants assumes about the means)
    z = sm.normals(seed, counter, step, act.shape[0], act.shape[1])
    err = np.abs(act - (head + sigma * z))
    zerr = float(((err - sm.bound(head, sigma, z, 0.0)) / sigma).max())
    if family not in _worst or zerr > _worst[family][0]:
        _worst[family] = (zerr, where)
    print(f"sampler {family} {where}: worst z error {zerr:.3e}")
    allowed = sm.bound(head, sigma, z, SAMPLER_Z_TOL)
    at = np.unravel_index(int(np.argmax(err / allowed)), err.shape)
    assert (err <= allowed).all(), f"{where}: |act - model| = {err[at]:.3e} > {allowed[at]:.3e} at (agent, component) {at}; z error / sigma {zerr:.3e}"


_built = {}


def built(c):
    """(torch module, its float64 copy, FusedQuadEncoder) of a configuration, built once"""
    import torch
    from quad_swarm_rl_amd import policy
    if c.name not in _built:
        kw = dict(seed=3, num_nbr=c.num_nbr, obst_dim=c.obst_dim)
        if c.model in (cases.MHA, cases.S2R):
            ref = (policy.make_reference_sim2real_encoder if c.model == cases.S2R else policy.make_reference_mha_encoder)(**kw).cuda()
            with torch.no_grad():   # as tests/test_policy_encoder_gpu.py scales these two
                for p in ref.parameters():
                    p.mul_(2.0)
                a = ref.attention_layer
                a.w_qs.weight.mul_(1.5)
                g = torch.Generator(device="cuda").manual_seed(17)
                a.layer_norm.weight.copy_(torch.rand(a.layer_norm.weight.shape, device="cuda", generator=g) + 0.5)
                a.layer_norm.bias.copy_(torch.rand(a.layer_norm.bias.shape, device="cuda", generator=g) * 0.6 - 0.3)
        else:
            ref = policy.make_reference_encoder(nbr_encoder=policy.NBR_ENCODERS[c.model], **kw).cuda()
            with torch.no_grad():   # away from the linear regime of the tanh layers
                for p in ref.parameters():
                    p.mul_(2.5)
        fused = policy.FusedQuadEncoder(ref, precision="fp32" if c.precision else "bf16")
        assert fused.params.nbr_encoder == c.model and fused.params.precision == c.precision
        _built[c.name] = (ref, copy.deepcopy(ref).double(), fused)
    return _built[c.name]


@contextlib.contextmanager
def selection(c):
    """the process-wide switches that make enc_select pick the configuration's kernels at every batch size"""
    from quad_swarm_rl_amd import policy
    L = policy.lib()
    prev_wide, prev_pp = L.qs_enc_set_wide_min(1 if c.wide else 0), L.qs_enc_set_pingpong(c.pingpong)
    try:
        yield
    finally:
        L.qs_enc_set_wide_min(prev_wide)
        L.qs_enc_set_pingpong(prev_pp)


def family_of(c):
    return "epilogue, reference precision (16 agents)" if c.precision else "epilogue, 32-agent kernels" if c.wide else "epilogue, 16-agent kernels"


class Pass:
    """the buffers of one forward pass, every output with PAD sentinel rows behind its B rows"""

    def __init__(self, fused, B, hd, gen):
        import torch
        R, dev = B + PAD, "cuda"
        self.B = B
        self.feats, self.head, self.act = (torch.full((R, n), SENT, device=dev) for n in (fused.out_dim, hd, hd))
        self.rew_dst = torch.full((R,), SENT, device=dev)
        self.done_dst = torch.full((R,), SENT_BYTE, device=dev, dtype=torch.uint8)
        self.rew_src = torch.randn((B,), device=dev, generator=gen) * 10.0
        self.done_src = torch.randint(0, 256, (B,), device=dev, generator=gen, dtype=torch.uint8)     # arbitrary bytes, not only 0 / 1

    def outputs(self):
        return (self.feats, self.head, self.act, self.rew_dst, self.done_dst)

    def sentinels_intact(self):
        B = self.B
        return all(bool((x[B:] == (SENT_BYTE if x is self.done_dst else SENT)).all()) for x in self.outputs())


def case_inputs(c, i, j, B, hd):
    import torch
    ref, ref64, fused = built(c)
    g = torch.Generator(device="cuda").manual_seed(1000 * i + j)
    D = fused.params.obs_dim
    obs = (torch.rand((B, D), device="cuda", generator=g) * 2 - 1) * torch.tensor([3.0] * 3 + [1.0] * (D - 3), device="cuda")
    W = torch.randn((hd, fused.out_dim), device="cuda", generator=g) * 0.1
    b = torch.randn((hd,), device="cuda", generator=g)
    return ref64, fused, g, obs, W, b


MATRIX = [(i, j) for i in range(len(cases.CONFIGS)) for j in range(len(cases.SHAPES))] + \
         [([c.name for c in cases.CONFIGS].index(name), len(cases.SHAPES)) for name in cases.TAIL_CONFIGS]


def _id(ij):
    B, hd = (cases.SHAPES + [cases.TAIL_SHAPE])[ij[1]]
    return f"{cases.CONFIGS[ij[0]].name}-B{B}-h{hd}"


@pytest.mark.parametrize("ij", MATRIX, ids=_id)
def test_head_sampling_and_trajectory_copy_in_one_pass(ij):
    import torch
    i, j = ij
    c = cases.CONFIGS[i]
    B, hd = (cases.SHAPES + [cases.TAIL_SHAPE])[j]
    ref64, fused, g, obs, W, b = case_inputs(c, i, j, B, hd)
    seed, counter0, step = cases.sampler_inputs_of(i, j)
    sigma = cases.SIGMAS[:hd]
    log_std = torch.log(torch.tensor(sigma, device="cuda"))
    counter = torch.tensor([counter0], device="cuda", dtype=torch.int32)
    fused.set_head(W, b)
    full, again, head_only = Pass(fused, B, hd, g), Pass(fused, B, hd, g), Pass(fused, B, hd, g)
    again.rew_src, again.done_src = full.rew_src, full.done_src
    with selection(c):
        for p in (full, again):
            fused.forward_head(obs, head_out=p.head[:B], features=p.feats[:B], sample=(log_std, p.act[:B], counter, step, seed),
                               traj=(p.rew_src, p.rew_dst[:B], p.done_src, p.done_dst[:B]))
        fused.forward_head(obs, head_out=head_only.head[:B], features=head_only.feats[:B])
        no_feats = fused.forward_head(obs).clone()                       # head without the feature tensor
        plain = fused(obs).clone()
    torch.cuda.synchronize()
    feats, head, act = full.feats[:B], full.head[:B], full.act[:B]
    assert torch.isfinite(feats).all() and torch.isfinite(head).all() and torch.isfinite(act).all()
    # untouched by one another
    assert full.sentinels_intact() and again.sentinels_intact() and head_only.sentinels_intact()
    assert torch.equal(head_only.feats[:B], feats) and torch.equal(plain, feats)
    assert torch.equal(head_only.head[:B], head) and torch.equal(no_feats, head)
    assert bool((head_only.act == SENT).all()) and bool((head_only.rew_dst == SENT).all()) and bool((head_only.done_dst == SENT_BYTE).all())
    for x, y in zip(full.outputs(), again.outputs()):
        assert torch.equal(x, y)                                         # a second identical pass, bit for bit
    assert int(counter.item()) == counter0                               # the forward pass reads the counter, it does not advance it
    # head: the float64 Linear on the features the kernel wrote
    want = feats.double() @ W.double().T + b.double()
    err = (head.double() - want).abs().max().item()
    print(f"head {_id(ij)}: max |head_out - Linear64(features)| = {err:.3e}")
    assert err < HEAD_TOL, err
    if c.precision:   # end to end: the module in float64 through a float64 Linear
        with torch.no_grad():
            want64 = ref64(obs.double()) @ W.double().T + b.double()
        allowed = REFERENCE_PRECISION_TOL * W.double().abs().sum(dim=1) + HEAD_TOL
        e64 = (head.double() - want64).abs()
        print(f"head {_id(ij)}: max |head_out - module64| = {e64.max().item():.3e}, features {(feats.double() - ref64(obs.double())).abs().max().item():.3e}")
        assert (e64 <= allowed[None, :]).all(), (e64.max(dim=0).values.tolist(), allowed.tolist())
    # sampler
    check_sampler(family_of(c), _id(ij), act, head, sigma, seed, counter0, step)
    # trajectory copy
    assert torch.equal(full.rew_dst[:B], full.rew_src) and torch.equal(full.done_dst[:B], full.done_src)


@pytest.mark.parametrize("name", cases.COUNTER_CONFIGS)
def test_counter_and_seed_semantics(name):
    """the Philox counter word is (*sample_counter + sample_step) mod 2^32 and the key the two halves of the seed: bit for bit from the kernel
    where two settings have to agree, and the model's draws at the summed value"""
    import torch
    i = [c.name for c in cases.CONFIGS].index(name)
    c = cases.CONFIGS[i]
    B, hd = cases.COUNTER_SHAPE
    _, fused, g, obs, W, b = case_inputs(c, i, 99, B, hd)
    sigma = cases.SIGMAS[:hd]
    log_std = torch.log(torch.tensor(sigma, device="cuda"))
    fused.set_head(W, b)

    def draw(seed, counter, step):
        ctr = torch.tensor([counter], device="cuda", dtype=torch.int32)
        head, act = torch.empty((B, hd), device="cuda"), torch.empty((B, hd), device="cuda")
        fused.forward_head(obs, head_out=head, sample=(log_std, act, ctr, step, seed))
        torch.cuda.synchronize()
        return head, act

    seen = []
    with selection(c):
        for case, (seed, counter, step, same_as) in cases.COUNTER_CASES.items():
            head, act = draw(seed, counter, step)
            check_sampler(family_of(c), f"{name}-{case}", act, head, sigma, seed, counter & 0xFFFFFFFF, step)
            if same_as is not None:
                head2, act2 = draw(seed, *same_as)
                assert torch.equal(act, act2) and torch.equal(head, head2), case
            seen.append(act)
    assert not torch.equal(seen[0], seen[1])             # counter 10 and counter 1
    for k in range(2, len(seen)):                        # every seed its own stream
        assert all(not torch.equal(seen[k], seen[m]) for m in range(k)), k


# ---- qs_rollout_pre / qs_rollout_post directly ----------------------------------------------------------------------------------------

def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _framed(n, offset, dtype=None, fill=SENT):
    """(whole allocation, its n-element window `4 + offset` elements in): sentinels on both sides, the window 16-byte aligned iff offset == 0"""
    import torch
    whole = torch.full((n + 12,), fill, device="cuda", dtype=dtype or torch.float32)
    assert whole.data_ptr() % 16 == 0
    return whole, whole[4 + offset:4 + offset + n]


def _frame_intact(whole, offset, n, fill=SENT):
    return bool((whole[:4 + offset] == fill).all()) and bool((whole[4 + offset + n:] == fill).all())


@pytest.mark.parametrize("A", cases.PRE_AGENTS)
def test_rollout_pre_samples_what_the_model_draws(A):
    import torch
    from quad_swarm_rl_amd import policy
    L = policy.lib()
    g = torch.Generator(device="cuda").manual_seed(A)
    sigma = cases.SIGMAS[:4]
    log_std = torch.log(torch.tensor(sigma, device="cuda"))
    counter = torch.tensor([cases.PRE_COUNTER], device="cuda", dtype=torch.int32)
    mean_values = (torch.randn((A, 4), device="cuda", generator=g) * 2.0).clamp_(-cases.HEAD_ABS_MAX, cases.HEAD_ABS_MAX)
    results = {}
    for mean_off, act_off in ((0, 0), (1, 1), (1, 0), (0, 1)):
        mean_whole, mean = _framed(4 * A, mean_off)
        mean.copy_(mean_values.reshape(-1))
        assert (mean.data_ptr() % 16 == 0) == (mean_off == 0)
        for with_noise in (True, False):
            act_whole, act = _framed(4 * A, act_off)
            assert (act.data_ptr() % 16 == 0) == (act_off == 0)
            rc = L.qs_rollout_pre(None, None, 0, _ptr(mean), _ptr(log_std) if with_noise else None, _ptr(act), A, C.c_uint64(cases.PRE_SEED), _ptr(counter), _stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert _frame_intact(act_whole, act_off, 4 * A) and _frame_intact(mean_whole, mean_off, 4 * A)
            results[(mean_off, act_off, with_noise)] = act.clone().reshape(A, 4)
    assert int(counter.item()) == cases.PRE_COUNTER
    check_sampler("qs_rollout_pre", f"A={A}", results[(0, 0, True)], mean_values, sigma, cases.PRE_SEED, cases.PRE_COUNTER, 0)
    for key, act in results.items():
        if key[2]:
            assert torch.equal(act, results[(0, 0, True)]), key     # the element path draws the same bits as the 16-byte path
        else:
            assert torch.equal(act, mean_values), key               # log_std = NULL: the action is the mean


@pytest.mark.parametrize("n_obs", cases.PRE_OBS_COUNTS)
def test_rollout_pre_copies_the_observations_exactly(n_obs):
    import torch
    from quad_swarm_rl_amd import policy
    L = policy.lib()
    g = torch.Generator(device="cuda").manual_seed(n_obs + 1)
    A = 5
    mean = torch.randn((A, 4), device="cuda", generator=g)
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    values = torch.randn((n_obs,), device="cuda", generator=g)
    for src_off, dst_off in ((0, 0), (0, 1), (1, 0), (1, 1)):
        src_whole, src = _framed(n_obs, src_off)
        src.copy_(values)
        dst_whole, dst = _framed(n_obs, dst_off, fill=-SENT)
        act = torch.full((A + PAD, 4), SENT, device="cuda")
        rc = L.qs_rollout_pre(_ptr(src) if n_obs else None, _ptr(dst) if n_obs else None, n_obs, _ptr(mean), None, _ptr(act), A, C.c_uint64(1), _ptr(counter), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(dst, values), (src_off, dst_off)
        assert _frame_intact(dst_whole, dst_off, n_obs, fill=-SENT) and _frame_intact(src_whole, src_off, n_obs)
        assert torch.equal(act[:A], mean) and bool((act[A:] == SENT).all())


@pytest.mark.parametrize("A", cases.POST_AGENTS)
def test_rollout_post_copies_and_counts(A):
    import torch
    from quad_swarm_rl_amd import policy
    L = policy.lib()
    g = torch.Generator(device="cuda").manual_seed(A + 2)
    counter = torch.tensor([-2], device="cuda", dtype=torch.int32)       # 0xfffffffe
    for want_counter in (-1, 0, 1):                                      # 0xffffffff, then the wrap to 0
        rew = torch.randn((A,), device="cuda", generator=g)
        done = torch.randint(0, 256, (A,), device="cuda", generator=g, dtype=torch.uint8)
        rew_whole, rew_out = _framed(A, 0)
        done_whole, done_out = _framed(A, 1, dtype=torch.uint8, fill=SENT_BYTE)
        assert L.qs_rollout_post(_ptr(rew), _ptr(rew_out), _ptr(done), _ptr(done_out), A, _ptr(counter), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(rew_out, rew) and torch.equal(done_out, done)
        assert _frame_intact(rew_whole, 0, A) and _frame_intact(done_whole, 1, A, fill=SENT_BYTE)
        assert int(counter.item()) == want_counter


def test_rollout_glue_refusals():
    """each NULL required pointer and each negative count: -1 with a message, and nothing ran"""
    import torch
    from quad_swarm_rl_amd import policy
    L = policy.lib()
    A, n = 5, 12
    obs, mean = torch.randn(n, device="cuda"), torch.randn((A, 4), device="cuda")
    obs_out, act = torch.full((n,), SENT, device="cuda"), torch.full((A, 4), SENT, device="cuda")
    log_std = torch.zeros(4, device="cuda")
    counter = torch.tensor([5], device="cuda", dtype=torch.int32)
    good = dict(obs=_ptr(obs), obs_out=_ptr(obs_out), n_obs=n, mean=_ptr(mean), log_std=_ptr(log_std), act_out=_ptr(act), A=A)
    bad = [dict(obs=None), dict(obs_out=None), dict(mean=None), dict(act_out=None), dict(counter=None), dict(n_obs=-1), dict(A=-1)]
    for change in bad:
        kw = dict(good, counter=_ptr(counter))
        kw.update(change)
        rc = L.qs_rollout_pre(kw["obs"], kw["obs_out"], kw["n_obs"], kw["mean"], kw["log_std"], kw["act_out"], kw["A"], C.c_uint64(3), kw["counter"], _stream())
        assert rc == -1 and L.qs_enc_last_error() == b"bad argument", change
    rew, done = torch.randn(A, device="cuda"), torch.ones(A, device="cuda", dtype=torch.uint8)
    rew_out, done_out = torch.full((A,), SENT, device="cuda"), torch.full((A,), SENT_BYTE, device="cuda", dtype=torch.uint8)
    good = dict(rew=_ptr(rew), rew_out=_ptr(rew_out), done=_ptr(done), done_out=_ptr(done_out), A=A, counter=_ptr(counter))
    for change in [dict(rew=None), dict(rew_out=None), dict(done=None), dict(done_out=None), dict(counter=None), dict(A=-1)]:
        kw = dict(good)
        kw.update(change)
        rc = L.qs_rollout_post(kw["rew"], kw["rew_out"], kw["done"], kw["done_out"], kw["A"], kw["counter"], _stream())
        assert rc == -1 and L.qs_enc_last_error() == b"bad argument", change
    torch.cuda.synchronize()
    assert bool((obs_out == SENT).all()) and bool((act == SENT).all()) and bool((rew_out == SENT).all()) and bool((done_out == SENT_BYTE).all())
    assert int(counter.item()) == 5
    # complete calls on the same buffers are accepted: each refusal above was about its one argument
    assert L.qs_rollout_pre(None, None, 0, _ptr(mean), None, _ptr(act), A, C.c_uint64(3), _ptr(counter), _stream()) == 0
    assert L.qs_rollout_post(_ptr(rew), _ptr(rew_out), _ptr(done), _ptr(done_out), A, _ptr(counter), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(act, mean) and torch.equal(rew_out, rew) and int(counter.item()) == 6


# ---- closed loop ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("copying", [False, True], ids=["in_place", "copying_glue"])
def test_every_action_of_a_replayed_segment_is_the_models_draw(copying):
    """GraphedRollout(sample=True), three replays of a six-step captured segment: actions[t] = means[t] + sigma * z_model(head.seed, counter
    before the run + t, agent), and the counter advances by exactly the steps run - so no (counter, agent) pair is ever drawn twice.
    in_place: the encoder's epilogue samples (counter + step, advanced once per segment); copying_glue (the replay wrapper keeps the outputs
    in the library's buffers): qs_rollout_pre samples and qs_rollout_post advances the counter every step."""
    import torch
    from quad_swarm_rl_amd import policy, rollout
    from quad_swarm_rl_amd.env import QuadSwarmVecEnv
    kw = dict(num_agents=cases.LOOP_AGENTS, neighbor_visible_num=6, neighbor_obs_type="pos_vel", use_numba=True, collision_falloff_radius=4.0)
    env = QuadSwarmVecEnv(cases.LOOP_ENVS, seed=5, **(dict(kw, episode_sums=True) if copying else kw))
    if copying:
        env.stepper.replay_enable(0.75)
    env.reset()
    enc = policy.FusedQuadEncoder(policy.make_reference_encoder(seed=2, nbr_encoder="mean_embed").cuda())
    head = rollout.GaussianActionHead(sample=True, seed=cases.LOOP_SEED)
    sigma = cases.SIGMAS[:4]
    with torch.no_grad():
        head.log_std.copy_(torch.log(torch.tensor(sigma, device=head.log_std.device)))
    T = cases.LOOP_STEPS
    seg = rollout.GraphedRollout(env, enc, head, steps=T)
    assert seg._glue and seg._in_place == (not copying) and seg.graph is not None
    drawn = set()
    for r in range(cases.LOOP_RUNS):
        before = int(seg._counter.item()) & 0xFFFFFFFF
        assert before == cases.LOOP_COUNTER0 + T * r                    # (the inputs tests/test_sampler_model_cpu.py holds the mutants against)
        out = {k: v.clone() for k, v in seg.run().items()}
        torch.cuda.synchronize()
        for t in range(T):
            where = f"{'copying' if copying else 'in place'} run {r} step {t}"
            if copying:
                check_sampler("closed loop, qs_rollout_pre", where, out["actions"][t], out["means"][t], sigma, cases.LOOP_SEED, before + t, 0)
            else:
                check_sampler("closed loop, epilogue", where, out["actions"][t], out["means"][t], sigma, cases.LOOP_SEED, before, t)
            assert before + t not in drawn
            drawn.add(before + t)
    assert (int(seg._counter.item()) & 0xFFFFFFFF) == cases.LOOP_COUNTER0 + T * cases.LOOP_RUNS
    assert len(drawn) == T * cases.LOOP_RUNS
    env.close()

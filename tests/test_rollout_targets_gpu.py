"""qs_rollout_targets and the critic inside a rollout segment (rollout.GraphedRollout critic= / targets=) on the GPU, against the float64
model of tests/rollout_targets_model.py under its rounding bounds (shown attainable on the CPU by tests/test_rollout_targets_cpu.py)."""
import copy
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rollout_targets_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

GAMMA = 0.99
VALUE_TOL = 1e-5   # tests/test_policy_encoder_gpu.py REFERENCE_PRECISION_TOL: what forward_head is held to in reference precision
ENV_KW = dict(num_agents=8, neighbor_visible_num=6, neighbor_obs_type="pos_vel", use_downwash=True, use_numba=True, collision_falloff_radius=4.0,
              rew_coeff=dict(quadcol_bin=5.0, quadcol_bin_smooth_max=10.0), ep_time=0.3)   # 31-step episodes
TARGETS = dict(gamma=GAMMA, gae_lambda=0.95, reward_scale=1.0, reward_clip=10.0)


def _device(d):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in d.items()}


def _check_against_model(tag, d, lam, scale, clip, logp, adv, ret):
    """d: float32 numpy inputs; logp / adv / ret: what the device produced from them.  Prints every figure before asserting."""
    args = (d["rewards"], d["dones"], d["values"], np.float32(GAMMA), np.float32(lam), np.float32(scale), np.float32(clip))
    m_adv, m_ret = model.gae(*args)
    b_adv, b_ret = model.gae_bounds(*args)
    w_adv = float((np.abs(adv.astype(np.float64) - m_adv) / b_adv).max())
    w_ret = float((np.abs(ret.astype(np.float64) - m_ret) / b_ret).max())
    w_lp = None
    if logp is not None:
        m_lp, b_lp = model.gaussian_logp(d["means"], d["actions"], d["log_std"]), model.logp_bound(d["means"], d["actions"], d["log_std"])
        w_lp = float((np.abs(logp.astype(np.float64) - m_lp) / b_lp).max())
    print(f"\n{tag}: |error| / bound - advantages {w_adv:.3f}, returns {w_ret:.3f}, log-probabilities {w_lp if w_lp is None else round(w_lp, 3)}")
    assert np.isfinite(adv).all() and np.isfinite(ret).all()
    assert w_adv <= 1.0 and w_ret <= 1.0 and (w_lp is None or w_lp <= 1.0), tag


@pytest.mark.parametrize("T,A,lam,scale", [(1, 1, 1.0, 1.0), (1, 1, 0.95, 1.0), (7, 100, 1.0, 1.0), (7, 100, 0.95, 30.0), (33, 4097, 1.0, 1.0),
                                           (33, 4097, 0.95, 1.0), (128, 8192, 1.0, 30.0), (128, 8192, 0.95, 1.0)])
def test_kernel_against_the_model(T, A, lam, scale):
    import torch
    from quad_swarm_rl_amd import policy
    d = model.synthetic(T, A, seed=T + A)
    if scale == 30.0:
        assert (np.abs(d["rewards"] * 30.0) > 10.0).mean() > 0.3          # the clip is active
    if A >= 3:
        assert d["dones"][:, 1].all() and not d["dones"][:, 2].any() and (T * A < 1000 or 0.01 < d["dones"][:, 3:].mean() < 0.03)
    t = _device(d)
    kw = dict(gamma=GAMMA, gae_lambda=lam, reward_scale=scale, reward_clip=10.0)
    logp, adv, ret = policy.rollout_targets(t["rewards"], t["dones"], t["values"], means=t["means"], actions=t["actions"], log_std=t["log_std"], **kw)
    logp2, adv2, ret2 = policy.rollout_targets(t["rewards"], t["dones"], t["values"], means=t["means"], actions=t["actions"], log_std=t["log_std"], **kw)
    none, adv3, ret3 = policy.rollout_targets(t["rewards"], t["dones"], t["values"], **kw)                     # no log-probabilities at all
    P = policy.RolloutTargetsParams()                                                                          # means / actions given, logp = NULL
    adv4, ret4 = torch.full_like(adv, 7.0), torch.full_like(ret, 7.0)
    P.T, P.A, P.rewards, P.dones, P.values = T, A, t["rewards"].data_ptr(), t["dones"].data_ptr(), t["values"].data_ptr()
    P.means, P.actions, P.log_std, P.act_dim = t["means"].data_ptr(), t["actions"].data_ptr(), t["log_std"].data_ptr(), 4
    P.gamma, P.gae_lambda, P.reward_scale, P.reward_clip = GAMMA, lam, scale, 10.0
    P.advantages, P.returns = adv4.data_ptr(), ret4.data_ptr()
    import ctypes as C
    assert policy.lib().qs_rollout_targets(C.byref(P), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(logp, logp2) and torch.equal(adv, adv2) and torch.equal(ret, ret2)                     # same inputs, same bits
    assert none is None and torch.equal(adv, adv3) and torch.equal(ret, ret3) and torch.equal(adv, adv4) and torch.equal(ret, ret4)
    _check_against_model(f"T={T} A={A} lambda={lam} scale={scale}", d, lam, scale, 10.0, logp.cpu().numpy(), adv.cpu().numpy(), ret.cpu().numpy())


@pytest.mark.parametrize("chunks", [1, 16])
def test_both_forms_of_the_scan(chunks):
    """the plain one-lane-per-agent form and the time-chunked form, each forced at every shape (qs_rollout_set_targets_chunks), T not a
    multiple of the chunk count and T smaller than it; each inside the bounds and bitwise reproducible"""
    import torch
    from quad_swarm_rl_amd import policy
    L = policy.lib()
    prev = L.qs_rollout_set_targets_chunks(chunks)
    try:
        for T, A in ((77, 1000), (5, 130)):
            d = model.synthetic(T, A, seed=chunks + T)
            t = _device(d)
            kw = dict(gamma=GAMMA, gae_lambda=0.95, reward_scale=2.0, reward_clip=10.0)
            logp, adv, ret = policy.rollout_targets(t["rewards"], t["dones"], t["values"], means=t["means"], actions=t["actions"], log_std=t["log_std"], **kw)
            again = policy.rollout_targets(t["rewards"], t["dones"], t["values"], means=t["means"], actions=t["actions"], log_std=t["log_std"], **kw)
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip((logp, adv, ret), again))
            _check_against_model(f"chunks={chunks} T={T} A={A}", d, 0.95, 2.0, 10.0, logp.cpu().numpy(), adv.cpu().numpy(), ret.cpu().numpy())
    finally:
        L.qs_rollout_set_targets_chunks(prev)


@pytest.mark.parametrize("act_dim", [1, 3, 8])
def test_other_action_widths(act_dim):
    """rows that are not one 16-byte load: the generic path of the log-probabilities"""
    import torch
    from quad_swarm_rl_amd import policy
    d = model.synthetic(9, 300, seed=act_dim, act_dim=act_dim)
    t = _device(d)
    logp, adv, ret = policy.rollout_targets(t["rewards"], t["dones"], t["values"], means=t["means"], actions=t["actions"], log_std=t["log_std"], **TARGETS)
    torch.cuda.synchronize()
    _check_against_model(f"act_dim={act_dim}", d, 0.95, 1.0, 10.0, logp.cpu().numpy(), adv.cpu().numpy(), ret.cpu().numpy())


def _critic(nbr_encoder, precision="fp32", seed=7):
    import torch
    from quad_swarm_rl_amd import policy
    module = policy.make_reference_encoder(seed=seed, nbr_encoder=nbr_encoder).cuda()
    torch.manual_seed(seed + 1)
    value = torch.nn.Linear(512, 1).cuda()
    critic = policy.FusedQuadEncoder(module, precision=precision)
    critic.set_head(value.weight, value.bias)
    return module, value, critic


def _values64(encoder_module, value_layer, obs, last_obs, chunk):
    """the critic's torch module in float64 over the recorded rows, batched as the segment batches them (the `attention` encoder pairs rows
    ACROSS a batch - quad_multi_model.py:84,92 tile the whole batch - so the slicing is part of the function)"""
    import torch
    T, A, D = obs.shape
    flat = obs.reshape(T * A, D).double()
    enc64, val64 = copy.deepcopy(encoder_module).double(), copy.deepcopy(value_layer).double()
    with torch.no_grad():
        parts = [val64(enc64(flat[s0:s0 + chunk])) for s0 in range(0, T * A, chunk)] + [val64(enc64(last_obs.double()))]
    return torch.cat(parts)


def _segments(nbr_encoder, graph, with_critic, E=6, T=40, sample=True, critic_chunk=1000, runs=2):
    """`runs` consecutive segments on a fresh environment (same seed every time): list of dicts of cloned tensors, + the objects"""
    import torch
    from quad_swarm_rl_amd import policy, rollout
    from quad_swarm_rl_amd.env import QuadSwarmVecEnv
    enc = policy.FusedQuadEncoder(policy.make_reference_encoder(seed=2, nbr_encoder=nbr_encoder).cuda())
    head = rollout.GaussianActionHead(sample=sample, seed=4)
    env = QuadSwarmVecEnv(E, seed=3, **ENV_KW)
    env.reset()
    extra, objs = {}, None
    if with_critic:
        objs = _critic(nbr_encoder)
        extra = dict(critic=objs[2], targets=TARGETS, critic_chunk=critic_chunk)
    seg = rollout.GraphedRollout(env, enc, head, steps=T, graph=graph, **extra)
    if not graph:
        seg.warmup()
    outs = []
    for _ in range(runs):
        outs.append({k: v.clone() for k, v in seg.run().items()})
    torch.cuda.synchronize()
    return outs, seg, env, head, objs


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("nbr_encoder", ["mean_embed", "attention"])
def test_the_segment_is_unchanged_by_critic_and_targets(nbr_encoder, graph):
    import torch
    plain, _, env_a, _, _ = _segments(nbr_encoder, graph, with_critic=False)
    full, _, env_b, _, _ = _segments(nbr_encoder, graph, with_critic=True)
    for a, b in zip(plain, full):
        for k in ("obs", "actions", "means", "rewards", "dones", "last_obs"):
            assert torch.equal(a[k], b[k]), k
        assert "values" not in a and "logp" not in a
        assert a["dones"].any() and not a["dones"].all()
        assert a["dones"].any(dim=0).all()                      # every agent finished an episode inside the segment
        for k in ("values", "logp", "advantages", "returns"):
            assert torch.isfinite(b[k]).all(), k
    env_a.close(); env_b.close()


@pytest.mark.parametrize("nbr_encoder", ["mean_embed", "attention"])
def test_values_logp_advantages_returns_of_a_segment(nbr_encoder):
    """values == eager critic.forward_head over the recorded rows with the segment's slicing, and within the reference-precision bound of the
    critic's torch module in float64; logp / advantages / returns == a stand-alone qs_rollout_targets call on the returned tensors, and
    inside the model's bounds"""
    import torch
    from quad_swarm_rl_amd import policy
    chunk = 1000
    outs, seg, env, head, (module, value, critic) = _segments(nbr_encoder, True, with_critic=True, critic_chunk=chunk)
    for out in outs:
        T, A, D = out["obs"].shape
        flat = torch.cat((out["obs"].reshape(T * A, D), out["last_obs"]))
        want = torch.empty((T * A + A, 1), device="cuda")
        for s0 in range(0, T * A, chunk):
            want[s0:min(T * A, s0 + chunk)] = critic.forward_head(flat[s0:min(T * A, s0 + chunk)].contiguous())
        want[T * A:] = critic.forward_head(out["last_obs"].contiguous())
        assert torch.equal(out["values"].reshape(-1, 1), want)
        v64 = _values64(module, value, out["obs"], out["last_obs"], chunk)
        err = (out["values"].reshape(-1, 1).double() - v64).abs().max().item()
        print(f"\n{nbr_encoder}: values vs the float64 module: max |error| {err:.3e} (bound {VALUE_TOL:g}), |V| up to {v64.abs().max().item():.3f}")
        assert err < VALUE_TOL
        logp, adv, ret = policy.rollout_targets(out["rewards"], out["dones"], out["values"], means=out["means"], actions=out["actions"],
                                                log_std=head.log_std, **TARGETS)
        torch.cuda.synchronize()
        assert torch.equal(logp, out["logp"]) and torch.equal(adv, out["advantages"]) and torch.equal(ret, out["returns"])
        d = {k: out[k].cpu().numpy() for k in ("rewards", "dones", "values", "means", "actions")}
        d["log_std"] = head.log_std.cpu().numpy()
        _check_against_model(f"segment {nbr_encoder}", d, TARGETS["gae_lambda"], TARGETS["reward_scale"], TARGETS["reward_clip"],
                             out["logp"].cpu().numpy(), out["advantages"].cpu().numpy(), out["returns"].cpu().numpy())
    assert outs[0]["dones"].any() and not torch.equal(outs[0]["values"], outs[1]["values"])
    env.close()


def test_the_copying_and_the_plain_paths_fill_the_same_outputs():
    """a handle with the device-side replay wrapper (_step_copying) and a head the library does not fuse (_step): values and targets of the
    recorded rows there too"""
    import torch
    from quad_swarm_rl_amd import policy, rollout
    from quad_swarm_rl_amd.env import QuadSwarmVecEnv
    kw = {k: v for k, v in ENV_KW.items() if k != "rew_coeff"}

    class PlainHead:   # no weight / from_mean: features -> actions in torch
        def __init__(self):
            self.lin = torch.nn.Linear(512, 4).cuda()

        def __call__(self, feats):
            with torch.no_grad():
                return self.lin(feats)

    for flavour in ("replay", "plain"):
        env = QuadSwarmVecEnv(8, seed=5, episode_sums=flavour == "replay", **kw)
        if flavour == "replay":
            env.stepper.replay_enable(0.75)
        env.reset()
        enc = policy.FusedQuadEncoder(policy.make_reference_encoder(seed=2, nbr_encoder="mean_embed").cuda())
        module, value, critic = _critic("mean_embed")
        head = rollout.GaussianActionHead(sample=True, seed=3) if flavour == "replay" else PlainHead()
        seg = rollout.GraphedRollout(env, enc, head, steps=12, critic=critic, targets=TARGETS, graph=flavour == "replay")
        if flavour == "plain":
            seg.warmup()
        assert (seg._glue and not seg._in_place) if flavour == "replay" else not seg._fused_head
        seg.run()
        out = {k: v.clone() for k, v in seg.run().items()}
        torch.cuda.synchronize()
        assert ("logp" in out) == (flavour == "replay")            # the plain head records no means: no density to report
        T, A, D = out["obs"].shape
        want = torch.cat((critic.forward_head(out["obs"].reshape(T * A, D)), critic.forward_head(out["last_obs"].contiguous())))   # the segment's own slicing
        assert torch.equal(out["values"].reshape(-1, 1), want)
        extra = dict(means=out["means"], actions=out["actions"], log_std=head.log_std) if flavour == "replay" else {}
        logp, adv, ret = policy.rollout_targets(out["rewards"], out["dones"], out["values"], **TARGETS, **extra)
        torch.cuda.synchronize()
        assert torch.equal(adv, out["advantages"]) and torch.equal(ret, out["returns"]) and (logp is None or torch.equal(logp, out["logp"]))
        env.close()


def test_refresh_reaches_the_captured_critic():
    """the critic's weights live in device buffers the captured graph points at: after the module moved and refresh(), a replay of the SAME
    mean_embed graph returns the new values"""
    import torch
    outs, seg, env, head, (module, value, critic) = _segments("mean_embed", True, with_critic=True, runs=1)
    graph = seg.graph
    with torch.no_grad():
        for prm in module.parameters():
            prm.mul_(0.5)
        value.weight.mul_(2.0); value.bias.add_(0.25)
    critic.refresh()
    out = {k: v.clone() for k, v in seg.run().items()}
    torch.cuda.synchronize()
    assert seg.graph is graph
    T, A, D = out["obs"].shape
    v64 = _values64(module, value, out["obs"], out["last_obs"], 1000)
    err = (out["values"].reshape(-1, 1).double() - v64).abs().max().item()
    print(f"\nafter refresh: values vs the moved float64 module: max |error| {err:.3e}")
    assert err < VALUE_TOL
    assert (out["values"][0] - outs[0]["values"][-1]).abs().max().item() > 1e-3    # the same rows (this segment starts where the first ended), new weights
    env.close()


def test_targets_need_a_critic_and_a_deterministic_head_has_no_logp():
    import torch
    from quad_swarm_rl_amd import policy, rollout
    from quad_swarm_rl_amd.env import QuadSwarmVecEnv
    env = QuadSwarmVecEnv(4, seed=5, **ENV_KW)
    env.reset()
    enc = policy.FusedQuadEncoder(policy.make_reference_encoder(seed=2, nbr_encoder="mean_embed").cuda())
    with pytest.raises(ValueError):
        rollout.GraphedRollout(env, enc, rollout.GaussianActionHead(sample=True), steps=4, targets=TARGETS)
    with pytest.raises(ValueError):   # a critic without its value head
        rollout.GraphedRollout(env, enc, rollout.GaussianActionHead(sample=True), steps=4,
                               critic=policy.FusedQuadEncoder(policy.make_reference_encoder(seed=3, nbr_encoder="mean_embed").cuda()))
    module, value, critic = _critic("mean_embed")
    seg = rollout.GraphedRollout(env, enc, rollout.GaussianActionHead(sample=False, seed=4), steps=4, critic=critic, targets=TARGETS)
    out = seg.run()
    torch.cuda.synchronize()
    assert "logp" not in out and {"values", "advantages", "returns"} <= set(out)
    assert "values" not in rollout.GraphedRollout(env, enc, rollout.GaussianActionHead(sample=False, seed=4), steps=4).run()
    env.close()


def test_the_harness_trains_on_device_targets():
    """tools/ppo_c5.py --device_targets=True: after collect() the learner's values, log-probabilities, advantages and returns are those of
    the torch path recomputed (in float64) from the same recorded buffers, and the updates run to finite losses"""
    import torch
    import ppo_c5
    cfg = ppo_c5.parse(["--device_targets=True", "--quads_num_envs=16", "--rollout=32", "--batch_size=512", "--iterations=2", "--seed=0"])
    env = ppo_c5.make_env(cfg)
    lr = ppo_c5.Learner(cfg, env)
    assert lr.segment is not None and lr.fused_critic is not None and lr.targets_note.startswith("device"), (lr.sampler_note, lr.targets_note)
    T = cfg.rollout
    for it in range(2):
        lr.collect()
        torch.cuda.synchronize()
        adv, ret = lr.advantages()
        with torch.no_grad():
            v64 = _values64(lr.ac.critic_encoder, lr.ac.value, lr.obs[:T], lr.obs[T], lr.segment.critic_chunk).reshape(T + 1, lr.A)
            lp64 = ppo_c5.gaussian_logp(lr.segment.means.double(), lr.head.log_std.double(), lr.act.double())
        err_v = (lr.val.double() - v64).abs().max().item()
        print(f"\niteration {it}: values vs the float64 critic: max |error| {err_v:.3e} (bound {VALUE_TOL:g})")
        assert err_v < VALUE_TOL
        d = dict(rewards=lr.rew.cpu().numpy(), dones=lr.done.cpu().numpy(), values=lr.val.cpu().numpy(), means=lr.segment.means.cpu().numpy(),
                 actions=lr.act.cpu().numpy(), log_std=lr.head.log_std.cpu().numpy())
        me = types.SimpleNamespace(torch=torch, cfg=cfg, rew=lr.rew.double(), done=lr.done.double(), val=lr.val.double())
        adv64, ret64 = ppo_c5.Learner.advantages(me)                      # the torch path, on the values the device path used
        b_adv, b_ret = model.gae_bounds(d["rewards"], d["dones"], d["values"], np.float32(cfg.gamma), np.float32(cfg.gae_lambda),
                                        np.float32(cfg.reward_scale), np.float32(cfg.reward_clip))
        b_lp = model.logp_bound(d["means"], d["actions"], d["log_std"])
        w = [float(((x.double() - y).abs().cpu().numpy() / b).max()) for x, y, b in ((adv, adv64, b_adv), (ret, ret64, b_ret), (lr.logp, lp64, b_lp))]
        print(f"iteration {it}: |error| / bound - advantages {w[0]:.3f}, returns {w[1]:.3f}, log-probabilities {w[2]:.3f}")
        assert max(w) <= 1.0
        st = lr.update()
        assert np.isfinite(st["policy_loss"]) and np.isfinite(st["value_loss"]) and np.isfinite(st["kl"]) and st["updates"] == T * lr.A // cfg.batch_size
    env.close()
    recs, summary = ppo_c5.train(cfg)
    assert summary["targets"].startswith("device") and all(np.isfinite(r["value_loss"]) and np.isfinite(r["policy_loss"]) for r in recs)

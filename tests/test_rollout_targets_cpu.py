"""qs_rollout_targets without a GPU: the test model (tests/rollout_targets_model.py) is tied to the functions the PPO harness already has,
the bounds the GPU test applies are shown to be attainable by plain float32 arithmetic, and the C ABI refuses bad arguments before anything
touches a device."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rollout_targets_model as model  # noqa: E402


def _float64_inputs(T, A, seed, reward_scale):
    g = np.random.default_rng(seed)
    rewards = g.standard_normal((T, A)) * 3.0
    values = g.standard_normal((T + 1, A)) * 5.0
    dones = (g.random((T, A)) < 0.1).astype(np.float64)
    assert dones.any() and (np.abs(rewards * reward_scale) > 4.0).any() and (np.abs(rewards * reward_scale) < 4.0).any()   # dones, active clipping
    return rewards, dones, values


@pytest.mark.parametrize("gae_lambda", [1.0, 0.95, 0.0])
def test_model_is_the_harness_arithmetic(gae_lambda):
    """float64 in, float64 out: the model equals tools.ppo_c5.gaussian_logp and tools.ppo_c5.Learner.advantages to 1e-12 relative"""
    torch = pytest.importorskip("torch")
    import ppo_c5
    T, A = 40, 37
    cfg = types.SimpleNamespace(rollout=T, gamma=0.99, gae_lambda=gae_lambda, reward_scale=1.7, reward_clip=4.0)
    rewards, dones, values = _float64_inputs(T, A, 3, cfg.reward_scale)
    me = types.SimpleNamespace(torch=torch, cfg=cfg, rew=torch.from_numpy(rewards), done=torch.from_numpy(dones), val=torch.from_numpy(values))
    adv, ret = ppo_c5.Learner.advantages(me)
    m_adv, m_ret = model.gae(rewards, dones, values, cfg.gamma, cfg.gae_lambda, cfg.reward_scale, cfg.reward_clip)
    np.testing.assert_allclose(m_adv, adv.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(m_ret, ret.numpy(), rtol=1e-12, atol=0)
    g = np.random.default_rng(5)
    means, log_std = g.standard_normal((T, A, 4)), g.uniform(-1.5, 0.5, 4)
    actions = means + np.exp(log_std) * g.standard_normal((T, A, 4))
    lp = ppo_c5.gaussian_logp(torch.from_numpy(means), torch.from_numpy(log_std), torch.from_numpy(actions))
    np.testing.assert_allclose(model.gaussian_logp(means, actions, log_std), lp.numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("reward_scale,gae_lambda", [(0.02, 1.0), (1.0, 0.95), (30.0, 0.9), (30.0, 1.0)])
def test_bounds_leave_room_for_sequential_float32(reward_scale, gae_lambda):
    """the GPU test's bounds, applied to a step-by-step float32 numpy evaluation of the same float32 inputs at the config-5 shape"""
    T, A = 128, 8192
    d = model.synthetic(T, A, seed=11, done_rate=0.01)
    args = (d["rewards"], d["dones"], d["values"], np.float32(0.99), np.float32(gae_lambda), np.float32(reward_scale), np.float32(10.0))
    adv, ret = model.gae(*args)
    adv32, ret32 = model.gae_float32(*args)
    b_adv, b_ret = model.gae_bounds(*args)
    assert (b_adv > 0).all()
    worst_adv, worst_ret = float((np.abs(adv32 - adv) / b_adv).max()), float((np.abs(ret32 - ret) / b_ret).max())
    lp, lp32 = model.gaussian_logp(d["means"], d["actions"], d["log_std"]), model.logp_float32(d["means"], d["actions"], d["log_std"])
    worst_lp = float((np.abs(lp32 - lp) / model.logp_bound(d["means"], d["actions"], d["log_std"])).max())
    print(f"\nsequential float32 / bound: advantages {worst_adv:.3f}, returns {worst_ret:.3f}, log-probabilities {worst_lp:.3f}")
    assert worst_adv <= 1.0 and worst_ret <= 1.0 and worst_lp <= 1.0
    assert worst_adv > 1e-3 and worst_lp > 1e-3          # ... and they are rounding bounds, not orders of magnitude of slack
    if reward_scale == 30.0:
        assert (np.abs(d["rewards"] * 30.0) > 10.0).mean() > 0.3   # the clip is active


def _params(policy, **kw):
    """a parameter struct whose pointers are all non-NULL (never dereferenced on the host: every call below is refused first)"""
    P = policy.RolloutTargetsParams()
    P.T, P.A, P.act_dim = 8, 16, 4
    P.gamma, P.gae_lambda, P.reward_scale, P.reward_clip = 0.99, 0.95, 1.0, 10.0
    for name in ("rewards", "dones", "values", "means", "actions", "log_std", "logp", "advantages", "returns"):
        setattr(P, name, 4096)
    for k, v in kw.items():
        setattr(P, k, v)
    return P


def test_c_abi_exports_layout_and_refusals():
    """libquadswarm_encoder.so exports qs_rollout_targets / qs_rollout_sizeof_targets, the ctypes mirror has the library's size, and every
    invalid argument of include/quadswarm_encoder.h is refused with a negative status and a message - before a launch (there is no GPU here)."""
    from quad_swarm_rl_amd import policy
    policy.build()
    lib = C.CDLL(policy.ENC_LIB_PATH)
    assert hasattr(lib, "qs_rollout_targets") and hasattr(lib, "qs_rollout_sizeof_targets") and hasattr(lib, "qs_rollout_set_targets_chunks")
    lib.qs_rollout_sizeof_targets.restype = C.c_size_t
    lib.qs_rollout_targets.argtypes = [C.POINTER(policy.RolloutTargetsParams), C.c_void_p]
    lib.qs_enc_last_error.restype = C.c_char_p
    assert lib.qs_rollout_sizeof_targets() == C.sizeof(policy.RolloutTargetsParams)
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quadswarm_encoder.h")).read()
    for decl in ("size_t qs_rollout_sizeof_targets(void);", "int qs_rollout_targets(const qs_rollout_targets_params *p, void *stream);"):
        assert decl in h
    nan = float("nan")
    bad = [dict(rewards=None), dict(dones=None), dict(values=None), dict(advantages=None), dict(returns=None), dict(log_std=None),
           dict(T=0), dict(A=0), dict(T=-3), dict(act_dim=0), dict(act_dim=9), dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=nan),
           dict(gae_lambda=-0.5), dict(gae_lambda=1.5), dict(gae_lambda=nan), dict(reward_clip=0.0), dict(reward_clip=-1.0), dict(reward_clip=nan),
           dict(means=None), dict(actions=None)]
    for kw in bad:
        P = _params(policy, **kw)
        rc = lib.qs_rollout_targets(C.byref(P), None)
        assert rc < 0 and len(lib.qs_enc_last_error()) > 0, kw
        assert b"qs_rollout_targets" in lib.qs_enc_last_error(), kw
    assert lib.qs_rollout_targets(None, None) < 0
    # the bench-only switch between the plain and the chunked scan (not in the header): returns the previous value, ignores what it does not accept
    lib.qs_rollout_set_targets_chunks.argtypes = [C.c_int32]
    lib.qs_rollout_set_targets_chunks.restype = C.c_int32
    assert lib.qs_rollout_set_targets_chunks(16) == 0 and lib.qs_rollout_set_targets_chunks(8) == 16 and lib.qs_rollout_set_targets_chunks(-1) == 16
    assert lib.qs_rollout_set_targets_chunks(1) == 16 and lib.qs_rollout_set_targets_chunks(0) == 1 and lib.qs_rollout_set_targets_chunks(-1) == 0


def test_the_library_is_stale_against_the_included_unit():
    from quad_swarm_rl_amd import policy
    assert any(os.path.basename(s) == "qs_rollout_targets.inc" for s in policy.ENC_SOURCES) and policy.ENC_SOURCE in policy.ENC_SOURCES


def test_harness_flag_defaults_to_off():
    pytest.importorskip("torch")
    import ppo_c5
    assert ppo_c5.parse([]).device_targets is False and ppo_c5.parse(["--device_targets=True"]).device_targets is True

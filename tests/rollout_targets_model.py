"""Test model of qs_rollout_targets (include/quadswarm_encoder.h): the formulas of tools/ppo_c5.py - Learner.advantages, gaussian_logp -
restated in float64 numpy, and the rounding bounds the float32 kernel is held to.  In the role tests/pilot_model.py has for the pilot.

    r_t   = clip(rewards_t * reward_scale, -reward_clip, +reward_clip)          nd_t = 1 - dones_t
    d_t   = r_t + gamma * V_{t+1} * nd_t - V_t
    adv_t = d_t + gamma * gae_lambda * nd_t * adv_{t+1},   adv_T = 0            ret_t = adv_t + V_t
    z_k   = (a_k - mean_k) * exp(-log_std_k)       logp = sum_k ( -0.5 * z_k^2 - log_std_k - 0.5 * log(2 pi) )

Bounds (t = 0 .. T - 1).  Every step of the recurrence is a handful of float32 operations on terms whose magnitudes sum to
S_t = |r_t| + gamma |V_{t+1}| nd_t + |V_t| + gamma lambda nd_t S_{t+1} (the same recurrence on absolute values), and adv_t has T - t steps
behind it: |error| <= 8 * (T - t + 1) * 2^-24 * S_t, with |V_t| more in S for the return.  A log-probability is ~ 6 operations per component
on terms of magnitude L = sum_k (0.5 z_k^2 + |log_std_k| + 0.5 log 2 pi): |error| <= 16 * 2^-24 * L.  A sequential float32 numpy evaluation
stays inside both (tests/test_rollout_targets_cpu.py), so they are attainable without the kernel."""
import math

import numpy as np

EPS = 2.0 ** -24
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def clipped_rewards(rewards, reward_scale, reward_clip):
    return np.clip(_f64(rewards) * float(reward_scale), -float(reward_clip), float(reward_clip))


def gae(rewards, dones, values, gamma, gae_lambda, reward_scale, reward_clip):
    """rewards [T, A], dones [T, A] (0 / 1), values [T + 1, A] -> (advantages, returns), float64 [T, A]"""
    r, nd, v = clipped_rewards(rewards, reward_scale, reward_clip), 1.0 - _f64(dones), _f64(values)
    gamma, lam = float(gamma), float(gae_lambda)
    T = r.shape[0]
    adv = np.zeros_like(r)
    last = np.zeros_like(r[0])
    for t in reversed(range(T)):
        last = (r[t] + gamma * v[t + 1] * nd[t] - v[t]) + gamma * lam * nd[t] * last
        adv[t] = last
    return adv, adv + v[:T]


def gaussian_logp(means, actions, log_std):
    """means, actions [..., K], log_std [K] -> log-probabilities [...] of a diagonal Gaussian"""
    ls = _f64(log_std)
    z = (_f64(actions) - _f64(means)) * np.exp(-ls)
    return (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)


def gae_magnitude(rewards, dones, values, gamma, gae_lambda, reward_scale, reward_clip):
    """S_t: the advantage recurrence on absolute values"""
    r, nd, v = np.abs(clipped_rewards(rewards, reward_scale, reward_clip)), 1.0 - _f64(dones), np.abs(_f64(values))
    gamma, lam = float(gamma), float(gae_lambda)
    T = r.shape[0]
    S = np.zeros_like(r)
    last = np.zeros_like(r[0])
    for t in reversed(range(T)):
        last = r[t] + gamma * v[t + 1] * nd[t] + v[t] + gamma * lam * nd[t] * last
        S[t] = last
    return S


def gae_bounds(rewards, dones, values, gamma, gae_lambda, reward_scale, reward_clip):
    """(allowed |error| of the advantages, of the returns), [T, A] each"""
    S = gae_magnitude(rewards, dones, values, gamma, gae_lambda, reward_scale, reward_clip)
    T = S.shape[0]
    steps = (T - np.arange(T) + 1.0).reshape((T,) + (1,) * (S.ndim - 1))
    return 8.0 * steps * EPS * S, 8.0 * steps * EPS * (S + np.abs(_f64(values)[:T]))


def logp_bound(means, actions, log_std):
    ls = _f64(log_std)
    z = (_f64(actions) - _f64(means)) * np.exp(-ls)
    return 16.0 * EPS * (0.5 * z * z + np.abs(ls) + HALF_LOG_2PI).sum(-1)


def gae_float32(rewards, dones, values, gamma, gae_lambda, reward_scale, reward_clip):
    """the same recurrence, every operation in float32, one step after the other (what the bounds must leave room for)"""
    f = np.float32
    r = np.clip(np.asarray(rewards, f) * f(reward_scale), -f(reward_clip), f(reward_clip))
    nd, v = f(1) - np.asarray(dones, f), np.asarray(values, f)
    T = r.shape[0]
    adv = np.zeros_like(r)
    last = np.zeros_like(r[0])
    for t in reversed(range(T)):
        last = (r[t] + f(gamma) * v[t + 1] * nd[t] - v[t]) + f(gamma) * f(gae_lambda) * nd[t] * last
        adv[t] = last
    return adv, adv + v[:T]


def logp_float32(means, actions, log_std):
    f = np.float32
    ls = np.asarray(log_std, f)
    z = (np.asarray(actions, f) - np.asarray(means, f)) * np.exp(-ls)
    return (f(-0.5) * z * z - ls - f(HALF_LOG_2PI)).sum(-1, dtype=f)


def synthetic(T, A, seed, act_dim=4, done_rate=0.02):
    """float32 inputs of a segment: rewards of a few units, values of ~ +-5, `done_rate` done flags plus (A >= 3) one agent that is done on
    every step and one that never is, action rows a standard normal step from their means, log_std in [-1, 0.5]"""
    g = np.random.default_rng(seed)
    rewards = (g.standard_normal((T, A)) * 0.5 - 0.2).astype(np.float32)
    values = (g.standard_normal((T + 1, A)) * 5.0).astype(np.float32)
    dones = (g.random((T, A)) < done_rate).astype(np.uint8)
    if A >= 3:
        dones[:, 1] = 1
        dones[:, 2] = 0
    means = g.standard_normal((T, A, act_dim)).astype(np.float32)
    log_std = g.uniform(-1.0, 0.5, act_dim).astype(np.float32)
    actions = (means + np.exp(log_std) * g.standard_normal((T, A, act_dim))).astype(np.float32)
    return dict(rewards=rewards, dones=dones, values=values, means=means, actions=actions, log_std=log_std)

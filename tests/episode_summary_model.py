"""The episode summary (include/quadswarm_summary.h) as a definition: numpy float64 from the raw arrays of a set of finished episodes to the two
tables, in the kernel's order (agents in index order, environments in index order) - and, for the tests, the thing the summary must equal: the
key-by-key mean of the per-agent dicts {"true_reward", **episode_extra_stats} that sf_env.EpisodeInfoBuilder.env_dicts gives, with the bound
each key is held to.

Bounds, u = 2^-53, m values x_j of a key:
  linear keys                  (m + 2) u sum|x_j| / m      - any summation order of m doubles is within (m - 1) u sum|x_j| of the exact sum, the
                                                             division and the expectation's own rounding add one u each
  true_reward, rewraw_main     the same with |main_j| + 1000 |quadcol_j| in place of |x_j| (the value is formed per agent from two sums)
  z_action*_std                per episode min(sqrt(d), d / std) with d = (n + 3) u (a2 + a1^2), n = agents per environment, averaged:
                               the variance a2 - a1^2 of n summed terms is off by at most d, and sqrt turns an error d of v into at most
                               sqrt(d) and, away from 0, into d / (2 sqrt(v))
  integer counts               exact
"""
import math

import numpy as np

from quad_swarm_rl_amd import abi, config as qcfg

U = 2.0 ** -53
COUNT_KEYS = ("episodes", "episodes_replayed", "overrun")


def left_out(key):
    """keys of the per-agent dicts that the summary does not carry (host scalars, and what replay_stats() gives at any time)"""
    return key == "z_approx_total_training_steps" or key.startswith("z_anneal_") or key.startswith("replay/")


def is_count(key):
    return key in COUNT_KEYS or key.startswith("episodes/")


def tables(n, sums, eps, cnt, ep_scen, cur_scen, was_replay, steps, episode_sums=True):
    """sums [QS_SUM_COUNT, F*n], eps [QS_EPS_COUNT, F*n], cnt [QS_CNT_COUNT, F], ep_scen / cur_scen / was_replay / steps [F] of F finished
    environments -> (sums table float64, counts table int64)"""
    D = np.zeros((abi.QS_SUMM_SCENARIOS, abi.QS_SUMM_D_COUNT), dtype=np.float64)
    I = np.zeros((abi.QS_SUMM_SCENARIOS, abi.QS_SUMM_I_COUNT), dtype=np.int64)
    sums, eps = np.asarray(sums, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    i_main, i_quadcol = qcfg.REW_INFO_KEYS.index("rewraw_main"), qcfg.REW_INFO_KEYS.index("rewraw_quadcol")
    i_pos, i_crash = qcfg.REW_INFO_KEYS.index("rew_pos"), qcfg.REW_INFO_KEYS.index("rew_crash")
    i_col, i_obst = qcfg.COUNTER_KEYS.index("collisions"), qcfg.COUNTER_KEYS.index("obst")
    for f in range(len(ep_scen)):
        s, c, rep = int(ep_scen[f]), int(cur_scen[f]), bool(was_replay[f])
        ag = slice(f * n, (f + 1) * n)
        I[s, abi.QS_SUMM_I_EPISODES] += 1
        I[c, abi.QS_SUMM_I_START_EPISODES] += 1
        if rep:
            I[s, abi.QS_SUMM_I_REPLAYED] += 1
            I[s, abi.QS_SUMM_I_COL_REPLAY] += int(cnt[i_col, f])
            I[s, abi.QS_SUMM_I_OBST_REPLAY] += int(cnt[i_obst, f])
        else:
            I[s, abi.QS_SUMM_I_CNT:abi.QS_SUMM_I_CNT + abi.QS_CNT_COUNT] += np.asarray(cnt[:, f], dtype=np.int64)
            reached, aok, ook = eps[3, ag], eps[4, ag] != 0, eps[5, ag] != 0
            ok = aok & ook
            rates = (np.sum(ok & (reached != 0)) / n, np.sum(ok & ((1 - reached) != 0)) / n, 1.0 - np.sum(ok) / n, 1.0 - np.sum(aok) / n, 1.0 - np.sum(ook) / n)
            for r, v in enumerate(rates):
                D[s, abi.QS_SUMM_D_SUCCESS + r] += v
            for d in range(3):
                for i in range(n):
                    D[s, abi.QS_SUMM_D_DIST_1S + d] += eps[d, f * n + i]
        if not episode_sums:
            continue
        for i in range(f * n, (f + 1) * n):
            for r in range(abi.QS_RI_COUNT):
                D[s, abi.QS_SUMM_D_REW + r] += sums[r, i]
            D[s, abi.QS_SUMM_D_TRUE_REWARD] += sums[i_main, i] + 1000.0 * sums[i_quadcol, i]
            D[c, abi.QS_SUMM_D_START_REW_POS] += sums[i_pos, i]
            D[c, abi.QS_SUMM_D_START_REW_CRASH] += sums[i_crash, i]
        count = float(steps[f]) * n
        for q in range(4):
            s1 = s2 = 0.0
            for i in range(f * n, (f + 1) * n):
                s1 += sums[abi.QS_SUM_ACT + q, i]
                s2 += sums[abi.QS_SUM_ACT2 + q, i]
            a1, a2 = s1 / count, s2 / count
            D[s, abi.QS_SUMM_D_ACT_MEAN + q] += a1
            D[s, abi.QS_SUMM_D_ACT_STD + q] += math.sqrt(max(a2 - a1 * a1, 0.0))
    return D, I


def flat(info):
    """{"true_reward", **episode_extra_stats} of one finished agent's info"""
    return {"true_reward": info["true_reward"], **info["episode_extra_stats"]}


class DictMean:
    """Collects per-agent dicts (flat()) and gives, per key the summary carries, the mean over the dicts that have it (math.fsum) and the
    bound of the module docstring.  n: agents per environment."""

    def __init__(self, n):
        self.n, self.vals, self.tr = n, {}, []

    def add(self, d):
        for k, v in d.items():
            if not left_out(k):
                self.vals.setdefault(k, []).append(float(v))
        self.tr.append(abs(d["true_reward"] - 1000.0 * d["rewraw_quadcol"]) + 1000.0 * abs(d["rewraw_quadcol"]) if "rewraw_quadcol" in d else 0.0)

    def mean(self):
        return {k: math.fsum(v) / len(v) for k, v in self.vals.items()}

    def bound(self, key):
        v = self.vals[key]
        m = len(v)
        if key in ("true_reward", "rewraw_main"):
            return (m + 2) * U * math.fsum(self.tr) / m
        if key.startswith("z_action") and key.endswith("_std"):
            a1 = self.vals[key[:-3] + "mean"]
            per = []
            for std, mu in zip(v, a1):
                d = (self.n + 3) * U * (std * std + 2.0 * mu * mu)     # a2 + a1^2 with a2 = std^2 + a1^2
                per.append(min(math.sqrt(d), d / std) if std > 0.0 else math.sqrt(d))
            return math.fsum(per) / m
        return (m + 2) * U * math.fsum(abs(x) for x in v) / m


def compare(summary, dm, report=None):
    """key sets equal, every value within its bound; returns the worst |error| / bound.  report: a list that receives (key, error, bound)"""
    want = dm.mean()
    got_keys = {k for k in summary if not is_count(k)}
    assert got_keys == set(want), f"key sets differ: {sorted(got_keys ^ set(want))}"
    worst = 0.0
    for k in sorted(want):
        err, bound = abs(summary[k] - want[k]), dm.bound(k)
        if report is not None:
            report.append((k, err, bound))
        assert err <= bound, f"{k}: {summary[k]!r} vs the mean of the dicts {want[k]!r}: |error| {err:.3e} above the bound {bound:.3e}"
        worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst

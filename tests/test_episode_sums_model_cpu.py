"""tests/episode_sums_model.py (the definition the device's `episode_sums` are held against in tests/test_episode_sums_gpu.py) against
the REFERENCE wrapper's records, and the inputs of that GPU file against what they must be able to show.  CPU only: model, oracle, fixtures.

1. Every fixture that recorded what QuadsRewardShapingWrapper did (tests/golden/wrapper_real_env_*.npz over the real env: per-step
   infos[i]['rewards'], done flags, episode-end dicts; wrapper_reward_shaping.json over the scripted env of tests/fake_env.py, whose
   per-step terms are a function of (seed, step) and are regenerated here) is replayed through the model: its `rew*` sums, `true_reward`
   and `z_action*_mean/_std` are the reference's to 1e-9.
2. The case list and the action generator of the GPU file, on the oracle alone: all 25 rows move, two episodes per environment end, actions
   leave [-1, 1], done flags differ inside a workgroup in the staggered case, episode ends fall on the first, the last and an inner step
   of a multi-step launch.
3. Twelve wrong versions of the bookkeeping are each OUTSIDE the float32 bound (the wider of the two) somewhere on those inputs - a wrong
   kernel of that kind cannot pass the GPU file."""
import functools
import json
import os

import numpy as np
import pytest

from tests import episode_sums_cases as esc
from tests import episode_sums_model as esm
from tests import golden_util as gu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("rew_main", "rew_pos", "rew_action", "rew_crash", "rew_orient", "rew_spin", "rewraw_main", "rewraw_pos", "rewraw_action",
        "rewraw_crash", "rewraw_orient", "rewraw_spin", "rew_quadcol", "rew_proximity", "rewraw_quadcol", "rew_quadcol_obstacle",
        "rewraw_quadcol_obstacle")


def check_end(model, e, n, true_reward, extra, where):
    st = esm.episode_stats(model.ep[:, e * n:(e + 1) * n], model.ep_actions[e])
    checked = 0
    for i in range(n):
        assert st["true_reward"][i] == pytest.approx(true_reward[i], rel=1e-9, abs=1e-9), f"{where} agent {i} true_reward"
        for q, key in enumerate(KEYS):
            if key in extra[i]:
                assert st["rew"][q, i] == pytest.approx(extra[i][key], rel=1e-9, abs=1e-9), f"{where} agent {i} {key}"
                checked += 1
        for k in range(4):
            assert st["mean"][k] == pytest.approx(extra[i][f"z_action{k}_mean"], rel=1e-9, abs=1e-9), f"{where} agent {i} mean {k}"
            assert st["std"][k] == pytest.approx(extra[i][f"z_action{k}_std"], rel=1e-9, abs=1e-9), f"{where} agent {i} std {k}"
    assert checked >= 15 * n


@pytest.mark.parametrize("name", ["wrapper_real_env_c2_annealed", "wrapper_real_env_c3_obst", "wrapper_real_env_mix"])
def test_model_equals_the_reference_wrapper_over_the_real_env(name):
    g, cfgd = gu.load(name)
    ends = {e["step"]: e for e in json.loads(str(g["ends"]))}
    n = cfgd["num_agents"]
    model = esm.EpisodeSums(1, n)
    seen = 0
    for t in range(g["actions"].shape[0]):
        model.step(g["actions"][t][None], g["rew_info"][t][None], g["done"][t][None])
        assert bool(g["done"][t].any()) == (t in ends)
        if t in ends:
            check_end(model, 0, n, ends[t]["true_reward"], ends[t]["extra"], f"{name} step {t}")
            assert not model.run.any()
            seen += 1
    assert seen >= 2


@pytest.mark.parametrize("case,seed", [("annealed", 1), ("plain", 2)])
def test_model_equals_the_reference_wrapper_over_the_scripted_env(case, seed):
    from tests.fake_env import FakeQuadEnv
    want = json.load(open(os.path.join(GOLDEN, "wrapper_reward_shaping.json")))[case]
    env = FakeQuadEnv(seed=seed)
    n = env.num_agents
    rng = np.random.RandomState(seed + 555)            # fake_env.drive(): the script the reference wrapper was recorded on
    model = esm.EpisodeSums(1, n)
    seen = 0
    for t, rec in enumerate(want["steps"]):
        act = np.stack([rng.uniform(-1, 1, 4) for _ in range(n)])
        _, rewards, dones, infos = env.step(list(act))
        assert rewards == pytest.approx(rec["rewards"], abs=1e-12) and [bool(d) for d in dones] == rec["dones"]
        ri = np.array([[info["rewards"].get(k, 0.0) for k in KEYS] for info in infos])
        model.step(act[None], ri[None], np.array(dones)[None])
        if dones[0]:
            check_end(model, 0, n, rec["true_reward"], rec["extra"], f"{case} step {t}")
            seen += 1
    assert seen == 4


# ---- the inputs of the GPU file, on the oracle alone ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def trace(name, variant):
    """the oracle-fed model over one input of the GPU file: per item (kind, t, actions, done, rew_info, run, ep, allowed run, allowed ep) with the
    float32 teacher-forced bound"""
    cfg = esc.config_of(name)
    oenvs = esc.make_oracles(cfg)
    kw = {"plain": {}, "staggered": dict(resets=esc.RESETS), "coeffs": dict(coeff_step=esc.COEFF_STEP), "coeffs_late": dict(coeff_step=esc.COEFF_STEP + 1),
          "many": dict(event_t=esc.many_event_t(name))}[variant]
    steps = esc.many_steps(name) if variant == "many" else esc.STEPS[name]
    out = []
    for item in esc.oracle_rollout(cfg, oenvs, steps, **kw):
        m = item[-1]
        snap = (m.run.copy(), m.ep.copy(), m.allowed("run", 1e-5, esm.U32), m.allowed("ep", 1e-5, esm.U32))
        out.append(item[:-1] + snap if item[0] == "step" else (item[0], item[1], item[2], None, None) + snap)
    for o in oenvs:
        o.close()
    return cfg.num_envs, cfg.num_agents, out


def test_every_row_moves_and_episodes_end():
    moved = np.zeros(esm.COUNT, dtype=bool)
    for name in esc.CASES:
        E, N, items = trace(name, "plain")
        ends = np.zeros(E, dtype=int)
        wild = False
        for kind, t, act, done, ri, run, ep, _, _ in items:
            fin = done.reshape(-1) != 0
            moved |= (ep[:, fin] != 0).any(axis=1)
            ends += done.any(axis=1)
            wild = wild or bool((np.abs(act) > 1.0).any())
        assert ends.min() >= 2, f"{name}: an environment finished {ends.min()} episodes"
        assert wild, f"{name}: no action component outside [-1, 1]"
    assert moved.all(), f"rows that are zero in every finished episode: {np.nonzero(~moved)[0].tolist()}"
    # one case alone moves all 17 term rows
    _, _, items = trace("c3_n8_obst_short", "plain")
    rows = np.zeros(esm.RI, dtype=bool)
    for it in items:
        rows |= (it[6][:esm.RI] != 0).any(axis=1)
    assert rows.all()


def test_staggered_case_has_mixed_done_flags_inside_a_workgroup():
    E, N, items = trace("c2_n8_dw", "staggered")
    per_wg = 64 // N
    mixed = 0
    for it in items:
        if it[0] == "step":
            d = it[3].any(axis=1)
            for w in range(0, E, per_wg):
                mixed += int(d[w:w + per_wg].any() and not d[w:w + per_wg].all())
    assert mixed >= 4
    assert sum(1 for it in items if it[0] == "reset") == 2


def test_multi_step_schedule_puts_episode_ends_on_first_last_and_inner_steps():
    where = set()
    for name in ("c2_n8_dw", "c3_n8_obst_short", "s_mix"):
        for it in trace(name, "many")[2]:
            lead = esc.MANY_LEAD.get(name, 0)
            if it[3].any() and it[1] >= lead:
                k = (it[1] - lead) % esc.MANY_K
                where.add("first" if k == 0 else "last" if k == esc.MANY_K - 1 else "inner")
    assert where == {"first", "last", "inner"}


# ---- wrong versions of the bookkeeping ------------------------------------------------------------------------------------------------------

class LastStepLeftOut(esm.EpisodeSums):
    def accumulate(self, add, fin):
        left_out = self.run[:, fin].copy()
        super().accumulate(add, fin)
        self.ep[:, fin] = left_out


class RunNotZeroed(esm.EpisodeSums):
    def accumulate(self, add, fin):
        v = self.run + add
        self.ep[:, fin] = v[:, fin]
        self.run = v


class DoneStepCountedTwice(esm.EpisodeSums):
    def accumulate(self, add, fin):
        super().accumulate(add, fin)
        self.run[:, fin] = add[:, fin]


class ClippedActions(esm.EpisodeSums):
    def addends(self, actions, rew_info):
        return super().addends(np.clip(actions, -1.0, 1.0), rew_info)


class PreviousActions(esm.EpisodeSums):
    def addends(self, actions, rew_info):
        prev, self.prev = getattr(self, "prev", np.zeros_like(actions)), np.array(actions)
        return super().addends(prev, rew_info)


class NextRingSlot(esm.EpisodeSums):
    """the ring holds the last RING_LEN batches; slot (t + 1) % RING_LEN is the oldest of them"""
    def addends(self, actions, rew_info):
        if not hasattr(self, "ring"):
            self.ring, self.t = [np.zeros_like(actions) for _ in range(esc.RING_LEN)], 0
        self.ring[self.t % esc.RING_LEN] = np.array(actions)
        got = self.ring[(self.t + 1) % esc.RING_LEN]
        self.t += 1
        return super().addends(got, rew_info)


class SquareKeepsSign(esm.EpisodeSums):
    def addends(self, actions, rew_info):
        add = super().addends(actions, rew_info)
        a = np.asarray(actions).reshape(self.T, 4)
        add[esm.ACT2:] = (a * np.abs(a)).T
        return add


class RawRowsExchanged(esm.EpisodeSums):
    PERM = list(range(6, 12)) + list(range(0, 6)) + [14, 13, 12, 16, 15]

    def addends(self, actions, rew_info):
        return super().addends(actions, np.asarray(rew_info)[..., self.PERM])


class NeighbourColumnsAfterAutoReset(esm.EpisodeSums):
    def accumulate(self, add, fin):
        if getattr(self, "shifted", False):
            add = np.roll(add, self.N, axis=1)
        self.shifted = getattr(self, "shifted", False) or bool(fin.any())
        super().accumulate(add, fin)


class ResetLeavesRun(esm.EpisodeSums):
    def zero_run(self, cols):
        pass


class ResetCopiesRunToEp(esm.EpisodeSums):
    def zero_run(self, cols):
        self.ep[:, cols] = self.run[:, cols]
        super().zero_run(cols)


MUTANTS = [(LastStepLeftOut, "plain"), (RunNotZeroed, "plain"), (DoneStepCountedTwice, "plain"), (ClippedActions, "plain"),
           (PreviousActions, "plain"), (NextRingSlot, "plain"), (SquareKeepsSign, "plain"), (RawRowsExchanged, "plain"),
           (NeighbourColumnsAfterAutoReset, "plain"), (ResetLeavesRun, "staggered"), (ResetCopiesRunToEp, "staggered")]


def excess_of(cls, name, variant, feed_from=None):
    """max |wrong model - model| / allowed over steps, rows and columns of one input (inf where nothing is allowed)"""
    E, N, items = trace(name, variant)
    feed = trace(name, feed_from)[2] if feed_from else items
    mut = cls(E, N)
    worst = 0.0
    for it, src in zip(items, feed):
        assert it[0] == src[0] and it[1] == src[1]
        if it[0] == "reset":
            mut.reset(it[2])
        else:
            mut.step(src[2], src[4], it[3])
        for got, ref, allowed in ((mut.run, it[5], it[7]), (mut.ep, it[6], it[8])):
            err = np.abs(got - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err > 0, err / allowed, 0.0)
            worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("cls,variant", MUTANTS, ids=[m[0].__name__ for m in MUTANTS])
def test_wrong_bookkeeping_is_outside_the_bound(cls, variant):
    names = ["c2_n8_dw"] if variant != "plain" else list(esc.CASES)
    worst = {name: excess_of(cls, name, variant) for name in names}
    assert max(worst.values()) > 1.0, f"{cls.__name__} stays inside the bound on every input: {worst}"
    if variant == "plain":      # ... and on the case every path of the GPU file runs
        assert worst["c2_n8_dw"] > 1.0, worst


def test_a_coefficient_update_one_step_late_is_outside_the_bound():
    """the model fed the reward terms of an oracle whose set_reward_coeffs came one step late, held against the one updated on time"""
    assert excess_of(esm.EpisodeSums, "c2_n8_dw", "coeffs", feed_from="coeffs_late") > 1.0

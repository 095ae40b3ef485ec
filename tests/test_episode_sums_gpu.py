"""The device's per-episode sums (`episode_sums=1`: run_sums / ep_sums, 25 rows per drone) on every step path, against
tests/episode_sums_model.py fed with the ORACLE's reward terms and done flags - never the kernel's own rew_info, which the production
combination (`write_rew_info=False`) does not even write.

Paths (the handle's flavour asserted by flag and kernel name; a multi-step launch by the conditions under which the library makes one):
one launch per step - specialised and generic objects, team and single-wave kernels, float64 free-running and float32 teacher-forced;
explicit masked resets in mid-episode, after which the done flags inside a workgroup differ; a coefficient update in mid-episode;
qs_step_many (registers carried across steps and auto-resets of a launch; float32 also in two-step launches forced from the oracle in
front of every launch, all rows against the model); qs_step_gated (actions from the gate's ring); a captured rollout segment; one full 1501-step float32 episode through EpisodeInfoBuilder.

The bound is derived (tests/episode_sums_model.py allowed()): per row, n steps into an episode,
    sum_t tol_step * max(1, |x_t|) + (n - 1) * u * max_t |partial_t|
tol_step = the per-step bound the parity suite asserts for reward terms (1e-5 teacher-forced float32, 1e-8 free-running float64; 0 for the
actions, u * a^2 for their squares), u = 2^-24 / 2^-53.  tests/test_episode_sums_model_cpu.py shows that twelve wrong versions of the
bookkeeping are outside it on these inputs.  QS_SUMS_REPORT=<path>: the worst |err| / allowed per (path, row group) is written there."""
import os
import time

import numpy as np
import pytest

from tests import episode_sums_cases as esc
from tests import episode_sums_model as esm
from tests import test_hip_parity as thp
from tests import tolerances as tolr

pytestmark = pytest.mark.gpu

GROUPS = (("terms", slice(0, esm.RI)), ("sum_a", slice(esm.ACT, esm.ACT2)), ("sum_a2", slice(esm.ACT2, esm.COUNT)))
PREC = {"f64": (1e-8, esm.U64), "f32": (1e-5, esm.U32)}
WORST, NOTES = {}, []


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0, n0 = time.perf_counter(), len(NOTES)
    yield
    path = os.environ.get("QS_SUMS_REPORT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("worst |device - model| / allowed per (path, row group); allowed = sum_t tol_step * max(1, |x_t|) + (n - 1) * u * max|partial|\n")
            for (where, group), v in sorted(WORST.items()):
                f.write(f"{where:58s} {group:8s} {v:.4f}\n")
            for line in NOTES[n0:]:
                f.write(line + "\n")
            f.write(f"wall time of the file: {time.perf_counter() - t0:.1f} s\n")


def record(path, group, ratio):
    WORST[(path, group)] = max(WORST.get((path, group), 0.0), float(ratio))


def ratio_of(got, ref, allowed):
    """|got - ref| / allowed; 0 where both are 0, inf where nothing is allowed or the device's value is not finite"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = err / allowed
    ratio[(err == 0) & (allowed == 0)] = 0.0
    ratio[~np.isfinite(err)] = np.inf
    return ratio


def check_sums(hip, model, precision, path, where, groups=("terms", "sum_a", "sum_a2"), which=("run", "ep")):
    tol_step, u = PREC[precision]
    for w in which:
        got, ref = hip.to_host(w + "_sums"), getattr(model, w)
        ratio = ratio_of(got, ref, model.allowed(w, tol_step, u))
        for name, rows in GROUPS:
            if name in groups:
                r = ratio[rows]
                record(path, name, r.max())
                if r.max() > 1.0:
                    q, col = np.unravel_index(int(np.argmax(r)), r.shape)
                    q += rows.start
                    raise AssertionError(f"{path} {where}: {w}_sums row {q} column {col} (env {col // model.N}): device {got[q, col]!r}, model {ref[q, col]!r}, "
                                         f"|err| / allowed = {r.max():.3g}; {int((r > 1).sum())} elements over their bound")


def assert_flavour(st, spec, team, precision, full=False):
    real = "double" if precision == "f64" else "float"
    assert bool(st.team) == team, f"asked for team={team}, the handle runs team={st.team}"
    assert bool(st.specialized) == spec, st.spec_note
    want = "qs_spec_step" if spec else ("qs_step_team" if team else "qs_step_kernel") + ("_full" if full else "") + f"<{real}>"
    assert st.kernel_name == want, (st.kernel_name, want)
    assert st.cfg.episode_sums == 1


class Device:
    """the device side of esc.oracle_rollout: one or more handles that are told the same things"""

    def __init__(self, hips, teacher_forced):
        self.hips, self.teacher_forced = hips, teacher_forced
        self.reset_checks, self.lifted = 0, 0

    def note_lift(self, t, e, drones):
        self.lifted += len(drones)

    def set_state(self, e, s, tick):
        for h in self.hips:
            h.set_state(e, s, tick)

    def set_reward_coeffs(self, vec):
        for h in self.hips:
            h.set_reward_coeffs(vec)

    def reset(self, mask):
        """qs_reset(env_mask) zeroes the running sums of the masked environments, and only those; ep_sums stays (qs_reset.h)"""
        for h in self.hips:
            h.sync()
            run0, ep0 = h.to_host("run_sums"), h.to_host("ep_sums")
            h.reset(mask)
            h.sync()
            run1, ep1 = h.to_host("run_sums"), h.to_host("ep_sums")
            cols = np.repeat(np.asarray(mask) != 0, h.N)
            assert run0[:, cols].any(), "nothing had been accumulated in the environments that are reset"
            assert not run1[:, cols].any(), "run_sums of a reset environment is not zero"
            np.testing.assert_array_equal(run1[:, ~cols], run0[:, ~cols], err_msg="a masked reset touched another environment's run_sums")
            np.testing.assert_array_equal(ep1, ep0, err_msg="a reset touched ep_sums")
            self.reset_checks += 1


def make_pair(name, precision, monkeypatch, spec=True, team=True, E=None, **over):
    case, case_over, case_E = esc.CASES[name]
    monkeypatch.setenv("QS_SPEC", "jit" if spec else "off")
    if team:
        monkeypatch.delenv("QS_TEAM", raising=False)
    else:
        monkeypatch.setenv("QS_TEAM", "0")
    pr = thp.Pair(case, E or case_E, precision, **dict(case_over, **dict(esc.SUMS_KW, **over)))
    assert_flavour(pr.hip, spec, team, precision, full=case.startswith("s_"))
    pr.reset()
    assert not pr.hip.to_host("run_sums").any() and not pr.hip.to_host("ep_sums").any()
    return pr


def run_stepwise(name, precision, monkeypatch, spec=True, team=True, rew_info=False, path=None, **schedule):
    """one launch per control step (qs_step): float64 free-running, float32 teacher-forced; run_sums and ep_sums after EVERY step, all 25 rows"""
    pr = make_pair(name, precision, monkeypatch, spec, team, **(dict(write_rew_info=True) if rew_info else {}))
    hip = pr.hip
    path = path or f"step {'spec' if spec else 'generic'} {'team' if team else 'single-wave'} {precision}"
    dev = Device([hip], teacher_forced=precision == "f32")
    ends = 0
    for item in esc.oracle_rollout(pr.cfg, pr.oenvs, esc.STEPS[name], device=dev, **schedule):
        if item[0] == "reset":
            check_sums(hip, item[-1], precision, path, f"{name} after the reset in front of step {item[1]}")
            continue
        _, t, act, done, ri, model = item
        hip.from_host("actions", act.reshape(-1, 4))
        hip.step()
        hip.sync()
        np.testing.assert_array_equal(hip.to_host("done").reshape(pr.E, pr.N), done, err_msg=f"{name} done step {t}")
        if rew_info:
            got = thp.soa(hip.to_host("rew_info"), pr.E, pr.N)
            tolr.check(f"{name} {precision} sums", "rew_info", got, ri, tolr.allowed_rel(ri, PREC[precision][0]), f"step {t}")
        check_sums(hip, model, precision, path, f"{name} step {t}")
        ends += int(done.any())
    assert ends >= 2 and model.episodes.min() >= (1 if schedule.get("resets") else 2)
    hip.check_errors()
    pr.close()
    return dev


FOUR = [(s, t) for s in (True, False) for t in (True, False)]
STEPWISE = [(n, s, t) for n in ("c2_n8_dw", "c3_n8_obst_short") for s, t in FOUR] + \
           [(n, True, t) for n in ("c1_single", "e_n33_k8", "e_n64_k6", "s_mix") for t in (True, False)]
IDS = [f"{n}-{'spec' if s else 'generic'}-{'team' if t else 'single'}" for n, s, t in STEPWISE]


@pytest.mark.parametrize("name,spec,team", STEPWISE, ids=IDS)
def test_one_launch_per_step_f32_teacher_forced(name, spec, team, monkeypatch):
    run_stepwise(name, "f32", monkeypatch, spec, team)


@pytest.mark.parametrize("name,spec,team", [c for c in STEPWISE if not (c[2] and c[0].startswith("e_"))],
                         ids=[i for i, c in zip(IDS, STEPWISE) if not (c[2] and c[0].startswith("e_"))])
def test_one_launch_per_step_f64_free_running(name, spec, team, monkeypatch):
    """(more than 8 drones: the float64 team layout does not fit the LDS of a workgroup - single-wave only)"""
    run_stepwise(name, "f64", monkeypatch, spec, team)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_sums_do_not_depend_on_write_rew_info(precision, monkeypatch):
    """the twin with write_rew_info=True: the same sums, and its rew_info is the oracle's per step (what the bound's tol_step assumes)"""
    run_stepwise("c2_n8_dw", precision, monkeypatch, rew_info=True, path=f"step spec team {precision} +rew_info")


@pytest.mark.parametrize("team", [True, False], ids=["team", "single"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_masked_resets_in_mid_episode_and_staggered_episode_ends(precision, team, monkeypatch):
    """qs_reset(env_mask) over environments {1, 4, 9} in front of step 7 and {0, 9} in front of step 31, on device, oracle and model: the masked
    environments' run_sums are zero after the reset launch, everything else is untouched (Device.reset), and from then on the episodes of
    one workgroup end on different steps - the per-lane `fin` is neither all-true nor all-false.  The oracle's explicit reset follows the
    device's draw-counter rule (include/quadswarm.h: qs_reset), so float64 stays free-running across the resets."""
    dev = run_stepwise("c2_n8_dw", precision, monkeypatch, team=team, path=f"step+resets spec {'team' if team else 'single-wave'} {precision}", resets=esc.RESETS)
    assert dev.reset_checks == 2


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_coefficient_update_in_mid_episode(precision, monkeypatch):
    """qs_set_reward_coeffs in front of step 12 (the annealing path of reward_shaping.py:111-118): the sums of that episode hold the old
    coefficients' terms up to step 11 and the new ones' from step 12"""
    run_stepwise("c2_n8_dw", precision, monkeypatch, path=f"step+coeffs spec team {precision}", coeff_step=esc.COEFF_STEP)


# ---- qs_step_many ---------------------------------------------------------------------------------------------------------------------------

def _table(acts, precision):
    import torch
    a = np.stack(acts).reshape(len(acts), -1, 4)
    return torch.as_tensor(a, dtype=torch.float64 if precision == "f64" else torch.float32).cuda().contiguous()


def same_rule(got, ref, what):
    """tests/test_gated_gpu.py::_same for float32: 2e-3 * (1 + max|x|)"""
    tol = 2e-3 * (1.0 + np.abs(ref).max())
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
    assert err <= tol, f"{what} differs by {err} (allowed {tol})"
    return err / tol


def run_many(name, precision, monkeypatch, team):
    """MANY_LAUNCHES launches of MANY_K steps (behind MANY_LEAD plain steps): the 25 sums live in registers across the steps and auto-resets of
    a launch.  float64: all rows against the oracle-fed model after every launch.  float32 (free-running, so its trajectory is its own): the
    action rows against the model - they depend on the actions and done flags only -, the term rows against a one-launch-per-step handle."""
    import torch
    pr = make_pair(name, precision, monkeypatch, True, team)
    hips = [pr.hip]
    if precision == "f32":
        from quad_swarm_rl_amd import native
        twin = native.Stepper(pr.cfg, device=0)
        assert_flavour(twin, True, team, precision, full=name.startswith("s_"))
        twin.reset()
        hips.append(twin)
    path = f"step_many spec {'team' if team else 'single-wave'} {precision}"
    lead, K = esc.MANY_LEAD.get(name, 0), esc.MANY_K
    pending, launches, ends_at = [], 0, set()
    for item in esc.oracle_rollout(pr.cfg, pr.oenvs, esc.many_steps(name), device=Device(hips, False), event_t=esc.many_event_t(name)):
        _, t, act, done, ri, model = item
        if done.any() and t >= lead:
            ends_at.add((t - lead) % K)
        pending.append(act)
        if t >= lead and len(pending) < K:
            continue
        table = _table(pending, precision)
        if t < lead:
            pr.hip.step(table.data_ptr())
        else:
            multi_step_launch(pr.hip, table, len(pending))
            launches += 1
        for a in (pending if len(hips) > 1 else []):
            hips[1].from_host("actions", a.reshape(-1, 4))
            hips[1].step()
        torch.cuda.synchronize()
        pending = []
        np.testing.assert_array_equal(pr.hip.to_host("done").reshape(pr.E, pr.N), done, err_msg=f"{name} done step {t}")
        if precision == "f64":
            check_sums(pr.hip, model, precision, path, f"{name} after step {t}")
        else:
            check_sums(pr.hip, model, precision, path, f"{name} after step {t}", groups=("sum_a", "sum_a2"))
            for w in ("run_sums", "ep_sums"):
                r = same_rule(pr.hip.to_host(w)[:esm.RI], hips[1].to_host(w)[:esm.RI], f"{name} after step {t}: term rows of {w} against one launch per step")
                record(path + " vs stepwise (2e-3 rule)", "terms", r)
    assert launches == esc.MANY_LAUNCHES and model.episodes.min() >= 1
    for h in hips:
        h.check_errors()
    if len(hips) > 1:
        hips[1].close()
    pr.close()
    return ends_at


@pytest.mark.parametrize("team", [True, False], ids=["team", "single"])
def test_step_many_f64(team, monkeypatch):
    where = set()
    for name in ("c2_n8_dw", "c3_n8_obst_short", "s_mix"):
        where |= run_many(name, "f64", monkeypatch, team)
    assert {0, esc.MANY_K - 1} <= where and len(where) > 2     # episode ends on the first, the last and inner steps of a launch


@pytest.mark.parametrize("name", ["c2_n8_dw", "e_n33_k8"])
@pytest.mark.parametrize("team", [True, False], ids=["team", "single"])
def test_step_many_f32(name, team, monkeypatch):
    run_many(name, "f32", monkeypatch, team)


def multi_step_launch(hip, table, k):
    """qs_step_many launches the multi-step (QS_MULTI) instantiation when k >= 2 and nothing makes it fall back to one launch per step
    (profiling, the replay wrapper, an observation exchange: quadswarm_hip.hip, qs_step_many / launch_step).  The ABI does not name the kernel
    of a multi-step launch, so the conditions are what can be asserted."""
    assert k >= 2 and table.shape[0] == k and not getattr(hip, "replay_on", False)
    hip.step_many(table.data_ptr(), k)


@pytest.mark.parametrize("name", ["c2_n8_dw", "e_n33_k8"])
@pytest.mark.parametrize("team", [True, False], ids=["team", "single"])
def test_step_many_two_step_launches_f32_against_the_oracle(name, team, monkeypatch):
    """The float32 multi-step instantiation against the oracle-fed model, all 25 rows: launches of k = 2, the oracle's state forced in front of
    every launch, so every launch loads the sums at its top, carries them in registers over one step boundary (and over the auto-resets that
    fall on a launch's first or second step) and stores them at its end.  The first step of a launch is a teacher-forced step (1e-5); the second
    starts from the device's own state and counts with the free-running envelope the parity suite asserts, 3 x (esc.FREE_STEP_SCALE)."""
    import torch
    K = 2
    pr = make_pair(name, "f32", monkeypatch, True, team)
    hip = pr.hip
    path = f"step_many k=2 forced per launch spec {'team' if team else 'single-wave'} f32"
    pending, ends_at = [], set()
    gen = esc.oracle_rollout(pr.cfg, pr.oenvs, esc.STEPS[name], device=Device([hip], True), force_every=K,
                             event_t=lambda t: t if t % K == 0 else None)
    for _, t, act, done, ri, model in gen:
        pending.append(act)
        if done.any():
            ends_at.add(t % K)
        if len(pending) < K:
            continue
        multi_step_launch(hip, _table(pending, "f32"), K)
        torch.cuda.synchronize()
        pending = []
        np.testing.assert_array_equal(hip.to_host("done").reshape(pr.E, pr.N), done, err_msg=f"{name} done step {t}")
        check_sums(hip, model, "f32", path, f"{name} after step {t}")
    # episode ends on a launch's second step in both cases (26- and 11-step episodes), on its first step too with the 11-step ones
    assert 1 in ends_at and (name != "e_n33_k8" or 0 in ends_at) and model.episodes.min() >= 2
    hip.check_errors()
    pr.close()


# ---- qs_step_gated --------------------------------------------------------------------------------------------------------------------------

GATE_E, GATE_K, GATE_LAUNCHES = 40, 24, 3
GATE_EVENT_T = {0: None, GATE_K: 6, GATE_K + 1: 22, 2 * GATE_K + 1: 14}     # states forced between launches only


@pytest.mark.parametrize("precision,closed_loop", [("f64", True), ("f32", False)])
def test_gated_launches(precision, closed_loop, monkeypatch):
    """qs_step_gated takes the four actions of the sums from the gate's ring, slot (sequence number) % ring_len - every other kernel reads the
    `actions` argument.  ring_len 8, K = 24 steps per launch: every slot is reused three times per launch; a plain step between launches.
    float64 closed loop: all rows against the oracle-fed model.  float32 running ahead: action rows against the model (a wrong slot is an
    O(1) difference), term rows against qs_step_many on a twin handle."""
    import torch
    from quad_swarm_rl_amd import native
    pr = make_pair("c2_n8_dw", precision, monkeypatch, E=GATE_E)
    gated = pr.hip
    twin = native.Stepper(pr.cfg, device=0)
    twin.reset()
    gated.gate_create(ring_len=esc.RING_LEN, wg_per_group=2)
    info = gated.gate_info()
    assert info.ring_len == esc.RING_LEN and info.wg_per_group == 2 and info.envs_per_workgroup == 64 // pr.N
    side, feed = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    path = f"step_gated spec team {precision} {'closed loop' if closed_loop else 'running ahead'}"
    total = GATE_K * GATE_LAUNCHES + 1
    # launch boundaries: [0, K) gated, K plain, [K + 1, 2K + 1) gated, [2K + 1, 3K + 1) gated
    bounds = {GATE_K - 1: "gated", GATE_K: "plain", 2 * GATE_K: "gated", 3 * GATE_K: "gated"}
    pending, launched = [], 0
    for item in esc.oracle_rollout(pr.cfg, pr.oenvs, total, device=Device([gated, twin], False), event_t=lambda t: GATE_EVENT_T.get(t)):
        _, t, act, done, ri, model = item
        pending.append(act)
        if t not in bounds:
            continue
        table = _table(pending, precision)
        if bounds[t] == "plain":
            gated.step(table.data_ptr()); twin.step(table.data_ptr())
        else:
            gated.step_gated(len(pending), stream=side)
            gated.gate_produce(table.data_ptr(), len(pending), len(pending), closed_loop=closed_loop, stream=feed)
            gated.gate_wait(stream=side)
            multi_step_launch(twin, table, len(pending))
            launched += len(pending)
        torch.cuda.synchronize()
        pending = []
        st = gated.gate_status()
        assert st["error"] == 0 and st["min_done_flag"] == launched and st["min_act_flag"] == launched, st
        np.testing.assert_array_equal(gated.to_host("done").reshape(pr.E, pr.N), done, err_msg=f"done step {t}")
        if precision == "f64":
            check_sums(gated, model, precision, path, f"after step {t}")
        else:
            check_sums(gated, model, precision, path, f"after step {t}", groups=("sum_a", "sum_a2"))
            for w in ("run_sums", "ep_sums"):
                r = same_rule(gated.to_host(w)[:esm.RI], twin.to_host(w)[:esm.RI], f"after step {t}: term rows of {w} against qs_step_many")
                record(path + " vs step_many (2e-3 rule)", "terms", r)
    assert launched == GATE_K * GATE_LAUNCHES and model.episodes.min() >= 2
    gated.check_errors(); twin.check_errors()
    twin.close()
    pr.close()


# ---- a captured rollout segment -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("copying", [False, True], ids=["in_place", "copying_glue"])
def test_rollout_segment_accumulates_the_actions_it_sampled(copying):
    """GraphedRollout over an episode_sums env with 4-step episodes and a 6-step segment, its warm-up step and three replays: rows 17..24 of run_sums / ep_sums
    are the model's over the segment's RECORDED actions and done flags.  copying_glue: the path the replay wrapper selects (here with a
    sample probability of 0, so that no episode is restored from a checkpoint)."""
    import torch
    from quad_swarm_rl_amd import policy, rollout
    from quad_swarm_rl_amd.env import QuadSwarmVecEnv
    from tests import encoder_epilogue_cases as cases
    kw = dict(num_agents=cases.LOOP_AGENTS, neighbor_visible_num=6, neighbor_obs_type="pos_vel", use_numba=True, collision_falloff_radius=4.0,
              ep_time=0.03, episode_sums=True, write_rew_info=False)
    env = QuadSwarmVecEnv(cases.LOOP_ENVS, seed=5, **kw)
    st = env.stepper
    assert st.cfg.episode_sums == 1 and st.specialized and st.team
    if copying:
        st.replay_enable(0.0)
    env.reset()
    enc = policy.FusedQuadEncoder(policy.make_reference_encoder(seed=2, nbr_encoder="mean_embed").cuda())
    head = rollout.GaussianActionHead(sample=True, seed=cases.LOOP_SEED)
    seg = rollout.GraphedRollout(env, enc, head, steps=cases.LOOP_STEPS)
    assert seg._glue and seg._in_place == (not copying) and seg.graph is not None
    model = esm.EpisodeSums(st.E, st.N)
    zeros = np.zeros((st.E, st.N, esm.RI))
    path = f"rollout segment {'copying' if copying else 'in place'} f32"
    torch.cuda.synchronize()     # the constructor took ONE control step eagerly (its warm-up): recorded in slot 0, and in the sums
    model.step(seg.actions[0].double().cpu().numpy().reshape(st.E, st.N, 4), zeros, seg.dones[0].cpu().numpy().reshape(st.E, st.N))
    check_sums(st, model, "f32", path, "warm-up step", groups=("sum_a", "sum_a2"))
    for r in range(cases.LOOP_RUNS):
        out = {k: v.clone() for k, v in seg.run().items()}
        torch.cuda.synchronize()
        acts, dones = out["actions"].double().cpu().numpy(), out["dones"].cpu().numpy()
        assert (np.abs(acts) > 1.0).any()
        for t in range(cases.LOOP_STEPS):
            model.step(acts[t].reshape(st.E, st.N, 4), zeros, dones[t].reshape(st.E, st.N))
        check_sums(st, model, "f32", path, f"run {r}", groups=("sum_a", "sum_a2"))
    assert model.episodes.min() >= 3
    env.close()


# ---- one full-length episode ----------------------------------------------------------------------------------------------------------------

def test_full_length_episode_f32_through_the_episode_info_builder(monkeypatch):
    """c2_n8_dw at the default episode length (1501 control steps), 2 environments, float32 specialised team kernel, teacher-forced, gentle
    actions throughout: ep_sums against the model with the derived bound, then sf_env.EpisodeInfoBuilder on the DEVICE's sums against
    episode_stats() of the model with the bound pushed through the formulas - `true_reward`, every `rew*` key, `z_action*_mean/_std` -
    and a2 - a1^2 not clamped.  What float32 accumulation leaves of them over a real episode is measured here for the first time
    (profiles/r12_episode_sums_errors.txt).

    Near-hover actions leave the drones on the floor, lifting off by fractions of a micrometre and landing again, for the whole episode.  Without the
    floor margin of esc.oracle_rollout two of the 24016 drone-steps (step 292 env 1 drone 6, step 543 env 0 drone 1) missed the per-step 1e-5 in
    every floor-dependent term - the oracle lifted the drone by 1.1e-9 / 5.2e-10 m, less than ulp(0.046) = 3.7e-9 of the float32 height, and
    the kernel kept it on the floor (rew_orient -0.005 instead of +0.005) - which put run_sums 3.3 x outside the derived bound: a gap in the
    teacher-forcing conditions ("where fp32 cannot follow"), not in the sums.  The margin moves every lift-off from rest of less
    than 1e-6 m (244 drone-steps of this episode, not only those two) to 1e-4 m above the floor: those steps are not floor-rest steps any more."""
    from quad_swarm_rl_amd import config as qcfg, sf_env
    monkeypatch.setenv("QS_SPEC", "jit")
    monkeypatch.delenv("QS_TEAM", raising=False)
    E = 2
    pr = thp.Pair("c2_n8_dw", E, "f32", **esc.SUMS_KW)
    hip, N = pr.hip, pr.N
    assert_flavour(hip, True, True, "f32")
    steps = pr.cfg.ep_len + 1
    assert steps == 1501
    pr.reset()
    path = "full episode spec team f32"
    dev = Device([hip], True)
    for item in esc.oracle_rollout(pr.cfg, pr.oenvs, steps, device=dev, gentle_only=True, events=False):
        _, t, act, done, ri, model = item
        hip.from_host("actions", act.reshape(-1, 4))
        hip.step()
        hip.sync()
        if t % 100 == 99 or t == steps - 1:
            np.testing.assert_array_equal(hip.to_host("done").reshape(E, N), done, err_msg=f"done step {t}")
            check_sums(hip, model, "f32", path, f"step {t}", which=("run",))
    assert done.all() and (model.ep_n == steps).all()
    NOTES.append(f"full float32 episode: {dev.lifted} of {steps * E * N} drone-steps did not start at rest on the floor but from the margin "
                 "above it (a lift-off from rest of less than 1e-6 m: esc.oracle_rollout)")
    check_sums(hip, model, "f32", path, "episode end")
    sums = hip.to_host("ep_sums").astype(np.float64)
    b = sf_env.EpisodeInfoBuilder(list(range(E)), N, sums, hip.to_host("ep_stats").astype(np.float64), hip.to_host("ep_counters"), hip.to_host("ep_scenario"),
                                  None, None, None, 0, qcfg.REW_INFO_KEYS, False, steps, [])
    err = model.allowed("ep", *PREC["f32"])
    count = float(steps * N)
    a1 = sums[esm.ACT:esm.ACT2].reshape(4, E, N).sum(axis=2) / count
    a2 = sums[esm.ACT2:].reshape(4, E, N).sum(axis=2) / count
    assert (a2 - a1 * a1 > 0).all(), "a2 - a1^2 <= 0: the builder's max(..., 0) clamped a cancellation"
    worst = {}
    for e in range(E):
        cols = slice(e * N, (e + 1) * N)
        want = esm.episode_stats(model.ep[:, cols], model.ep_actions[e], err=err[:, cols])
        dicts = b.env_dicts(e)
        for i in range(N):
            ex = dicts[i]["episode_extra_stats"]
            items = [("true_reward", dicts[i]["true_reward"], want["true_reward"][i], want["err"]["true_reward"][i])]
            items += [(k, ex[k], want["rew"][q, i], want["err"]["rew"][q, i]) for q, k in enumerate(qcfg.REW_INFO_KEYS_NO_OBST)]
            for k in range(4):
                items.append(("z_action_mean", ex[f"z_action{k}_mean"], want["mean"][k], want["err"]["mean"][k]))
                items.append(("z_action_std", ex[f"z_action{k}_std"], want["std"][k], want["err"]["std"][k]))
            for key, got, ref, allowed in items:
                d = abs(float(got) - ref)
                ratio = 0.0 if d == 0 else d / allowed
                group = key if key.startswith(("true", "z_")) else "rew*"
                if ratio >= worst.get(group, (-1.0,))[0]:
                    worst[group] = (ratio, d, ref)
                assert ratio <= 1.0, f"env {e} agent {i} {key}: builder {got!r}, model {ref!r}, |err| / allowed = {ratio:.3g}"
    for group, (ratio, d, ref) in sorted(worst.items()):
        record(path + " stats", group, ratio)
        NOTES.append(f"full float32 episode ({steps} steps, {N} drones): worst {group}: |err| {d:.3e} at a value of {ref:.6g} ({ratio:.4f} of the bound)")
    rel = np.abs(sums - model.ep) / np.maximum(np.abs(model.ep), 1e-300)
    for name, rows in GROUPS:
        NOTES.append(f"full float32 episode: ep_sums {name}: worst |err| {np.abs(sums - model.ep)[rows].max():.3e}, worst relative {rel[rows][np.abs(model.ep[rows]) > 1e-3].max():.3e}")
    hip.check_errors()
    pr.close()

"""The device-side position controller (include/quadswarm_control.h, csrc/qs_pilot.hip) on the GPU: the kernel against the thrusts the reference's
NonlinearPositionController computed (tests/golden/pilot_mellinger.npz: all 1024 rows, both element orders of the state blocks, drone counts
that do and do not divide 64, both precisions), the raw-action form, the mask, the goal override, a closed loop flown by step_pilot, and the
same closed loop captured into a HIP graph.  Configurations of tests/test_hip_parity.py whose code objects `__graft_entry__.build()` prebuilds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pilot_model  # noqa: E402
import test_hip_parity as thp  # noqa: E402
from quad_swarm_rl_amd import config as qcfg  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"f64": 1e-9, "f32": 1e-5}     # |thrust - reference|: the project's float64 bound / the float32 rule of tests/tolerances.py
# (case of tests/test_hip_parity.py, QS_TEAM, environments, state_lane_major): N = 1, 8 (both element orders), 32, and 33 - which does not
# divide 64, 31 idle lanes per block; tests/test_state_layout_gpu.py: which handles are lane-major
HANDLES = [("c1_single", None, 1024, 1), ("c2_n8_dw", None, 128, 1), ("c2_n8_dw", "0", 128, 0), ("c4_n32_svs", None, 32, 0), ("e_n33_k8", None, 32, 0)]
# the closed loop: one drone per environment, no sensor noise, no thrust noise, no downwash (the settings the fixture's `closed_loop` was flown with)
LOOP_KW = dict(num_agents=1, neighbor_visible_num=0, neighbor_obs_type="none", use_numba=False, use_downwash=False, quads_mode="static_same_goal",
               sense_noise=None, thrust_noise_ratio=0.0, ep_time=15.0)


def fixture():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "pilot_mellinger.npz")))


@pytest.fixture(scope="module", params=[(h, p) for h in HANDLES for p in ("f32", "f64")], ids=lambda hp: f"{hp[0][0]}-team{hp[0][1]}-{hp[1]}")
def loaded(request):
    """a handle whose drones hold the fixture's rows (row index = global drone index modulo 1024: every row is used, by every handle)"""
    from quad_swarm_rl_amd import native
    (case, team, E, lane_major), precision = request.param
    mp = pytest.MonkeyPatch()
    if team is not None:
        mp.setenv("QS_TEAM", team)
    try:
        st = native.Stepper(qcfg.make_config(num_envs=E, seed=3, precision=precision, **thp.CASES[case]), device=0)
    finally:
        mp.undo()
    assert st.bufs.state_lane_major == lane_major, (case, team, st.bufs.state_lane_major)
    assert st.T >= 1024 and st.bufs.envs_per_block == 64 // st.N
    fx = fixture()
    rows = np.arange(st.T) % 1024
    st.reset()
    for e in range(st.E):
        st.set_state(e, fx["state"][rows[e * st.N:(e + 1) * st.N]])
    yield st, fx, rows, precision
    st.close()


def run(st, out=None, mask=None, goals=None, as_thrust=True):
    """one pilot launch; returns the [T, 4] result on the host (of the library's `actions` buffer, or of the torch tensor `out`)"""
    st.pilot_actions(out.data_ptr() if out is not None else None, mask.data_ptr() if mask is not None else None,
                     goals.data_ptr() if goals is not None else None, as_thrust=as_thrust)
    st.sync()
    return st.to_host("actions").copy() if out is None else out.cpu().numpy()


def test_kernel_against_the_reference(loaded):
    st, fx, rows, precision = loaded
    got = run(st)
    assert got.dtype == st.np_real and got.shape == (st.T, 4)
    err = np.abs(got.astype(np.float64) - fx["thrust"][rows])
    print(f"N={st.N} lane_major={st.bufs.state_lane_major} {precision}: max |thrust - reference| = {err.max():.3g} (bound {TOL[precision]:g}), "
          f"worst row {int(rows[err.max(axis=1).argmax()])}")
    assert err.max() <= TOL[precision]
    assert (got >= 0).all() and (got <= 1).all()


def test_raw_action_form(loaded):
    st, fx, rows, precision = loaded
    t = run(st, as_thrust=True)
    a = run(st, as_thrust=False)
    assert np.array_equal(a, st.np_real(2) * t - st.np_real(1))


def test_mask_leaves_the_other_rows_alone(loaded):
    import torch
    st, fx, rows, precision = loaded
    dt = torch.float64 if precision == "f64" else torch.float32
    full = run(st, as_thrust=False)
    pattern = (torch.arange(st.T * 4, device="cuda", dtype=dt).reshape(st.T, 4) * 0.37 - 11.0).contiguous()
    out = pattern.clone()
    mask = (torch.arange(st.T, device="cuda") % 2 == 0).to(torch.uint8)
    got = run(st, out=out, mask=mask, as_thrust=False)
    pat, m = pattern.cpu().numpy(), mask.cpu().numpy().astype(bool)
    assert np.array_equal(got[~m].view(np.uint8), pat[~m].view(np.uint8))     # bit for bit
    assert np.array_equal(got[m], full[m])
    none = run(st, out=pattern.clone(), mask=torch.zeros(st.T, device="cuda", dtype=torch.uint8), as_thrust=False)
    assert np.array_equal(none.view(np.uint8), pat.view(np.uint8))


def test_goal_override(loaded):
    import torch
    st, fx, rows, precision = loaded
    dt = torch.float64 if precision == "f64" else torch.float32
    state = fx["state"][rows]
    base = run(st)
    own = torch.as_tensor(state[:, 32:35].astype(st.np_real), device="cuda").contiguous()      # what qs_set_state put into the state
    assert np.array_equal(run(st, goals=own).view(np.uint8), base.view(np.uint8))
    rng = np.random.RandomState(17)
    other = rng.uniform([-5.0, -5.0, 0.0], [5.0, 5.0, 10.0], size=(st.T, 3)).astype(st.np_real)
    got = run(st, goals=torch.as_tensor(other, device="cuda", dtype=dt).contiguous())
    want = pilot_model.thrusts_of_state(state, fx["jinv"], goal=other.astype(np.float64), gravity=float(fx["gravity"]), x_des=fx["x_des"])
    acc, cx = pilot_model.guard_quantities(np.concatenate([state[:, :32], other.astype(np.float64)], axis=1), gravity=float(fx["gravity"]), x_des=fx["x_des"])
    assert min(acc.min(), cx.min()) > 1e-3, "a drawn goal sits on one of normalize()'s branches"
    err = np.abs(got.astype(np.float64) - want)
    print(f"N={st.N} {precision}: goal override, max |thrust - twin| = {err.max():.3g}")
    assert err.max() <= TOL[precision] and not np.array_equal(got, base)


def test_closed_loop_reaches_the_goal():
    """E = 1024 single-drone environments, float32: the even ones flown by step_pilot, the odd ones with their motors off.  After 1000 control
    steps every piloted drone is within 10 x the worst distance the REFERENCE controller left on the reference env at step 1000 (the fixture's
    closed_loop[2], >= 256 seeds): the factor covers other spawn draws, 1024 against 256 samples and float32 - the error shrinks about tenfold
    per 200 steps, so it is about 200 steps of slack.  Every motors-off drone lies on the floor, more than 0.5 m from its goal."""
    import torch
    from quad_swarm_rl_amd import env as qenv
    E = 1024
    ref_worst = fixture()["closed_loop"]
    venv = qenv.QuadSwarmVecEnv(E, seed=21, precision="f32", **LOOP_KW)
    venv.reset()
    act = torch.full((E, 4), -1.0, device="cuda")
    mask = (torch.arange(E, device="cuda") % 2 == 0).to(torch.uint8)
    done_any = torch.zeros((), device="cuda", dtype=torch.bool)
    for t in range(1000):
        _, _, done, _ = venv.step_pilot(actions=act, mask=mask)
        done_any |= done.ne(0).any()                           # dones are uint8, whose any() is uint8 too
    torch.cuda.synchronize()
    venv.stepper.check_errors()
    assert not bool(done_any)                                  # 15-second episodes: no reset inside the 1000 steps
    st = venv.stepper
    dist = np.linalg.norm(st.to_host("pos").astype(np.float64) - st.to_host("goal").astype(np.float64), axis=0)
    piloted = np.arange(E) % 2 == 0
    a = act.cpu().numpy()
    assert (a[~piloted] == -1.0).all() and (a[piloted] > -1.0).any()
    print(f"piloted: worst distance to the goal after 1000 steps {dist[piloted].max():.3g} m (reference worst {ref_worst[2]:.3g} m over {int(ref_worst[3])} seeds, "
          f"bound {10 * ref_worst[2]:.3g}); motors off: nearest to its goal {dist[~piloted].min():.3g} m")
    assert dist[piloted].max() <= 10.0 * ref_worst[2]
    on_floor = np.array([st.get_state(e)[0][0, 30] for e in range(1, E, 2)])
    assert (on_floor == 1.0).all() and (dist[~piloted] > 0.5).all()
    venv.close()


def test_graph_capture_replays_the_eager_run():
    """64 x (pilot launch, step launch) captured with torch.cuda.graph and replayed once = the same 64 steps issued eagerly: bit-identical state"""
    import torch
    from quad_swarm_rl_amd import env as qenv
    kw = dict(thp.CASES["c2_n8_dw"])
    final = {}
    for mode in ("eager", "graph"):
        venv = qenv.QuadSwarmVecEnv(8, seed=5, precision="f32", **kw)
        venv.reset()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            venv.step_pilot()                                  # library warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if mode == "eager":
            for _ in range(64):
                venv.step_pilot()
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(64):
                    venv.step_pilot()
            torch.cuda.synchronize()
            assert int(venv.stepper.to_host("tick")[0]) == 1   # capturing ran nothing
            g.replay()
        torch.cuda.synchronize()
        venv.stepper.check_errors()
        st = venv.stepper
        final[mode] = {n: st.to_host(n).copy() for n in ("pos", "vel", "rot", "omega", "goal", "tick", "actions", "obs", "reward")}
        venv.close()
    assert int(final["eager"]["tick"][0]) == 65
    for n, a in final["eager"].items():
        assert np.array_equal(a.view(np.uint8), final["graph"][n].view(np.uint8)), n


def test_refused_while_a_gated_launch_holds_the_state():
    import torch
    from quad_swarm_rl_amd import native
    cfg = qcfg.make_config(num_envs=40, seed=9, precision="f32", **dict(thp.CASES["c2_n8_dw"], ep_time=0.5))
    st = native.Stepper(cfg, device=0)
    assert st.team                                             # resident-state stepping lives in the team kernels
    st.reset()
    st.pilot_actions()
    K = 4
    table = (torch.rand((K, st.T, 4), device="cuda") * 2 - 1).contiguous()
    st.gate_create(ring_len=8, wg_per_group=2)
    side, feed = torch.cuda.Stream(), torch.cuda.Stream()
    st.step_gated(K, stream=side)
    st.gate_produce(table.data_ptr(), K, K, closed_loop=False, stream=feed)
    st.gate_wait(stream=side)
    with pytest.raises(native.QsError, match="gated launch"):
        st.pilot_actions()
    st.sync()
    torch.cuda.synchronize()
    st.pilot_actions()
    st.sync()
    assert st.gate_status()["error"] == 0
    st.close()

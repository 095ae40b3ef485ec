"""CPU-side checks of the device-side position controller (include/quadswarm_control.h): the NumPy twin of the kernel's arithmetic
(tests/pilot_model.py) against the thrusts the reference's NonlinearPositionController computed (tests/golden/pilot_mellinger.npz, captured by
tools/capture_pilot_fixture.py from gym_art/quadrotor_multi/quadrotor_control.py:282-330), the host-side parameter derivation against the
reference's inverse Jacobian, the exported symbols, and the properties the fixture promises to the GPU tests."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pilot_model  # noqa: E402
from quad_swarm_rl_amd import config as qcfg, native  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "pilot_mellinger.npz")))


def test_the_twin_reproduces_the_reference_controller(fx):
    """float64, all 1024 rows, nothing excluded: 1e-12 (a vectorised evaluation differs from the reference's per-drone one by the
    summation order of the 3- and 4-term dot products only)"""
    got = pilot_model.thrusts_of_state(fx["state"], fx["jinv"], gravity=float(fx["gravity"]), x_des=fx["x_des"])
    err = float(np.abs(got - fx["thrust"]).max())
    print("twin - reference, float64: max |diff| =", err)
    assert got.shape == (1024, 4) and err <= 1e-12
    f32 = pilot_model.thrusts_of_state(fx["state"], fx["jinv"], gravity=float(fx["gravity"]), x_des=fx["x_des"], dtype=np.float32)
    err32 = float(np.abs(f32.astype(np.float64) - fx["thrust"]).max())
    print("twin - reference, float32: max |diff| =", err32)
    assert f32.dtype == np.float32 and err32 <= 1e-5     # the float32 rule of tests/tolerances.py


def test_default_params_are_the_references(fx):
    cfg = qcfg.make_config(num_envs=2, num_agents=8)
    p = native.pilot_default_params(cfg)
    np.testing.assert_allclose(np.array(p.jinv), fx["jinv"], rtol=1e-12, atol=0)
    assert [p.kp_p, p.kd_p, p.kp_a, p.kd_a, p.yaw_gain, p.max_pos_err] == fx["gains"].tolist() == list(pilot_model.GAINS.values())
    assert p.gravity == float(fx["gravity"]) == cfg.gravity and list(p.x_des) == fx["x_des"].tolist() == list(pilot_model.X_DES)
    np.testing.assert_allclose(np.array(p.jinv)[0], [0.05365095, -0.0008059, -0.00084643, -0.00848246], rtol=0, atol=5e-9)   # as printed: 8 decimals
    J = pilot_model.jacobian(cfg)
    np.testing.assert_allclose(np.array(p.jinv) @ J, np.eye(4), atol=1e-13)
    assert 60.0 < np.linalg.cond(J) < 70.0     # the reference warns above 50 and reports 66.6 for the Crazyflie
    L = native.lib()
    assert L.qs_pilot_default_params(None, C.byref(p)) == -1 and L.qs_pilot_default_params(C.byref(cfg), None) == -1
    bad = qcfg.make_config(num_envs=2, num_agents=8)
    bad.thrust_max[:] = [0.0] * 4              # no thrust, no inverse
    assert L.qs_pilot_default_params(C.byref(bad), C.byref(p)) == -1 and b"singular" in L.qs_last_error()


def test_library_exports_every_symbol_of_the_control_header():
    native.build()
    lib = C.CDLL(native.LIB_PATH)
    text = open(os.path.join(REPO, "include", "quadswarm_control.h")).read()
    declared = sorted(set(re.findall(r"^int\s+(qs_\w+)\(", text, flags=re.M)))
    assert declared == ["qs_pilot_actions", "qs_pilot_default_params", "qs_pilot_set_params"]
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} declared in include/quadswarm_control.h but not exported"
    # (the prototype table, qs_pilot_params' field names, size and offsets: tests/test_abi_layout.py)
    # null handles are refused before anything touches a GPU
    L = native.lib()
    assert L.qs_pilot_actions(None, None, None, None, 0, None) == -1
    assert L.qs_pilot_set_params(None, C.byref(native.PilotParams())) == -1


def test_fixture_properties(fx):
    """what tests/test_pilot_gpu.py relies on: 512 uniform + 504 near-hover + 8 crafted rows; no random row near one of normalize()'s two
    branches and every guard row deep inside one; at least half of the rows with a motor that is not clipped; orthonormal rotations"""
    state, thrust, kind = fx["state"], fx["thrust"], fx["kind"]
    assert state.shape == (1024, qcfg.QS_STATE_STRIDE) and thrust.shape == (1024, 4) and fx["jinv"].shape == (4, 4)
    assert [(kind == k).sum() for k in (0, 1, 2)] == [512, 504, 8]
    acc, cx = pilot_model.guard_quantities(state, gravity=float(fx["gravity"]), x_des=fx["x_des"])
    near = np.minimum(acc, cx)
    assert (near[kind < 2] > 1e-3).all()
    crafted = near[kind == 2]
    assert ((crafted < 1e-7) | (crafted > 1e-3)).all()
    assert (acc[kind == 2] < 1e-7).sum() >= 2 and ((cx[kind == 2] < 1e-7) & (acc[kind == 2] > 1e-3)).sum() >= 2
    dist = np.linalg.norm(state[:, 32:35] - state[:, 0:3], axis=1)
    assert (dist[kind == 2] > 4.0).sum() >= 3 and (dist[kind == 0] > 4.0).any() and (dist[kind == 1] < 0.6).all()
    unclipped = ((thrust > 0) & (thrust < 1)).any(axis=1)
    print("rows with an unclipped motor: uniform %.3f, near-hover %.3f, all %.3f" % (unclipped[kind == 0].mean(), unclipped[kind == 1].mean(), unclipped.mean()))
    assert unclipped.mean() >= 0.5 and (thrust >= 0).all() and (thrust <= 1).all()
    R = state[:, 6:15].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.allclose(np.linalg.det(R), 1.0)
    assert np.abs(np.linalg.norm(state[kind == 0, 15:18], axis=1)).max() > 40.0          # the x4 angular velocities
    loop = fx["closed_loop"]
    assert loop.shape == (4,) and loop[3] >= 256 and loop[0] > loop[1] > loop[2] > 0     # worst goal distance at 600 / 800 / 1000 steps, seeds

#!/usr/bin/env python
"""Build-container only (needs the reference checkout at /root/reference).  Records what the reference's NonlinearPositionController
(gym_art/quadrotor_multi/quadrotor_control.py:251-330, numpy branch `step`) answers for 1024 drone states, and how close it flies the
reference's own QuadrotorEnvMulti to a goal, into tests/golden/pilot_mellinger.npz (data only):

    state[1024, 35]   QS_STATE_STRIDE rows (pos 0:3, vel 3:6, rot 6:15 row-major, omega 15:18, goal 32:35; the motor columns are zero)
    thrust[1024, 4]   controller.action after controller.step(dynamics, goal, dt): normalised motor thrusts in [0, 1]
    jinv[4, 4], gains[6] (kp_p, kd_p, kp_a, kd_a, yaw_gain, max_pos_err), gravity, x_des[3]
    kind[1024]        0 = uniform row, 1 = near-hover row, 2 = crafted row
    closed_loop[4]    worst distance to the goal after 600 / 800 / 1000 control steps over `seeds` noise-free single-drone episodes, seeds

The controller imports tensorflow in its constructor whatever branch it runs: an empty module of that name stands in (the numpy branch never
touches it).  The dynamics handed to `step` is a stand-in with the four state attributes and a `step` that does nothing - the controller's
answer is `controller.action`.

Usage: python tools/capture_pilot_fixture.py [--seeds 256]
"""
import argparse
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "ref_harness"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.modules.setdefault("tensorflow", types.ModuleType("tensorflow"))

import capture as cap                                                                   # noqa: E402  (stub path + /root/reference)
from gym_art.quadrotor_multi.quadrotor_control import NonlinearPositionController       # noqa: E402
from gym_art.quadrotor_multi.quadrotor_dynamics import GRAV                             # noqa: E402
import pilot_model                                                                      # noqa: E402

ROOM_LO, ROOM_HI = np.array([-5.0, -5.0, 0.0]), np.array([5.0, 5.0, 10.0])
GUARD_KEEP, GUARD_CRAFT = 1e-3, 1e-7


class FrozenDynamics:
    """what NonlinearPositionController.step reads of a QuadrotorDynamics; its step() does nothing"""

    def __init__(self, pos, vel, rot, omega):
        self.pos, self.vel, self.rot, self.omega = pos, vel, rot, omega

    def step(self, thrusts, dt):
        pass


def noise_free_env(seed):
    cfg = cap.default_cfg(num_agents=1, neighbor_visible_num=0, neighbor_obs_type="none", use_downwash=False, use_numba=False,
                          quads_mode="static_same_goal", sense_noise=None, thrust_noise_ratio=0.0, ep_time=15.0)
    np.random.seed(seed)
    env = cap.make_env(cfg)
    env.envs[0].np_random = cap.RecordingNpRandom(seed)   # the spawn draws follow the seed too
    return env


def rand_rot(rng, n):
    """uniform over SO(3): unit quaternions from a 4-d normal"""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return quat_rot(q)


def quat_rot(q):
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def rotvec_rot(v):
    a = np.linalg.norm(v, axis=1, keepdims=True)
    ax = v / np.maximum(a, 1e-12)
    return quat_rot(np.concatenate([np.cos(a / 2), np.sin(a / 2) * ax], axis=1))


def pack(pos, vel, rot, omega, goal):
    s = np.zeros((len(pos), 35))
    s[:, 0:3], s[:, 3:6], s[:, 6:15], s[:, 15:18], s[:, 32:35] = pos, vel, rot.reshape(-1, 9), omega, goal
    return s


def keep_clear_of_the_guards(make, count, rng):
    """`count` rows of make(rng, n) whose |acc_des| and |zb x x_des| are both above GUARD_KEEP"""
    rows = np.zeros((0, 35))
    while len(rows) < count:
        s = make(rng, 2 * count)
        a, c = pilot_model.guard_quantities(s, gravity=GRAV)
        rows = np.concatenate([rows, s[(a > GUARD_KEEP) & (c > GUARD_KEEP)]])
    return rows[:count]


def uniform_rows(rng, n):
    omega = rng.normal(0.0, 5.0, (n, 3))
    omega[::7] *= 4.0
    return pack(rng.uniform(ROOM_LO, ROOM_HI, (n, 3)), rng.normal(0.0, 2.0, (n, 3)), rand_rot(rng, n), omega, rng.uniform(ROOM_LO, ROOM_HI, (n, 3)))


def hover_rows(rng, n):
    pos = rng.uniform(ROOM_LO + 1.0, ROOM_HI - 1.0, (n, 3))
    return pack(pos, rng.normal(0.0, 0.3, (n, 3)), rotvec_rot(rng.normal(0.0, 0.3 / np.sqrt(3.0), (n, 3))), rng.normal(0.0, 1.0, (n, 3)),
                pos + rng.uniform(-0.3, 0.3, (n, 3)))


def crafted_rows(rng):
    """goals beyond max_pos_err; acc_des inside normalize()'s 1e-5 guard (the velocity whose damping cancels gravity and the position term);
    zb parallel to x_des (acc_des along +-x).  Positions / goals are short binary fractions, so that float32 holds them exactly."""
    kp, kd = pilot_model.GAINS["kp_p"], pilot_model.GAINS["kd_p"]
    eye, tilt = np.eye(3), rotvec_rot(np.array([[0.25, -0.125, 0.5]]))[0]
    z3 = np.zeros(3)
    rows = [
        (np.array([-4.0, -3.5, 1.0]), np.array([0.5, -0.25, 0.125]), tilt, np.array([0.5, -1.0, 0.25]), np.array([4.0, 3.0, 8.5])),     # 12.7 m
        (np.array([4.5, 4.5, 9.5]), z3, eye, z3, np.array([4.5, 4.5, 0.5])),                                                              # straight down, 9 m
        (np.array([0.0, 0.0, 2.0]), np.array([-1.0, 2.0, 0.5]), rand_rot(rng, 1)[0], np.array([3.0, -2.0, 1.0]), np.array([3.0, 3.0, 4.0])),   # 4.7 m
    ]
    for pos, tg, rot, om in ((np.array([1.5, -2.25, 3.0]), z3, eye, z3), (np.array([-2.0, 0.5, 1.25]), z3, tilt, np.array([1.0, -2.0, 0.5]))):
        vel = (kp * tg + np.array([0.0, 0.0, GRAV])) / kd                                                                                 # acc_des = 0
        rows.append((pos, vel, rot, om, pos + tg))
    for sign, rot, om in ((1.0, eye, z3), (-1.0, tilt, np.array([-0.5, 0.25, 2.0]))):
        tg = np.array([sign * 1.0, 0.0, 0.0])
        vel = np.array([0.0, 0.0, GRAV / kd])                                                                                              # acc_des = (+-4.5, 0, 0)
        rows.append((np.array([0.5, -1.0, 2.0]), vel, rot, om, np.array([0.5, -1.0, 2.0]) + tg))
    tg = np.array([-6.0, 0.0, 0.0])                                                                                                       # clamped to 4 m AND zb = -x
    rows.append((np.array([3.0, 1.0, 2.5]), np.array([0.0, 0.0, GRAV / kd]), tilt, z3, np.array([3.0, 1.0, 2.5]) + tg))
    return pack(*[np.array([r[k] for r in rows]) for k in range(5)])


def reference_thrusts(ctrl, state):
    out = np.empty((len(state), 4))
    for k, s in enumerate(state):
        ctrl.step(FrozenDynamics(s[0:3].copy(), s[3:6].copy(), s[6:15].reshape(3, 3).copy(), s[15:18].copy()), s[32:35].copy(), 0.005)
        out[k] = ctrl.action
    return out


def closed_loop(seeds, steps=(600, 800, 1000)):
    """the reference env flown by the reference controller (actions 2 * thrust - 1, what RawControl maps back, quadrotor_control.py:53-56)"""
    worst = np.zeros(len(steps))
    for seed in range(seeds):
        env = noise_free_env(seed)
        env.reset()
        single = env.envs[0]
        ctrl = NonlinearPositionController(single.dynamics, tf_control=False)
        for t in range(1, steps[-1] + 1):
            d = single.dynamics
            ctrl.step(FrozenDynamics(d.pos, d.vel, d.rot, d.omega), single.goal, 0.01)
            _, _, done, _ = env.step([2.0 * ctrl.action - 1.0])
            assert not any(done)
            if t in steps:
                k = steps.index(t)
                worst[k] = max(worst[k], float(np.linalg.norm(single.dynamics.pos - single.goal)))
        if seed % 16 == 15:
            print(f"closed loop: {seed + 1} seeds, worst distance at steps {steps}: {worst}", flush=True)
    return np.concatenate([worst, [float(seeds)]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=256)
    args = ap.parse_args()
    rng = np.random.RandomState(20111)
    env = noise_free_env(0)
    ctrl = NonlinearPositionController(env.envs[0].dynamics, tf_control=False)
    crafted = crafted_rows(rng)
    state = np.concatenate([keep_clear_of_the_guards(uniform_rows, 512, rng), keep_clear_of_the_guards(hover_rows, 504, rng), crafted])
    kind = np.concatenate([np.zeros(512, np.int8), np.ones(504, np.int8), np.full(len(crafted), 2, np.int8)])
    assert state.shape == (1024, 35)
    thrust = reference_thrusts(ctrl, state)
    a, c = pilot_model.guard_quantities(state, gravity=GRAV)
    near = np.minimum(a, c)
    assert (near[kind < 2] > GUARD_KEEP).all() and ((near[kind == 2] < GUARD_CRAFT) | (near[kind == 2] > GUARD_KEEP)).all()
    unclipped = ((thrust > 0) & (thrust < 1)).any(axis=1)
    print("rows with an unclipped motor: uniform %.2f, near-hover %.2f, all %.2f; crafted rows inside a guard: %d" % (
        unclipped[kind == 0].mean(), unclipped[kind == 1].mean(), unclipped.mean(), int((near[kind == 2] < GUARD_CRAFT).sum())))
    twin = pilot_model.thrusts_of_state(state, ctrl.Jinv, gravity=GRAV)
    print("numpy twin against the reference: max |diff| = %.3g; cond(J) = %.1f" % (np.abs(twin - thrust).max(), np.linalg.cond(np.linalg.inv(ctrl.Jinv))))
    g = pilot_model.GAINS
    assert (ctrl.kp_p, ctrl.kd_p, ctrl.kp_a, ctrl.kd_a) == (g["kp_p"], g["kd_p"], g["kp_a"], g["kd_a"])
    loop = closed_loop(args.seeds)
    path = os.path.join(cap.GOLDEN_DIR, "pilot_mellinger.npz")
    np.savez_compressed(path, state=state, thrust=thrust, jinv=np.array(ctrl.Jinv, dtype=np.float64), kind=kind, gravity=np.float64(GRAV),
                        gains=np.array([ctrl.kp_p, ctrl.kd_p, ctrl.kp_a, ctrl.kd_a, g["yaw_gain"], g["max_pos_err"]]),
                        x_des=np.array(ctrl.rot_des[:, 0], dtype=np.float64), closed_loop=loop)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB; closed loop {loop}")


if __name__ == "__main__":
    main()

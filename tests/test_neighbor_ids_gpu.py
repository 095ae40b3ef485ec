"""The neighbour identities on the GPU (include/quadswarm_neighbors.h, csrc/qs_neighbor_ids.hip): the kernel against the numpy statement of
its definition (tests/neighbor_ids_model.py) - exact, there is no tolerance in this file but the row-sum bound of the attention probe - on
drone counts that do and do not divide 64, partial last blocks, one environment per block, both precisions, both element orders of the
state blocks, self blocks of 18 / 19 / 24 columns; rows that are older than the state, canaries around the output, a captured launch,
the reference's own indices through the float64 tape kernels, the refusals; then qs_neighbor_scatter, the facade and the rollout segment.

Every handle of this file is listed by spec_jobs(), so that `__graft_entry__.build()` can compile their config-specialised objects ahead of time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ids_model as nim  # noqa: E402
import test_hip_parity as thp  # noqa: E402
from quad_swarm_rl_amd import config as qcfg  # noqa: E402
from tests import attention_weights_cases as awc  # noqa: E402
from tests import golden_util as gu  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 7
BASE = dict(neighbor_obs_type="pos_vel", use_downwash=True, use_numba=True, collision_falloff_radius=4.0, rew_coeff=thp.REW, ep_time=0.2)
# (N, K, E): 2 drones; 21 environments of 3 drones fill a block with one idle lane, the 22nd starts a partial block; 8 drones (8 per block) with
# E no multiple of 8; every drone sees all others; 12 drones (5 per block, 4 idle lanes); 33 and 64 drones: a block is one environment
SHAPES = [(2, 1, 3), (3, 1, 22), (8, 2, 5), (8, 6, 17), (8, 7, 4), (12, 6, 6), (33, 8, 2), (64, 6, 2), (64, 63, 1)]


def shape_kw(N, K, **over):
    return dict(BASE, num_agents=N, neighbor_visible_num=K, **over)


# name -> (make_config keywords, environments, QS_TEAM, expected state_lane_major or None, expected self_dim)
VARIANTS = {
    "obst_floor": (dict(thp.CASES["c3_n8_obst"], ep_time=0.2), 5, None, None, 19),
    "wall": (shape_kw(8, 2, obs_repr="xyz_vxyz_R_omega_wall"), 5, None, None, 24),
    "lane_major": (shape_kw(8, 6), 17, None, 1, 18),       # the 8-wave team kernels' element order (tests/test_replay_gpu.py: c2_team) ...
    "rows": (shape_kw(8, 6), 17, "0", 0, 18),              # ... and the single-wave kernels' (c2_rows)
}
GATED = (dict(thp.CASES["c2_n8_dw"], ep_time=0.5), 40)     # the handle of tests/test_pilot_gpu.py's gated refusal
BLIND = (dict(thp.CASES["x_n8_blind"]), 8)
ROLLOUT_KW = dict(num_agents=8, neighbor_visible_num=6, neighbor_obs_type="pos_vel", use_numba=True, collision_falloff_radius=4.0)
FACADE = dict(ep_time=0.2, rew_coeff=None, obs_repr="xyz_vxyz_R_omega", neighbor_obs_type="pos_vel", collision_hitbox_radius=2.0,
              collision_falloff_radius=4.0, use_obstacles=False, obst_density=0.2, obst_size=0.6, obst_spawn_area=(8.0, 8.0), use_downwash=True,
              use_numba=True, quads_mode="static_same_goal", room_dims=(10.0, 10.0, 10.0))


def spec_jobs():
    """(make_config keywords, precision, QS_TEAM) of the handles this file creates, for __graft_entry__._spec_jobs"""
    jobs = []
    for N, K, E in SHAPES:
        jobs += [(dict(shape_kw(N, K), num_envs=E, seed=SEED), p) for p in ("f32", "f64") if not (p == "f64" and K == 63)]   # (no such float64 handle)
    for kw, E, team, _, _ in VARIANTS.values():
        jobs += [(dict(kw, num_envs=E, seed=SEED), p) + ((int(team),) if team is not None else ()) for p in ("f32", "f64")]
    jobs.append((dict(BLIND[0], num_envs=BLIND[1], seed=SEED), "f32"))
    jobs.append((dict(ROLLOUT_KW, num_envs=4, seed=5), "f32"))
    for K in (6, -1, 0):
        kw = dict(FACADE, num_agents=8, neighbor_visible_num=K, neighbor_obs_type="pos_vel" if K else "none")
        jobs.append((dict({k: v for k, v in kw.items() if v is not None}, num_envs=1, seed=0), "f32"))   # (what env.QuadrotorEnvMulti adds are make_config defaults)
    return jobs


def make(kw, E, precision, team=None, monkeypatch=None):
    from quad_swarm_rl_amd import native
    if team is not None:
        monkeypatch.setenv("QS_TEAM", team)
    return native.Stepper(qcfg.make_config(num_envs=E, seed=SEED, precision=precision, **kw), device=0)


def host_state(st):
    """(pos [T, 3], vel [T, 3]) of the handle's stored state, in its precision"""
    return st.to_host("pos").T.copy(), st.to_host("vel").T.copy()


def model(st, rows=None):
    pos, vel = host_state(st)
    return nim.neighbor_ids(st.to_host("obs") if rows is None else rows, pos, vel, **nim.layout_of(st.cfg))


def check_rows(ids, N, what):
    """no -1, no drone twice in a row, never the drone itself"""
    ids = ids.reshape(-1, N, ids.shape[-1])
    assert (ids >= 0).all() and (ids < N).all(), f"{what}: a slot without a drone"
    assert (ids != np.arange(N)[None, :, None]).all(), f"{what}: a drone is its own neighbour"
    srt = np.sort(ids, axis=-1)
    assert (srt[..., 1:] != srt[..., :-1]).all(), f"{what}: a drone twice in a row"


def step_random(st, rng):
    st.from_host("actions", rng.uniform(-1, 1, size=(st.T, 4)))
    st.step()
    st.sync()


def moments(st, what):
    """after reset, after one step, on every one of 30 steps of random actions - the step on which the 0.2-s episodes end and the environments
    reset themselves among them, by name: kernel == model, exact, and the rows name K distinct other drones"""
    N, K = st.N, int(st.cfg.num_neighbors)
    rng = np.random.RandomState(3)

    def check(moment):
        got = st.neighbor_ids().cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (st.T, K)
        want = model(st)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{what} {moment}: {len(bad)} slots differ from the model, first (row, slot) {bad[0]}: kernel {got[tuple(bad[0])]}, model {want[tuple(bad[0])]}"
        check_rows(got, N, f"{what} {moment}")

    st.reset()
    st.sync()
    check("after reset")
    ends = []
    for t in range(30):
        step_random(st, rng)
        done = st.to_host("done")
        assert done.all() == done.any()
        if done.any():
            ends.append(t)
            check(f"step {t}: the episode end, rows of the auto-reset")
        else:
            check(f"step {t}")
    st.check_errors()
    assert ends == [st.cfg.ep_len], (ends, st.cfg.ep_len)     # tick > ep_len: the 21st step of a 0.2-s episode at 100 Hz


# (64 drones that all see each other exist in float32 only: qs_create refuses the float64 handle, whose rows would need 198 KiB of LDS -
# tests/test_hip_parity.py::test_largest_observation_rows - so there are no such rows to name the neighbours of)
@pytest.mark.parametrize("shape,precision", [(s, p) for s in SHAPES for p in ("f32", "f64") if not (p == "f64" and s[1] == 63)],
                         ids=lambda v: v if isinstance(v, str) else "n%d_k%d_e%d" % v)
def test_kernel_against_the_model(shape, precision):
    N, K, E = shape
    st = make(shape_kw(N, K), E, precision)
    assert st.bufs.envs_per_block == 64 // N and st.real_size == (8 if precision == "f64" else 4)
    moments(st, f"N={N} K={K} E={E} {precision}")
    st.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_against_the_model_variants(variant, precision, monkeypatch):
    kw, E, team, lane_major, self_dim = VARIANTS[variant]
    st = make(kw, E, precision, team, monkeypatch)
    assert lane_major is None or st.bufs.state_lane_major == lane_major, (variant, st.bufs.state_lane_major)
    assert nim.layout_of(st.cfg)["self_dim"] == self_dim and st.obs_dim == self_dim + 6 * st.cfg.num_neighbors + (9 if st.cfg.use_obstacles else 0)
    moments(st, f"{variant} {precision}")
    st.close()


@pytest.fixture(scope="module", params=["f32", "f64"])
def live(request):
    """8 drones, 6 slots, 17 environments (two full blocks and one with a single environment), a few steps into an episode"""
    st = make(shape_kw(8, 6), 17, request.param)
    st.reset()
    rng = np.random.RandomState(11)
    for _ in range(3):
        step_random(st, rng)
    yield st, rng
    st.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_crafted_rows_exercise_the_tie_rules_and_the_clamp(precision):
    """What a live state never holds: two drones at ONE position (told apart by velocity in the even environments; with one velocity in the odd
    ones, where the lowest free index wins and the next slot gets the other) and differences beyond the clip box.  The state is planted with
    set_state, the rows are crafted the way the environment emits them (rows_for of tests/test_neighbor_ids_cpu.py) and passed as obs_dev."""
    import torch
    import test_neighbor_ids_cpu as tnc
    st = make(shape_kw(8, 2), 5, precision)
    st.reset()
    st.sync()
    for e in range(st.E):
        s, tick = st.get_state(e)
        s[2, 0:3] = s[1, 0:3] = [1.0, 0.5, 2.0]
        s[1, 3:6] = [0.3, 0.0, 0.0]
        s[2, 3:6] = [-0.2, 0.1, 0.0] if e % 2 == 0 else [0.3, 0.0, 0.0]
        s[4, 0:3], s[6, 0:3] = [7.0, -1.0, 3.0], [-7.0, 2.0, 1.0]                  # 14 m apart in x: the slot holds the clamp's 10
        s[4, 3:6], s[6, 3:6] = [5.0, 0.0, 0.0], [-5.0, 0.5, 0.0]                   # 10 m/s apart: the slot holds 6
        st.set_state(e, s, tick)
    lay = nim.layout_of(st.cfg)
    pos, vel = host_state(st)
    order = [[2, 1], [2, 0], [1, 3], [1, 2], [6, 7], [4, 6], [4, 0], [6, 4]]
    rows = np.concatenate([tnc.rows_for(pos[e * 8:(e + 1) * 8], vel[e * 8:(e + 1) * 8], order, lay=lay, dtype=st.np_real) for e in range(st.E)])
    assert rows.shape == (st.T, st.obs_dim) and abs(rows[4, lay["self_dim"]]) == lay["clip_pos"][0] and abs(rows[4, lay["self_dim"] + 3]) == lay["clip_vel"][0]
    got = st.neighbor_ids(obs=torch.as_tensor(rows, device="cuda")).cpu().numpy()
    want = nim.neighbor_ids(rows, pos, vel, **lay)
    assert np.array_equal(got, want)
    got = got.reshape(st.E, 8, 2)
    for e in range(st.E):
        assert got[e, 0].tolist() == ([2, 1] if e % 2 == 0 else [1, 2]), e        # by velocity / the lowest free index, then the other
        assert got[e, 3].tolist() == [1, 2] and got[e, 4].tolist() == [6, 7] and got[e, 7].tolist() == [6, 4], e
        assert got[e, 1].tolist() == [2, 0] and got[e, 2].tolist() == [1, 3], e    # a coincident drone seen from its twin: a zero difference
    st.close()


def test_an_old_copy_of_the_rows_meets_the_new_state_as_the_model_says(live):
    st, rng = live
    old = st.tensor("obs").clone()
    step_random(st, rng)
    got = st.neighbor_ids(obs=old).cpu().numpy()
    want = model(st, rows=old.cpu().numpy())
    assert np.array_equal(got, want)
    print(f"{(got < 0).sum()} of {got.size} slots of the old rows find no drone in the new state")
    assert (got < 0).any()                                    # every drone moved: the old differences are gone (premise of the -1 rule)
    fresh = st.neighbor_ids().cpu().numpy()
    assert np.array_equal(fresh, model(st)) and (fresh >= 0).all()


def test_a_fresh_copy_gives_what_null_gives(live):
    import torch
    st, _ = live
    a, b = st.neighbor_ids(), st.neighbor_ids(obs=st.tensor("obs").clone())
    assert torch.equal(a, b) and bool((a >= 0).all())


def test_nothing_is_written_outside_the_rows(live):
    import torch
    st, _ = live
    K, pad = int(st.cfg.num_neighbors), 256
    buf = torch.full((st.T * K + 2 * pad,), -77, device="cuda", dtype=torch.int32)
    out = buf[pad:pad + st.T * K].view(st.T, K)
    assert st.neighbor_ids(out=out).data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool((buf[:pad] == -77).all()) and bool((buf[pad + st.T * K:] == -77).all())
    assert np.array_equal(out.cpu().numpy(), model(st))


def test_a_captured_launch_replays_on_later_states(live):
    import torch
    st, rng = live
    out = torch.full((st.T, int(st.cfg.num_neighbors)), -5, device="cuda", dtype=torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st.neighbor_ids(out=out)                              # library warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.fill_(-5)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st.neighbor_ids(out=out)
    torch.cuda.synchronize()
    assert bool((out == -5).all())                            # capturing ran nothing
    seen = []
    for _ in range(3):
        step_random(st, rng)
        g.replay()
        torch.cuda.synchronize()
        eager = st.neighbor_ids()
        assert torch.equal(out, eager) and np.array_equal(eager.cpu().numpy(), model(st))
        seen.append(out.cpu().numpy().copy())
    assert len(seen) == 3


@pytest.mark.parametrize("name", ["nbr_n8_k2_obst", "nbr_n12_k6_svs"])
def test_the_references_own_indices_through_the_tape_kernels(name, monkeypatch):
    """tools/capture_neighbor_ids.py recorded what the reference's step() and reset() ranked; the float64 tape kernels replay its noise (as
    tests/test_hip_vs_reference.py does, 3 environments on one tape): ids equal on every step, episode ends and the reset row included, no
    excused rows - the fixture's rankings are decided by at least 1e-6 and the kernels meet the reference to 1e-9"""
    from quad_swarm_rl_amd import native
    monkeypatch.setenv("QS_SPEC", "off")          # a handle with a noise tape only ever launches the library's tape kernels
    E = 3
    g, cfgd = gu.load(name)
    cfg = gu.config_from_golden(cfgd, num_envs=E, precision="f64")
    n, K = cfgd["num_agents"], cfg.num_neighbors
    st = native.Stepper(cfg, device=0)
    st.set_noise_tape(np.tile(g["tape"], (E, 1)))
    st.reset()
    st.sync()
    assert np.array_equal(st.neighbor_ids().cpu().numpy().reshape(E, n, K), np.tile(g["nbr_idx0"], (E, 1, 1)))
    assert len(g["force_steps"]) == 0
    ends = 0
    for t in range(g["actions"].shape[0]):
        st.from_host("actions", np.tile(g["actions"][t], (E, 1, 1)).reshape(-1, 4))
        st.step()
        st.sync()
        st.check_errors()
        np.testing.assert_array_equal(st.to_host("done").reshape(E, n), np.tile(g["done"][t], (E, 1)), err_msg=f"done step {t}")
        assert np.abs(st.to_host("obs").reshape(E, n, -1) - g["obs"][t]).max() <= 1e-9, f"step {t}: the replay left the reference"
        got = st.neighbor_ids().cpu().numpy().reshape(E, n, K)
        ends += int(g["done"][t].any())
        assert np.array_equal(got, np.tile(g["nbr_idx"][t], (E, 1, 1))), f"{name} step {t} (episode end: {bool(g['done'][t].any())})"
    assert ends >= 2
    st.close()


def test_refusals():
    import ctypes as C
    import torch
    from quad_swarm_rl_amd import abi, native
    blind = make(*BLIND, "f32")                               # rows without neighbour slots
    with pytest.raises(native.QsError, match="num_neighbors is 0"):
        blind.neighbor_ids()
    out = torch.zeros((blind.T, 1), device="cuda", dtype=torch.int32)
    assert native.lib().qs_neighbor_ids(blind._h, None, C.c_void_p(out.data_ptr()), None) == abi.QS_ERR_INVALID
    blind.close()
    st = make(*GATED, "f32")
    st.reset()
    L = native.lib()
    assert L.qs_neighbor_ids(st._h, None, None, None) == abi.QS_ERR_INVALID and b"NULL" in L.qs_last_error()
    assert L.qs_neighbor_ids(None, None, C.c_void_p(out.data_ptr()), None) == abi.QS_ERR_INVALID
    with pytest.raises(ValueError):
        st.neighbor_ids(obs=torch.zeros((st.T, st.obs_dim), device="cuda", dtype=torch.float64))     # not the handle's precision
    with pytest.raises(ValueError):
        st.neighbor_ids(out=torch.zeros((st.T, 5), device="cuda", dtype=torch.int32))
    # a resident gated launch holds the state (set up as tests/test_pilot_gpu.py does)
    assert st.team
    st.neighbor_ids()
    K = 4
    table = (torch.rand((K, st.T, 4), device="cuda") * 2 - 1).contiguous()
    st.gate_create(ring_len=8, wg_per_group=2)
    side, feed = torch.cuda.Stream(), torch.cuda.Stream()
    st.step_gated(K, stream=side)
    st.gate_produce(table.data_ptr(), K, K, closed_loop=False, stream=feed)
    st.gate_wait(stream=side)
    with pytest.raises(native.QsError, match="gated launch"):
        st.neighbor_ids()
    st.sync()
    torch.cuda.synchronize()
    ids = st.neighbor_ids().cpu().numpy()
    assert np.array_equal(ids, model(st)) and (ids >= 0).all()
    assert st.gate_status()["error"] == 0
    st.close()


# ---- scatter, facade, rollout ------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,K", [(3, 8, 3), (1, 2, 1), (5, 12, 6), (2, 64, 63), (300, 3, 2)])
def test_scatter_against_the_numpy_form(E, N, K):
    import torch
    from quad_swarm_rl_amd import attention, native
    rng = np.random.RandomState(E * 100 + N)
    ids = np.stack([rng.permutation(N)[:K] for _ in range(E * N)]).astype(np.int32)      # distinct per row; the own index among them now and then
    ids[rng.rand(E * N, K) < 0.1] = -1
    w = rng.rand(E * N, K).astype(np.float32)
    w[0, 0] = np.float32(-0.0)
    want = nim.scatter(ids, w, N)
    got = attention.attention_matrix(torch.as_tensor(w, device="cuda"), N, ids=torch.as_tensor(ids, device="cuda"))
    assert got.dtype == torch.float32 and tuple(got.shape) == (E, N, N)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))       # bit copies, +0 everywhere else
    assert np.array_equal(attention.attention_matrix(w, N, ids=ids).view(np.uint32), want.view(np.uint32))
    L = native.lib()
    o = torch.zeros((E, N, N), device="cuda")
    i_d, w_d = torch.as_tensor(ids, device="cuda"), torch.as_tensor(w, device="cuda")
    for bad in ((None, w_d.data_ptr(), E, N, K, o.data_ptr()), (i_d.data_ptr(), w_d.data_ptr(), E, 1, K, o.data_ptr()), (i_d.data_ptr(), w_d.data_ptr(), E, N, 0, o.data_ptr()),
                (i_d.data_ptr(), w_d.data_ptr(), E, N, N, o.data_ptr()), (i_d.data_ptr(), w_d.data_ptr(), 0, N, K, o.data_ptr()), (i_d.data_ptr(), w_d.data_ptr(), E, 65, K, o.data_ptr()),
                (i_d.data_ptr(), w_d.data_ptr(), E, N, K, None)):
        assert L.qs_neighbor_scatter(*bad, None) == -1
    torch.cuda.synchronize()
    assert bool((o == 0).all())


def test_attention_weights_of_a_live_handle_as_drone_matrices():
    """AttentionProbe weights of the attention encoder at K = 6 of 8 on the handle's rows, scattered by the handle's neighbour ids"""
    import torch
    from quad_swarm_rl_amd import attention, policy
    import test_attention_weights_gpu as tawg
    st = make(shape_kw(8, 6), 17, "f32")                      # (the policy path reads float32 rows)
    st.reset()
    rng = np.random.RandomState(5)
    for _ in range(4):
        step_random(st, rng)
    N, K = st.N, int(st.cfg.num_neighbors)
    ref = policy.make_reference_encoder(seed=3, nbr_encoder="attention", num_nbr=K, self_dim=18, obst_dim=0).cuda()
    w = attention.AttentionProbe(ref).weights(st.tensor("obs").clone())
    ids = st.neighbor_ids()
    M = attention.attention_matrix(w, N, ids=ids)
    torch.cuda.synchronize()
    Mh, idh, wh = M.cpu().numpy(), ids.cpu().numpy().reshape(st.E, N, K), w.cpu().numpy().reshape(st.E, N, K)
    assert (idh >= 0).all()
    points = np.zeros((st.E, N, N), dtype=bool)
    for s in range(K):
        np.put_along_axis(points, idh[:, :, s:s + 1], True, axis=2)
    assert points.sum() == st.E * N * K and (Mh[~points] == 0).all() and (np.diagonal(Mh, axis1=1, axis2=2) == 0).all()
    assert np.array_equal(np.take_along_axis(Mh, idh, axis=2).view(np.uint32), wh.view(np.uint32))
    bound = min(tawg.TOL, awc.ROW_SUM_TOL)                    # the probe's bounds against its module, the tighter of the two
    err = float(np.abs(Mh.astype(np.float64).sum(axis=2) - 1.0).max())
    print(f"rows of the {st.E} drone-by-drone matrices sum to 1 within {err:.2e} (bound {bound:g})")
    assert err <= bound
    st.close()


def test_facade_neighborhood_indices():
    from quad_swarm_rl_amd import env as qenv

    def facade(K):
        return qenv.QuadrotorEnvMulti(num_agents=8, neighbor_visible_num=K, **dict(FACADE, neighbor_obs_type="pos_vel" if K else "none"))

    e = facade(6)                                              # 1 <= K < N - 1: a list of N arrays of length K
    e.reset()
    for moment in range(3):
        idx = e.neighborhood_indices()
        assert isinstance(idx, list) and len(idx) == 8 and all(isinstance(a, np.ndarray) and a.shape == (6,) and a.dtype.kind == "i" for a in idx)
        st = e._vec.stepper
        assert np.array_equal(np.stack(idx), model(st))
        check_rows(np.stack(idx), 8, f"facade moment {moment}")
        e.step(np.random.RandomState(moment).uniform(-1, 1, size=(8, 4)))
    e.close()
    e = facade(-1)                                             # K == N - 1: an ndarray [N, N - 1], all others in index order
    e.reset()
    idx = e.neighborhood_indices()
    assert isinstance(idx, np.ndarray) and idx.shape == (8, 7) and np.array_equal(idx, [[j for j in range(8) if j != i] for i in range(8)])
    assert np.array_equal(idx, e._vec.neighbor_ids().cpu().numpy())      # what the kernel reads off the rows
    e.close()
    e = facade(0)
    e.reset()
    with pytest.raises(RuntimeError, match="Incorrect number of neigbors"):
        e.neighborhood_indices()
    e.close()


def test_rollout_segment_records_the_neighbour_ids():
    """GraphedRollout(record_neighbor_ids=True) at T = 4, E = 4 against its eager twin; off, the segment has no such output"""
    import torch
    from quad_swarm_rl_amd import policy, rollout
    from quad_swarm_rl_amd.env import QuadSwarmVecEnv
    E, T = 4, 4
    enc = policy.FusedQuadEncoder(policy.make_reference_encoder(seed=2, nbr_encoder="mean_embed").cuda())
    head = rollout.GaussianActionHead(sample=False, seed=4)
    runs = []
    for graph in (True, False):
        env = QuadSwarmVecEnv(E, seed=5, **ROLLOUT_KW)
        env.reset()
        seg = rollout.GraphedRollout(env, enc, head, steps=T, graph=graph, record_neighbor_ids=True)
        if not graph:
            seg.warmup()
        first = {k: v.clone() for k, v in seg.run().items()}
        second = {k: v.clone() for k, v in seg.run().items()}
        last_ids = env.neighbor_ids().clone()                  # of last_obs, which the next segment would read first
        torch.cuda.synchronize()
        runs.append((first, second, last_ids))
        env.close()
    for a, b in zip(runs[0][:2], runs[1][:2]):
        for k in ("obs", "actions", "rewards", "dones", "last_obs", "neighbor_ids"):
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(runs[0][2], runs[1][2])
    first, second, _ = runs[0]
    ids = torch.cat([first["neighbor_ids"], second["neighbor_ids"]]).cpu().numpy()
    assert ids.dtype == np.int32 and ids.shape == (2 * T, E * 8, 6)
    check_rows(ids, 8, "segment")
    env = QuadSwarmVecEnv(E, seed=5, **ROLLOUT_KW)
    env.reset()
    plain = rollout.GraphedRollout(env, enc, head, steps=T)
    assert plain.neighbor_ids is None and "neighbor_ids" not in plain.run()
    # the ids of a segment's first step are those of the rows it started from
    seg = rollout.GraphedRollout(env, enc, head, steps=T, graph=False, record_neighbor_ids=True)
    before = env.neighbor_ids().clone()
    out = seg.run()
    assert torch.equal(out["neighbor_ids"][0], before)
    env.close()

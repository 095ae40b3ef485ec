"""The neighbour identities without a GPU: the numpy statement of include/quadswarm_neighbors.h (tests/neighbor_ids_model.py, the yardstick of
the kernel) against the recorded float64 runs of the reference, crafted rows for each rule of the definition, attention.attention_matrix with
ids, and the two prototypes of the header against abi.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbor_ids_model as nim  # noqa: E402
from quad_swarm_rl_amd import abi, attention  # noqa: E402
from tests import golden_util as gu  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# recorded runs of the reference: 1090 + 30 + 60 steps; the slim ones (e_*) keep positions but no velocities
FIXTURES = ["c2_n8_random", "c2_n8_k2_numpy", "c4_n32_svs", "c4_svs_resets", "c2_n8_episode", "e_n64_k20", "e_n2_k1_swap", "e_n33_k8_numpy_wall", "c2_n8_kall"]
NEW_FIXTURES = ["nbr_n8_k2_obst", "nbr_n12_k6_svs"]      # tools/capture_neighbor_ids.py: with the reference's own indices


def model_on_fixture(name):
    """(ids0 [N, K], ids [T, N, K], g, layout): the model on the rows reset() returned and on the rows of every step, each with the state
    recorded behind it; the velocities only where the fixture has them (they break ties between drones at ONE position, nothing else)"""
    g, cfgd = gu.load(name)
    lay = nim.layout_of(gu.config_from_golden(cfgd, num_envs=1))
    N, K = lay["num_agents"], lay["num_neighbors"]
    T = g["obs"].shape[0]
    has_vel = "s_vel" in g.files
    ids0 = nim.neighbor_ids(g["obs0"], g["s0_pos"], g["s0_vel"] if has_vel else None, **lay)
    ids = nim.neighbor_ids(g["obs"].reshape(T * N, -1), g["s_pos"].reshape(T * N, 3), g["s_vel"].reshape(T * N, 3) if has_vel else None, **lay)
    return ids0, ids.reshape(T, N, K), g, lay


def reference_order(pos, vel, K):
    """neighborhood_indices (gym_art/quadrotor_multi/quadrotor_multi.py:247-274) written out: all others in index order when K == N - 1, else
    the first K of a stable argsort of  max(|dp|, 0.01) + (dp / that) . dv  over the others"""
    N = pos.shape[0]
    out = np.zeros((N, K), dtype=np.int64)
    for i in range(N):
        others = np.array([j for j in range(N) if j != i])
        if K == N - 1:
            out[i] = others
            continue
        rel_pos, rel_vel = pos[others] - pos[i], vel[others] - vel[i]
        rel_dist = np.maximum(np.linalg.norm(rel_pos, axis=1), 0.01)
        new_rel_dist = rel_dist + np.sum(rel_pos / rel_dist[:, None] * rel_vel, axis=1)
        out[i] = others[np.argsort(new_rel_dist, kind="stable")[:K]]
    return out


def check_rows(ids, N, what):
    """no -1, no drone twice in a row, never the drone itself"""
    ids = ids.reshape(-1, N, ids.shape[-1])
    assert (ids >= 0).all() and (ids < N).all(), f"{what}: a slot without a drone"
    assert (ids != np.arange(N)[None, :, None]).all(), f"{what}: a drone is its own neighbour"
    srt = np.sort(ids, axis=-1)
    assert (srt[..., 1:] != srt[..., :-1]).all(), f"{what}: a drone twice in a row"


@pytest.mark.parametrize("name", FIXTURES)
def test_model_on_the_recorded_runs(name):
    ids0, ids, g, lay = model_on_fixture(name)
    N, K = lay["num_agents"], lay["num_neighbors"]
    check_rows(ids0, N, f"{name} reset")
    check_rows(ids, N, name)
    done = g["done"].any(axis=1)
    index_order = np.array([[j for j in range(N) if j != i] for i in range(N)])
    ranked = 0
    for t in range(ids.shape[0]):
        if K == N - 1:
            assert np.array_equal(ids[t], index_order), f"{name} step {t}"      # the reset rows of an episode end included
        elif not done[t] and "s_vel" in g.files:
            assert np.array_equal(ids[t], reference_order(g["s_pos"][t], g["s_vel"][t], K)), f"{name} step {t}"
            ranked += 1
    if K == N - 1:
        assert np.array_equal(ids0, index_order)
    print(f"{name}: N={N} K={K}, {ids.shape[0]} steps ({int(done.sum())} episode ends), {ranked} of them against the reference's ranking")
    assert K == N - 1 or ranked > 0 or "s_vel" not in g.files


def test_the_ranking_is_checked_where_it_can_be():
    """which recorded runs kept their velocities: on the five of them with K < N - 1 the ranking is compared, c2_n8_kall (K == N - 1) is held to
    index order; the slim ones (e_n64_k20, e_n33_k8_numpy_wall, e_n2_k1_swap) hold no s_vel, so their ranking cannot be"""
    with_vel = [n for n in FIXTURES if "s_vel" in gu.load(n)[0].files]
    assert sorted(with_vel) == sorted(["c2_n8_random", "c2_n8_k2_numpy", "c4_n32_svs", "c4_svs_resets", "c2_n8_episode", "c2_n8_kall"])


@pytest.mark.parametrize("name", NEW_FIXTURES)
def test_model_meets_the_references_own_indices(name):
    """every step, the episode-end steps (whose rows the reset inside the step ranked, with the previous episode's velocities) and the reset row"""
    ids0, ids, g, lay = model_on_fixture(name)
    done = g["done"].any(axis=1)
    assert done.sum() >= 2 and g["nbr_idx"].shape == ids.shape and g["nbr_idx0"].shape == ids0.shape
    assert np.array_equal(ids0, g["nbr_idx0"])
    for t in range(ids.shape[0]):
        assert np.array_equal(ids[t], g["nbr_idx"][t]), f"{name} step {t} (episode end: {bool(done[t])})"
    check_rows(ids, lay["num_agents"], name)


# ---- crafted rows, one per rule ----------------------------------------------------------------------------
LAY = dict(num_agents=4, num_neighbors=2, self_dim=18, clip_pos=[10.0, 10.0, 10.0], clip_vel=[6.0, 6.0, 6.0])


def rows_for(pos, vel, order, lay=LAY, dtype=np.float64):
    """observation rows whose slots hold the drones `order` [N, K], emitted the way the environment does"""
    N, K, sd = lay["num_agents"], lay["num_neighbors"], lay["self_dim"]
    pos, vel = np.asarray(pos, dtype=dtype), np.asarray(vel, dtype=dtype)
    obs = np.full((N, sd + 6 * K), 0.25, dtype=dtype)
    cp, cv = np.asarray(lay["clip_pos"], dtype=dtype), np.asarray(lay["clip_vel"], dtype=dtype)
    for i in range(N):
        for s in range(K):
            j = order[i][s]
            obs[i, sd + 6 * s:sd + 6 * s + 3] = np.clip(pos[j] - pos[i], -cp, cp)
            obs[i, sd + 6 * s + 3:sd + 6 * s + 6] = np.clip(vel[j] - vel[i], -cv, cv)
    return obs


POS = [[0.0, 0.0, 2.0], [1.0, 0.5, 2.0], [1.0, 0.5, 2.0], [-2.0, 1.0, 3.0]]     # drones 1 and 2 at ONE position


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_drones_at_one_position_are_told_apart_by_velocity(dtype):
    vel = [[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [-0.2, 0.1, 0.0], [0.0, 0.0, 0.5]]
    order = [[2, 1], [2, 3], [1, 0], [2, 0]]
    got = nim.neighbor_ids(rows_for(POS, vel, order, dtype=dtype), np.asarray(POS, dtype=dtype), np.asarray(vel, dtype=dtype), **LAY)
    assert np.array_equal(got, order)


def test_equal_velocities_lowest_free_index_wins_and_the_next_slot_gets_the_other():
    vel = [[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, 0.0, 0.5]]     # 1 and 2: one position, one velocity
    got = nim.neighbor_ids(rows_for(POS, vel, [[2, 1], [3, 0], [3, 0], [2, 1]]), np.asarray(POS), np.asarray(vel), **LAY)
    assert np.array_equal(got, [[1, 2], [3, 0], [3, 0], [1, 2]])
    # the same without any velocity: nothing matches the velocity columns, the lowest free index among the position matches wins
    got = nim.neighbor_ids(rows_for(POS, vel, [[2, 1], [3, 0], [3, 0], [2, 1]]), np.asarray(POS), None, **LAY)
    assert np.array_equal(got, [[1, 2], [3, 0], [3, 0], [1, 2]])
    # a velocity that matches no candidate does not turn a position match away (the reset rows: ranked and emitted with stale velocities)
    stale = np.asarray(vel) + 0.125
    stale[0] = 0.0
    got = nim.neighbor_ids(rows_for(POS, stale, [[3, 1], [3, 0], [3, 0], [0, 1]]), np.asarray(POS), np.asarray(vel), **LAY)
    assert np.array_equal(got, [[3, 1], [3, 0], [3, 0], [0, 1]])


def test_a_stale_row_gives_minus_one():
    vel = np.zeros((4, 3))
    obs = rows_for(POS, vel, [[1, 3], [0, 3], [0, 3], [0, 1]])
    moved = np.asarray(POS).copy()
    moved[3] += [0.01, 0.0, 0.0]                      # drone 3 moved behind the rows' back (qs_set_state)
    got = nim.neighbor_ids(obs, moved, vel, **LAY)
    assert np.array_equal(got, [[1, -1], [0, -1], [0, -1], [-1, -1]])


def test_a_difference_beyond_the_clip_box_still_matches():
    pos = [[-4.9, 0.0, 1.0], [4.9, 0.1, 1.0], [4.5, -4.0, 9.0], [0.0, 0.0, 5.0]]
    vel = [[3.0, 0.0, 0.0], [-3.0, 0.0, 0.0], [-3.0, 0.5, 0.0], [0.0, 0.0, 0.0]]
    lay = dict(LAY, clip_pos=[5.0, 5.0, 5.0], clip_vel=[4.0, 4.0, 4.0])
    order = [[1, 2], [0, 3], [0, 3], [2, 1]]
    obs = rows_for(pos, vel, order, lay=lay)
    assert obs[0, 18] == 5.0 and obs[0, 18 + 3] == -4.0 and obs[1, 18] == -5.0     # the premise: clipped columns
    assert np.array_equal(nim.neighbor_ids(obs, np.asarray(pos), np.asarray(vel), **lay), order)


# ---- attention.attention_matrix --------------------------------------------------------------------------------
def test_attention_matrix_with_ids_equals_the_old_form_when_every_drone_sees_all_others():
    N, E = 5, 3
    w = np.random.RandomState(2).rand(E * N, N - 1).astype(np.float32)
    ids = np.tile(np.array([[j for j in range(N) if j != i] for i in range(N)], dtype=np.int32), (E, 1))
    old, new = attention.attention_matrix(w, N), attention.attention_matrix(w, N, ids=ids)
    assert new.dtype == old.dtype and np.array_equal(old.view(np.uint32), new.view(np.uint32))
    assert np.array_equal(new, nim.scatter(ids, w, N))


def test_attention_matrix_k2_of_4_drops_a_slot_without_a_drone():
    w = np.array([[0.7, 0.3], [0.6, 0.4], [0.5, 0.5], [0.9, 0.1]], dtype=np.float32)
    ids = np.array([[2, 1], [3, -1], [0, 3], [1, 2]], dtype=np.int32)
    want = np.zeros((1, 4, 4), dtype=np.float32)
    want[0, 0, 2], want[0, 0, 1], want[0, 1, 3], want[0, 2, 0], want[0, 2, 3], want[0, 3, 1], want[0, 3, 2] = 0.7, 0.3, 0.6, 0.5, 0.5, 0.9, 0.1
    got = attention.attention_matrix(w, 4, ids=ids)
    assert np.array_equal(got, want) and (np.diagonal(got, axis1=1, axis2=2) == 0).all()
    assert np.array_equal(nim.scatter(ids, w, 4), want)
    import torch
    host = attention.attention_matrix(torch.from_numpy(w), 4, ids=torch.from_numpy(ids))     # a host tensor takes the same loop
    assert isinstance(host, torch.Tensor) and np.array_equal(host.numpy(), want)


def test_attention_matrix_refusals():
    w = np.zeros((8, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="every drone sees all others"):
        attention.attention_matrix(w, 4)                                          # as before: K < N - 1 without ids
    with pytest.raises(ValueError):
        attention.attention_matrix(w, 4, ids=np.zeros((8, 3), dtype=np.int32))    # ids of another shape
    with pytest.raises(ValueError):
        attention.attention_matrix(np.zeros((8, 4), dtype=np.float32), 4, ids=np.zeros((8, 4), dtype=np.int32))   # K > N - 1
    with pytest.raises(ValueError):
        attention.attention_matrix(np.zeros((7, 2), dtype=np.float32), 4, ids=np.zeros((7, 2), dtype=np.int32))   # rows no multiple of N


# ---- the header ------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_states_the_prototypes_of_abi_py(tmp_path):
    """quadswarm_control.h alone brings the two functions in, for a C compiler; their names, arity and the kind of each argument (a pointer, or
    an int32_t by value) are those abi.py binds"""
    import re
    c = tmp_path / "nbr_abi.c"
    c.write_text('#include "quadswarm_control.h"\nint main(void) { return qs_neighbor_ids == 0 || qs_neighbor_scatter == 0; }\n')
    res = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-address", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(c)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    text = open(os.path.join(REPO, "include", "quadswarm_neighbors.h")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["quadswarm.h"]            # needs only quadswarm.h
    protos = re.findall(r"^int (qs_\w+)\(([^)]*)\);", text, flags=re.M)
    assert [p[0] for p in protos] == abi.names(abi.QUADSWARM_NEIGHBORS_H) == ["qs_neighbor_ids", "qs_neighbor_scatter"]
    for (name, args), (_, restype, argtypes) in zip(protos, abi.QUADSWARM_NEIGHBORS_H):
        kinds = [abi.vp if "*" in a else {"int32_t": abi.i32}[a.split()[0]] for a in args.split(",")]
        assert restype is abi.cint and kinds == list(argtypes), name

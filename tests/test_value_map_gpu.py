"""The value map on the GPU (include/quadswarm_valuemap.h, quad_swarm_rl_amd/value_map.py): the expansion bit for bit against the numpy model of
tests/value_map_model.py, the reduction against numpy on crafted buffers, the whole path against FusedQuadEncoder.forward_head on the same
rows in the same chunks and against the fixtures the reference's V_ValueMapWrapper answered (tests/golden/value_map_*.npz), inside a HIP
graph, and behind the wrapper over the batched env."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import value_map_model as vm  # noqa: E402

pytestmark = pytest.mark.gpu

VALUE_TOL = 1e-5      # tests/test_rollout_targets_gpu.py VALUE_TOL; tests/test_value_map_cpu.py shows the reference's own fp32 inside it
ARGMAX_GAP = 2e-5     # an agent whose two largest float64 values are closer than 2 * VALUE_TOL may legitimately answer either cell
# the chunking of the whole-path tests.  `attention` pairs rows ACROSS a batch (quad_multi_model.py:84,92), so the reference's batch of one per
# cell is chunk_rows = 1 for it and nothing else; the other encoders take ragged chunks (1323 = 2 * 500 + 323).
CHUNK = {"mean_embed": 500, "attention_obst": 1, "none_obst": 500, "mha_k6": 500}


def _bits(x):
    return x.view(np.int32) if isinstance(x, np.ndarray) else x.cpu().numpy().view(np.int32)


def _expand_in_chunks(obs, off_x, off_y, shifts, chunk):
    """qs_value_map_expand chunk by chunk into a scratch of `chunk` rows (+ 2 guard rows that must stay as they are) -> all rows [A * nx * ny, D]"""
    import torch
    from quad_swarm_rl_amd import abi, policy
    A, D = obs.shape
    nx, ny = len(off_x), len(off_y)
    total = A * nx * ny
    P = abi.ValueMapParams()
    P.A, P.obs_dim, P.nx, P.ny, P.n_shifts = A, D, nx, ny, len(shifts)
    P.off_x[:nx], P.off_y[:ny] = [float(v) for v in off_x], [float(v) for v in off_y]
    for s, (col, axis, sign) in enumerate(shifts):
        P.shift_col[s], P.shift_axis[s], P.shift_sign[s] = col, axis, sign
    scratch = torch.full((chunk + 2, D), 777.0, device="cuda")
    out = torch.empty((total, D), device="cuda")
    P.obs, P.rows, P.cap_rows = obs.data_ptr(), scratch.data_ptr(), chunk
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for row0 in range(0, total, chunk):
        n = min(chunk, total - row0)
        rc = policy.lib().qs_value_map_expand(C.byref(P), row0, n, stream)
        assert rc == 0, policy.lib().qs_enc_last_error()
        out[row0:row0 + n] = scratch[:n]
        assert bool((scratch[n:] == 777.0).all()), "rows behind the chunk were written"
        scratch.fill_(777.0)
    return out


def _obs(A, D, seed):
    """uniform rows with a -0.0, a +0.0 and a denormal among the copied columns (a bit copy keeps them; an add of 0.0 would not keep -0.0)"""
    obs = np.random.default_rng(seed).uniform(-1, 1, (A, D)).astype(np.float32)
    obs[0, D - 1], obs[A - 1, 2], obs[0, 5] = -0.0, 0.0, 1e-41
    return obs


NBR6 = types.SimpleNamespace(num_nbr=6, self_dim=18, nbr_dim=6)
EXPAND_CASES = {   # name: (D, A, nx, ny, chunk, shifts or None = default, source offset in floats)
    "d54_4byte_chunks_inside_a_grid": (54, 5, 21, 21, 1000, None, 0),
    "d40_16byte_one_chunk": (40, 3, 21, 21, 3 * 441, None, 0),
    "d40_source_off_by_4_bytes": (40, 3, 21, 21, 3 * 441, None, 1),
    "grid_1x1": (40, 70, 1, 1, 64, None, 0),
    "grid_64x3": (40, 3, 64, 3, 200, None, 0),
    "neighbors_follow_k6": (54, 3, 21, 21, 700, "follow", 0),
    "two_on_one_axis_and_a_negative_sign": (40, 3, 21, 21, 999, [(0, 0, 1), (3, 0, -1), (1, 1, 1), (39, 1, -1)], 0),
    "chunks_of_one_row": (40, 2, 3, 2, 1, None, 0),
}


@pytest.mark.parametrize("name", EXPAND_CASES)
def test_expansion_bit_for_bit(name):
    import torch
    from quad_swarm_rl_amd import value_map
    D, A, nx, ny, chunk, shifts, src_off = EXPAND_CASES[name]
    shifts = vm.DEFAULT_SHIFTS if shifts is None else value_map.shift_list(NBR6, neighbors_follow=True) if shifts == "follow" else shifts
    if name == "neighbors_follow_k6":
        assert shifts == vm.DEFAULT_SHIFTS + [(c, ax, -1) for k in range(6) for c, ax in ((18 + 6 * k, 0), (19 + 6 * k, 1))]
    obs = _obs(A, D, seed=A + D)
    off_x, off_y = vm.offset_table(nx, 0.2), vm.offset_table(ny, 0.2)
    flat = torch.zeros(A * D + 4, device="cuda")
    flat[src_off:src_off + A * D] = torch.from_numpy(obs).cuda().reshape(-1)
    dev = flat[src_off:src_off + A * D].view(A, D)
    assert dev.data_ptr() % 16 == 4 * src_off                       # (torch allocations are at least 256-byte aligned)
    got = _expand_in_chunks(dev, off_x, off_y, shifts, chunk)
    torch.cuda.synchronize()
    want = vm.expand(obs, off_x, off_y, shifts)
    assert np.array_equal(_bits(got), _bits(want)), name


def _crafted(n):
    """six [4, n] buffers: the maximum in the last element (agent 0) and in lane 63's last element (agent 1); an exact tie of the maximum and
    of the minimum; all values equal; a -0.0 / +0.0 pair on top; one NaN; two NaNs"""
    g = np.random.default_rng(n)
    base = lambda: g.standard_normal((4, n)).astype(np.float32)
    last63 = max(k for k in range(n) if k % 64 == 63) if n >= 64 else n - 1
    out = {}
    b = base(); b[0, n - 1] = 9.0; b[1, last63] = 9.0; b[2, 0] = 9.0; b[3, n // 2] = -9.0
    out["max_in_the_last_element"] = b
    b = base()
    for a, (p, q) in enumerate(((n // 3, n - 1), (0, n // 2), (n - 1 - n // 5, n - 1), (1 % n, 70 % n))):
        b[a, [p, q]] = 7.0
        b[a, [(p + 1) % n, (q + 1) % n] if n > 4 else []] = -7.0
    out["exact_tie"] = b
    out["all_equal"] = np.full((4, n), -3.25, dtype=np.float32)
    b = -np.abs(base()) - 1.0
    b[0, [n // 2, n - 1]] = (-0.0, 0.0); b[1, [n // 2, n - 1]] = (0.0, -0.0); b[2, [0, n - 1]] = (-0.0, 0.0); b[3] = -b[3]; b[3, [0, n // 2]] = (0.0, -0.0)
    out["signed_zeros"] = b
    b = base(); b[0, n - 1] = np.nan; b[1, 0] = np.nan; b[2, n // 2] = np.nan; b[3, last63] = np.nan
    out["one_nan"] = b
    b = base(); b[0, [n // 2, n - 1]] = np.nan; b[1, [0, n - 1]] = np.nan; b[2, [last63, n // 4]] = np.nan; b[3, :] = np.nan
    out["two_nans"] = b
    return out


@pytest.mark.parametrize("nx,ny", [(21, 21), (1, 1), (64, 64)])
def test_reduction_against_numpy(nx, ny):
    """441, 1 and 4096 values per agent: not a multiple of 64, less than a wave, the maximum"""
    import torch
    from quad_swarm_rl_amd import abi, policy
    n = nx * ny
    for name, buf in _crafted(n).items():
        values = torch.from_numpy(buf).cuda()
        runs = []
        for _ in range(2):
            vmax, vmin, arg = torch.full((4,), 5.0, device="cuda"), torch.full((4,), 5.0, device="cuda"), torch.full((4,), -1, device="cuda", dtype=torch.int32)
            P = abi.ValueMapParams()
            P.A, P.nx, P.ny, P.values, P.vmax, P.vmin, P.argmax = 4, nx, ny, values.data_ptr(), vmax.data_ptr(), vmin.data_ptr(), arg.data_ptr()
            assert policy.lib().qs_value_map_reduce(C.byref(P), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            torch.cuda.synchronize()
            runs.append((vmax.cpu().numpy(), vmin.cpu().numpy(), arg.cpu().numpy()))
        (vmax, vmin, arg), again = runs
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(runs[0][:2], again[:2])) and np.array_equal(arg, again[2]), name
        w_max, w_min, w_arg = vm.reduce(buf)
        np.testing.assert_array_equal(arg, w_arg, err_msg=name)              # first index on ties, the first NaN
        np.testing.assert_array_equal(vmax, w_max, err_msg=name)             # (NaN equals NaN and -0.0 equals +0.0 here, as in numpy's own answer)
        np.testing.assert_array_equal(vmin, w_min, err_msg=name)
        assert np.array_equal(_bits(vmax), _bits(buf[np.arange(4), arg])), name   # vmax carries the bits of the element argmax names
    # a subset of the outputs: the others are not touched
    P = abi.ValueMapParams()
    arg = torch.full((4,), -1, device="cuda", dtype=torch.int32)
    P.A, P.nx, P.ny, P.values, P.argmax = 4, nx, ny, values.data_ptr(), arg.data_ptr()
    assert policy.lib().qs_value_map_reduce(C.byref(P), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(arg.cpu().numpy(), vm.reduce(buf)[2])


def _fused_critic(case, precision):
    from quad_swarm_rl_amd import policy
    fx = vm.load(case)
    module, value = vm.reference_critic(case, fx["seed"])
    critic = policy.FusedQuadEncoder(module.cuda(), precision=precision)
    critic.set_head(value.weight, value.bias)
    return fx, critic


def _whole_path(case, precision):
    """(fixture, ValueMap outputs as numpy, forward_head on the expanded rows in the same chunks)"""
    import torch
    from quad_swarm_rl_amd import value_map
    fx, critic = _fused_critic(case, precision)
    chunk = CHUNK[case]
    m = value_map.ValueMap(critic, chunk_rows=chunk)
    obs = torch.from_numpy(fx["obs"]).cuda()
    out = {k: v.clone() for k, v in m(obs).items()}
    rows = m.expand(obs)
    head = torch.cat([critic.forward_head(rows[s:s + chunk].contiguous()) for s in range(0, rows.shape[0], chunk)]).reshape(3, 21, 21)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rows), _bits(vm.expand(fx["obs"], m.off_x, m.off_y, m.shifts)))
    return fx, {k: v.cpu().numpy() for k, v in out.items()}, head.cpu().numpy(), m


@pytest.fixture(scope="module")
def fp32_maps():
    return {case: _whole_path(case, "fp32") for case in vm.CASES}


@pytest.mark.parametrize("case", vm.CASES)
def test_whole_path_against_forward_head_and_the_reference(fp32_maps, case):
    fx, out, head, m = fp32_maps[case]
    assert out["values"].shape == (3, 21, 21) and np.array_equal(_bits(out["values"]), _bits(head)), "values differ from forward_head on the same rows, same chunks"
    err = float(np.abs(out["values"].astype(np.float64) - fx["values64"]).max())
    print(f"\n{case}: max |values - float64 reference module| = {err:.2e} (bound {VALUE_TOL})")
    assert err <= VALUE_TOL
    flat = out["values"].reshape(3, -1)
    w_max, w_min, w_arg = vm.reduce(flat)
    assert np.array_equal(out["argmax"], w_arg) and np.array_equal(_bits(out["vmax"]), _bits(w_max)) and np.array_equal(_bits(out["vmin"]), _bits(w_min))
    assert out["argmax"].dtype == np.int32 and out["argmax_xy"].shape == (3, 2)
    assert np.array_equal(out["argmax_xy"], np.stack([m.off_x[w_arg // 21], m.off_y[w_arg % 21]], axis=1))
    idx, idy = m.offsets()
    assert np.array_equal(idx, fx["idx"]) and np.array_equal(idy, fx["idy"])


def test_argmax_is_the_references(fp32_maps):
    """wherever the fixture's two largest values differ by more than 2e-5; at most 1 of the 12 agents may be left out by that rule"""
    excluded = 0
    for case, (fx, out, _, _) in fp32_maps.items():
        ref = fx["values64"].reshape(3, -1)
        top = np.sort(ref, axis=1)
        decided = (top[:, -1] - top[:, -2]) > ARGMAX_GAP
        excluded += int((~decided).sum())
        assert np.array_equal(out["argmax"][decided], ref.argmax(axis=1)[decided]), case
    print(f"\nagents excluded by the top-two rule: {excluded} of 12")
    assert excluded <= 1


def test_whole_path_bf16_is_forward_head():
    _, out, head, _ = _whole_path("mean_embed", "bf16")
    assert np.array_equal(_bits(out["values"]), _bits(head))


def test_constructor_refusals():
    from quad_swarm_rl_amd import policy, value_map
    _, critic = _fused_critic("none_obst", "fp32")
    for kw in (dict(nx=0), dict(ny=65), dict(nx=65), dict(chunk_rows=0), dict(shifts=[(40, 0, 1)])):
        with pytest.raises(ValueError):
            value_map.ValueMap(critic, **kw)
    module, _ = vm.reference_critic("none_obst", 1)
    bare = policy.FusedQuadEncoder(module.cuda(), precision="fp32")
    with pytest.raises(ValueError):
        value_map.ValueMap(bare)
    bare.set_head(*[p.detach() for p in __import__("torch").nn.Linear(512, 2).parameters()])
    with pytest.raises(ValueError):
        value_map.ValueMap(bare)


def test_hip_graph_replay_and_no_allocation():
    import torch
    from quad_swarm_rl_amd import value_map
    fx, critic = _fused_critic("attention_obst", "fp32")
    m = value_map.ValueMap(critic, chunk_rows=500)
    obs = torch.from_numpy(fx["obs"]).cuda()
    first = {k: v.clone() for k, v in m(obs).items()}                # allocates; sets the kernels' attributes
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    m(obs)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before, "the second call with the same number of agents allocated"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(obs)
    new = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, fx["obs"].shape).astype(np.float32)).cuda()
    obs.copy_(new)                                                   # in place: the graph reads the same address
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.clone() for k, v in out.items()}
    eager = {k: v.clone() for k, v in value_map.ValueMap(critic, chunk_rows=500)(new.clone()).items()}
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(replayed[k].view(torch.int32) if replayed[k].dtype == torch.float32 else replayed[k],
                           eager[k].view(torch.int32) if eager[k].dtype == torch.float32 else eager[k]), k
    assert not torch.equal(replayed["values"], first["values"])


def test_wrapper_single_env_surface():
    """the single-env protocol (numpy observations, SingleQuadSwarm keeps its batched env as ._b) over a scripted stand-in: the reference's
    return value - the [21, 21] map of agent 0 - as numpy"""
    import torch
    from quad_swarm_rl_amd import value_map
    fx, critic = _fused_critic("mean_embed", "fp32")
    rows = fx["obs"].astype(np.float64)

    class Scripted:
        _b, num_agents = None, 3

        def reset(self, **kw):
            return rows, {}

        def step(self, actions):
            return rows[::-1].copy(), [0.0] * 3, np.zeros(3, bool), np.zeros(3, bool), [{}] * 3

        def render(self, *a, **k):
            return None

    env = value_map.V_ValueMapWrapper(Scripted(), critic, chunk_rows=500)
    with pytest.raises(RuntimeError):
        env.get_v_value_map_2d()
    env.reset()
    first = env.get_v_value_map_2d()
    env.step(None)
    second = env.get_v_value_map_2d()
    direct = value_map.ValueMap(critic, chunk_rows=500)                # one agent per call, as the wrapper calls it: the same chunking
    want = [direct(torch.from_numpy(fx["obs"][[a]]).cuda())["values"][0].cpu().numpy() for a in (0, 2)]
    assert isinstance(first, np.ndarray) and first.shape == (21, 21) and first.dtype == np.float32 and env.num_agents == 3 and env.render() is None
    assert np.array_equal(_bits(first), _bits(want[0])) and np.array_equal(_bits(second), _bits(want[1]))
    assert float(np.abs(first - fx["values64"][0]).max()) <= VALUE_TOL


def test_wrapper_over_the_batched_env():
    """2 environments x 8 drones, the `attention` critic, 6 neighbours.  chunk_rows = 1: `attention` pairs rows across a batch, so the
    unshifted row inside a larger chunk is NOT the critic's value of that row on its own - with chunks of one row the centre cell is."""
    import torch
    from quad_swarm_rl_amd import policy, sf_env, value_map
    kw = dict(num_agents=8, neighbor_visible_num=6, neighbor_obs_type="pos_vel", use_numba=True, collision_falloff_radius=4.0, use_downwash=True, ep_time=0.3)
    scheme = dict(quad_rewards=dict(pos=1.0, effort=0.05, spin=0.1, vel=0.0, crash=1.0, orient=1.0, yaw=0.0, quadcol_bin=5.0, quadcol_bin_smooth_max=10.0,
                                    quadcol_bin_obst=0.0))
    module = policy.make_reference_encoder(seed=7, nbr_encoder="attention").cuda()
    torch.manual_seed(8)
    value = torch.nn.Linear(512, 1).cuda()
    critic = policy.FusedQuadEncoder(module, precision="fp32")
    critic.set_head(value.weight, value.bias)
    env = value_map.V_ValueMapWrapper(sf_env.BatchedQuadSwarm(2, reward_shaping_scheme=scheme, seed=3, **kw), critic, chunk_rows=1)
    try:
        assert env.num_agents == 16 and env.render() is None
        obs, _ = env.reset()
        assert env.curr_obs is obs
        obs, rew, term, trunc, infos = env.step(torch.zeros((16, 4), device="cuda"))
        assert env.curr_obs is obs and obs["obs"].is_cuda and obs["obs"].shape == (16, 54)
        out = env.get_v_value_map_2d()
        cur = obs["obs"]
        assert out["values"].shape == (16, 21, 21) and out["argmax_xy"].shape == (16, 2)
        direct = value_map.ValueMap(critic, chunk_rows=1)(cur)
        alone = torch.cat([critic.forward_head(cur[a:a + 1].contiguous()) for a in range(16)]).reshape(16)
        torch.cuda.synchronize()
        assert torch.equal(out["values"].view(torch.int32), direct["values"].view(torch.int32))
        # the centre cell adds 0.0 to columns 0 and 1: the row's bits stay unless a coordinate is exactly -0.0 (a drone exactly on its goal's
        # x or y, which a stepped state is not); torch.equal compares with ==, for which even that row gives the same value
        assert torch.equal(out["values"][:, 10, 10], alone)
    finally:
        env.close()

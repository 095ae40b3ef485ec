"""Critic value maps over a grid of position offsets, on the device (include/quadswarm_valuemap.h states the semantics; csrc/qs_value_map.inc).

The reference's `--visualize_v_value` (swarm_rl/env_wrappers/v_value_map.py:39-67, wired at quad_utils.py:96-108) takes ONE agent's observation
row, overwrites columns 0 and 1 - x / y relative to the goal - with `init + i * 0.2`, `init + j * 0.2` for i, j in -10..10 and calls the critic
once per cell: 441 forward passes of batch one per frame.  `ValueMap` does that for every agent of every running environment in a handful of
launches behind a step: the rows are expanded on the device, the fused critic (`FusedQuadEncoder` with a 1-row head) runs on them in chunks,
and one wave per agent reduces its grid to maximum, minimum and the place of the maximum.  It produces the numbers, not the picture.
"""
import ctypes as C

import numpy as np

from . import abi, native, policy

AXIS_X, AXIS_Y = 0, 1


def offset_table(n, step):
    """n offsets centred on 0: float32(k * step) with k * step evaluated in double - what the reference's `float32 tensor + python float`
    adds (v_value_map.py:50-51), so the expanded rows equal the reference's inputs bit for bit.  Even n: k runs from -n/2 to n/2 - 1."""
    return np.array([np.float32(k * step) for k in range(-(n // 2), n - n // 2)], dtype=np.float32)


def grid_offsets(nx=21, ny=21, step=0.2):
    """(idx, idy) of ValueMap.offsets(): per cell, in the order of the cells, the offsets in double (the tables are their float32 roundings)"""
    kx, ky = np.arange(-(nx // 2), nx - nx // 2), np.arange(-(ny // 2), ny - ny // 2)
    return np.repeat(kx * float(step), ny), np.tile(ky * float(step), nx)


def shift_list(critic_params=None, neighbors_follow=False):
    """[(column, axis, sign)]: the reference's two columns; neighbors_follow adds the relative x / y of every neighbour slot with the
    opposite sign (a neighbour that stays where it is moves by -offset relative to a drone displaced by +offset)."""
    shifts = [(0, AXIS_X, 1), (1, AXIS_Y, 1)]
    if neighbors_follow:
        P = critic_params
        for k in range(P.num_nbr):
            shifts += [(P.self_dim + P.nbr_dim * k, AXIS_X, -1), (P.self_dim + P.nbr_dim * k + 1, AXIS_Y, -1)]
    return shifts


class ValueMap:
    """ValueMap(critic)(obs[A, D]) -> dict of device tensors: values [A, nx, ny] (values[a, i, j] = critic's value of agent a's row with
    off_x[i] added to column 0 and off_y[j] to column 1: the reference's tmp_score[i][j], i moves x), vmax [A], vmin [A], argmax [A] (int32,
    flat index i * ny + j, first index on ties, the first NaN if there is one) and argmax_xy [A, 2] (the maximum's offsets in metres).

    critic: a policy.FusedQuadEncoder with a 1-row head (set_head).  Defaults are the reference's grid: 21 x 21, step 0.2, centred, columns
    0 and 1.  neighbors_follow=True also shifts the relative x / y of every neighbour slot by the opposite amount, so that the neighbours
    stay where they are in the world while the drone is displaced (the reference leaves them attached to the drone).  What can NOT be made
    consistent from an observation: the obstacle SDF columns are a function of the map around the true position and are left alone, and so
    are velocities, attitude and the floor distance.

    The rows go through the critic in chunks of `chunk_rows`.  Every encoder but `attention` evaluates a row on its own; the reference's
    `attention` neighbour encoder pairs rows ACROSS a batch (quad_multi_model.py:84,92 tile the whole batch), so with it the values are those
    of the module on each chunk as ONE batch, and only chunk_rows=1 reproduces the reference's batch of one per cell.

    The object owns the scratch rows, the outputs and the critic's attention scratch at the chunk size, allocated on the first call (and
    again only if the number of agents changes): later calls allocate nothing, launch on the current stream and record into a HIP graph.
    The returned tensors are reused by the next call."""

    def __init__(self, critic, nx=21, ny=21, step=0.2, neighbors_follow=False, chunk_rows=65536, shifts=None):
        if getattr(critic, "_head", None) is None or critic._head[0].shape[0] != 1:
            raise ValueError("ValueMap: the critic needs a head of one row (FusedQuadEncoder.set_head(weight [1, out_dim], bias [1]))")
        if not (1 <= nx <= abi.QS_VMAP_MAX_GRID and 1 <= ny <= abi.QS_VMAP_MAX_GRID):
            raise ValueError(f"ValueMap: nx and ny must be 1..{abi.QS_VMAP_MAX_GRID}")
        if chunk_rows < 1:
            raise ValueError("ValueMap: chunk_rows must be at least 1")
        self.critic, self.nx, self.ny, self.step, self.chunk_rows = critic, int(nx), int(ny), float(step), int(chunk_rows)
        self.off_x, self.off_y = offset_table(self.nx, self.step), offset_table(self.ny, self.step)
        self.shifts = list(shifts) if shifts is not None else shift_list(critic.params, neighbors_follow)
        D = critic.params.obs_dim
        if len(self.shifts) > abi.QS_VMAP_MAX_SHIFTS or any(not 0 <= c < D for c, _, _ in self.shifts):
            raise ValueError(f"ValueMap: at most {abi.QS_VMAP_MAX_SHIFTS} shift entries, columns below {D}")
        self._A = 0
        policy.lib()

    def offsets(self):
        """(idx, idy) as the reference records them (v_value_map.py:59-60): float64, length nx * ny, idx[i * ny + j] = i-th x offset"""
        return grid_offsets(self.nx, self.ny, self.step)

    def _params(self, A):
        P = abi.ValueMapParams()
        P.A, P.obs_dim, P.nx, P.ny = A, self.critic.params.obs_dim, self.nx, self.ny
        P.off_x[:self.nx], P.off_y[:self.ny] = self.off_x.tolist(), self.off_y.tolist()
        P.n_shifts = len(self.shifts)
        for s, (col, axis, sign) in enumerate(self.shifts):
            P.shift_col[s], P.shift_axis[s], P.shift_sign[s] = col, axis, sign
        return P

    def _allocate(self, A, device):
        torch = self.critic._torch
        cr, D, n = self.critic, self.critic.params.obs_dim, self.nx * self.ny
        cap = min(self.chunk_rows, A * n)
        self._rows = torch.empty((cap, D), device=device, dtype=torch.float32)
        self._out = dict(values=torch.empty((A, self.nx, self.ny), device=device), vmax=torch.empty(A, device=device), vmin=torch.empty(A, device=device),
                         argmax=torch.empty(A, device=device, dtype=torch.int32))
        self._xy = torch.empty((2, A), device=device)                       # argmax_xy is its transpose: each table's gather writes one dense row
        self._out["argmax_xy"] = self._xy.t()
        self._tab = (torch.from_numpy(self.off_x).to(device), torch.from_numpy(self.off_y).to(device))
        self._ij = (torch.empty(A, device=device, dtype=torch.int32), torch.empty(A, device=device, dtype=torch.int32))
        E = abi.EncParams.from_buffer_copy(cr.params)   # a copy: the critic's own struct stays as it is
        w, b = cr._head
        E.head_w, E.head_b, E.head_dim, E.head_out = w.data_ptr(), b.data_ptr(), 1, None
        if cr.attention:   # the handover buffers of the two attention launches (policy.FusedQuadEncoder._scratch), at the chunk size
            self._ebuf = torch.empty((cap * E.num_nbr, policy.HIDDEN * (2 if cr._split else 1)), device=device, dtype=torch.bfloat16)
            self._gbuf = torch.empty((cap, policy.HIDDEN), device=device, dtype=torch.float32)
            E.ebuf, E.gbuf = self._ebuf.data_ptr(), self._gbuf.data_ptr()
        P = self._params(A)
        P.rows, P.cap_rows = self._rows.data_ptr(), cap
        o = self._out
        P.values, P.vmax, P.vmin, P.argmax = o["values"].data_ptr(), o["vmax"].data_ptr(), o["vmin"].data_ptr(), o["argmax"].data_ptr()
        self._P, self._E, self._A, self._device = P, E, A, device

    def __call__(self, obs):
        torch = self.critic._torch
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous() and obs.dim() == 2 and obs.shape[1] == self.critic.params.obs_dim
        A = obs.shape[0]
        if A != self._A or obs.device != self._device:
            self._allocate(A, obs.device)
        self._P.obs = obs.data_ptr()
        (w, b), E = self.critic._head, self._E                            # what set_head / refresh may have replaced since the last call
        E.head_w, E.head_b, E.a3b = w.data_ptr(), b.data_ptr(), self.critic.params.a3b
        rc = policy.lib().qs_value_map(C.byref(self._P), C.byref(self._E), C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
        if rc != 0:
            raise native.QsError(f"qs_value_map failed ({rc}): {policy.lib().qs_enc_last_error().decode()}")
        o, (i, j) = self._out, self._ij
        torch.div(o["argmax"], self.ny, rounding_mode="floor", out=i)      # a torch gather on the tables, no kernel of ours
        torch.remainder(o["argmax"], self.ny, out=j)
        torch.index_select(self._tab[0], 0, i, out=self._xy[0])
        torch.index_select(self._tab[1], 0, j, out=self._xy[1])
        return o

    def expand(self, obs, row0=0, n_rows=None, out=None):
        """the hypothetical rows row0 .. row0 + n_rows of `obs` alone (qs_value_map_expand): [n_rows, D]; tests and tools/bench_value_map.py"""
        torch = self.critic._torch
        A, D = obs.shape
        n_rows = A * self.nx * self.ny - row0 if n_rows is None else n_rows
        out = torch.empty((n_rows, D), device=obs.device, dtype=torch.float32) if out is None else out
        P = self._params(A)
        P.obs, P.rows, P.cap_rows = obs.data_ptr(), out.data_ptr(), out.shape[0]
        rc = policy.lib().qs_value_map_expand(C.byref(P), row0, n_rows, C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
        if rc != 0:
            raise native.QsError(f"qs_value_map_expand failed ({rc}): {policy.lib().qs_enc_last_error().decode()}")
        return out

    def reduce(self, values):
        """(vmax, vmin, argmax) of a values tensor [A, nx, ny] the caller supplies (qs_value_map_reduce)"""
        torch = self.critic._torch
        assert values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and values.shape[1:] == (self.nx, self.ny)
        A = values.shape[0]
        vmax, vmin, argmax = torch.empty(A, device=values.device), torch.empty(A, device=values.device), torch.empty(A, device=values.device, dtype=torch.int32)
        P = self._params(A)
        P.values, P.vmax, P.vmin, P.argmax = values.data_ptr(), vmax.data_ptr(), vmin.data_ptr(), argmax.data_ptr()
        rc = policy.lib().qs_value_map_reduce(C.byref(P), C.c_void_p(torch.cuda.current_stream(values.device).cuda_stream))
        if rc != 0:
            raise native.QsError(f"qs_value_map_reduce failed ({rc}): {policy.lib().qs_enc_last_error().decode()}")
        return vmax, vmin, argmax


class V_ValueMapWrapper:
    """The reference wrapper's surface (swarm_rl/env_wrappers/v_value_map.py) over sf_env.SingleQuadSwarm / BatchedQuadSwarm: reset / step pass
    through and remember the current observation - for the batched env the device tensor itself, not a copy to the host - and
    get_v_value_map_2d() answers the value map of that observation: the [nx, ny] array of agent 0 (numpy, the reference's tmp_score) for the
    single env, the whole ValueMap dict (every agent of every environment, device tensors) for the batched one.

    It returns NUMBERS.  The reference returns a matplotlib image of them (gym_art/quadrotor_multi/tests/plot_v_value_2d.py) and glues it to
    the rendered frame; rendering is out of this package's scope, and render() is the wrapped env's."""

    def __init__(self, env, critic, **grid):
        self.env, self.model, self.curr_obs = env, critic, None
        self.value_map = ValueMap(critic, **grid)
        self._batched = not hasattr(env, "_b")   # SingleQuadSwarm wraps a BatchedQuadSwarm of one environment as ._b

    def __getattr__(self, name):
        if name == "env":   # (not yet set: copy / pickle probing an empty instance)
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def unwrapped(self):
        return self.env.unwrapped

    def reset(self, **kwargs):
        obs, info = self.env.reset(**kwargs)
        self.curr_obs = obs
        return obs, info

    def step(self, action):
        out = self.env.step(action)
        self.curr_obs = out[0]
        return out

    def render(self, *a, **k):
        return self.env.render(*a, **k)

    def get_v_value_map_2d(self, width=None, height=None):
        torch = self.model._torch
        if self.curr_obs is None:
            raise RuntimeError("get_v_value_map_2d: call reset() first")
        if self._batched:
            return self.value_map(self.curr_obs["obs"].float().contiguous())   # (both are no-ops on the float32 stepper's tensor)
        row = torch.as_tensor(np.asarray(self.curr_obs)[:1], dtype=torch.float32, device=self.model.device).contiguous()   # the reference maps agent 0
        return self.value_map(row)["values"][0].cpu().numpy()

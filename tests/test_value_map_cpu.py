"""The value map without a GPU: include/quadswarm_valuemap.h against its mirror in abi.py (checked the way tests/test_abi_layout.py checks the
other four headers), the numpy model of tests/value_map_model.py against the fixtures the reference's V_ValueMapWrapper answered
(tools/capture_value_map.py), the condition the GPU test's value bound rests on, and the refusals of qs_value_map before any launch."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_abi_layout as tal  # noqa: E402  (strip_comments, declared, RESTYPE: the same rules for this header)
import value_map_model as vm  # noqa: E402

from quad_swarm_rl_amd import abi, policy, value_map  # noqa: E402

HEADER = "quadswarm_valuemap.h"
CONSTANTS = ["QS_VMAP_MAX_GRID", "QS_VMAP_MAX_SHIFTS", "QS_VMAP_MAX_OBS_DIM"]
VALUE_TOL = 1e-5          # tests/test_rollout_targets_gpu.py VALUE_TOL: what forward_head is held to in reference precision
RESTATEMENT_TOL = 1e-6    # oracle/ref_harness/capture_encoders.py: restatement vs reference class


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None
    tmp = tmp_path_factory.mktemp("vmap_abi")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             '    printf("S %zu", sizeof(qs_value_map_params));']
    lines += [f'    printf(" %zu", offsetof(qs_value_map_params, {f[0]}));' for f in abi.ValueMapParams._fields_]
    lines += ['    printf("\\n");'] + [f'    printf("C {n} %lld\\n", (long long)({n}));' for n in CONSTANTS] + ["    return 0;", "}"]
    (tmp / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", tal.INCLUDE, str(tmp / "layout.c"), "-o", str(tmp / "layout")])
    out = subprocess.check_output([str(tmp / "layout")], text=True).splitlines()
    # ... and with the encoder's header in front of it (each includes the other)
    (tmp / "both.c").write_text('#include "quadswarm_encoder.h"\n#include "quadswarm_valuemap.h"\nint main(void) { return (int)sizeof(qs_value_map_params) == 0; }\n')
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", tal.INCLUDE, str(tmp / "both.c"), "-o", str(tmp / "both")])
    return {("S" if t[0] == "S" else t[1]): [int(x) for x in t[1 if t[0] == "S" else 2:]] for t in (ln.split() for ln in out)}


def test_struct_constants_prototypes_and_exports(compiled):
    mirror = abi.ValueMapParams
    names = [f[0] for f in mirror._fields_]
    text = tal.strip_comments(open(os.path.join(tal.INCLUDE, HEADER)).read())
    body = re.search(r"typedef struct qs_value_map_params \{(.*?)\} qs_value_map_params;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\w+\])*\s*[,;]", body) == names and len(set(names)) == len(names)
    assert compiled["S"] == [C.sizeof(mirror)] + [getattr(mirror, n).offset for n in names]
    assert {n: compiled[n] for n in CONSTANTS} == {n: [getattr(abi, n)] for n in CONSTANTS}
    assert sorted(re.findall(r"#define (QS_\w+)", text)) == sorted(CONSTANTS)
    table, decl = abi.QUADSWARM_VALUEMAP_H, tal.declared(HEADER)
    assert sorted(abi.names(table)) == sorted(decl) == sorted(["qs_value_map", "qs_value_map_expand", "qs_value_map_reduce", "qs_value_map_sizeof_params"])
    for name, restype, argtypes in table:
        ret, nargs = decl[name]
        assert len(argtypes) == nargs and restype is tal.RESTYPE[ret], name
    policy.build()
    lib = C.CDLL(policy.ENC_LIB_PATH)
    for name in abi.names(table):
        assert hasattr(lib, name), name
    lib.qs_value_map_sizeof_params.restype = C.c_size_t
    assert lib.qs_value_map_sizeof_params() == C.sizeof(mirror)
    assert policy.ValueMapParams is mirror and any(os.path.basename(s) == "qs_value_map.inc" for s in policy.ENC_SOURCES)
    assert any(os.path.basename(s) == HEADER for s in policy.ENC_SOURCES)


@pytest.mark.parametrize("case", vm.CASES)
def test_model_and_offsets_reproduce_the_reference(case):
    """the reference's idx / idy are offsets(); the model's rows for the default shift list, fed to policy.make_reference_* in torch fp32 one
    row at a time (the reference's batch of one), give the reference's values to 1e-6"""
    torch = pytest.importorskip("torch")
    fx = vm.load(case)
    idx, idy = value_map.grid_offsets()
    assert idx.dtype == np.float64 and np.array_equal(idx, fx["idx"]) and np.array_equal(idy, fx["idy"])
    assert np.array_equal(value_map.offset_table(21, 0.2), vm.offset_table(21, 0.2))
    assert np.array_equal(value_map.offset_table(21, 0.2), fx["idx"].reshape(21, 21)[:, 0].astype(np.float32))
    assert value_map.shift_list() == vm.DEFAULT_SHIFTS
    assert fx["obs"].shape == (3, vm.CASES[case][4]) and fx["values"].dtype == np.float32 and fx["values"].shape == (3, 21, 21)
    module, value = vm.reference_critic(case, fx["seed"])
    np.testing.assert_array_equal(vm.weight_sums(module, value), fx["weight_sums"])
    rows = torch.from_numpy(vm.expand(fx["obs"], vm.offset_table(21, 0.2), vm.offset_table(21, 0.2)))
    with torch.no_grad():
        got = torch.cat([value(module(r[None])) for r in rows]).reshape(3, 21, 21).numpy()
    err = float(np.abs(got - fx["values"]).max())
    print(f"\n{case}: max |restatement on the model's rows - reference wrapper| = {err:.2e}")
    assert err <= RESTATEMENT_TOL


def test_the_references_own_float32_lies_inside_the_value_bound():
    """what the GPU test's bound rests on: the reference's float32 values within VALUE_TOL of the same module in float64, in every fixture;
    and at most one of the 12 agents has its two largest values closer than 2e-5 (the GPU test's argmax rule skips those)"""
    close = 0
    for case in vm.CASES:
        fx = vm.load(case)
        err = float(np.abs(fx["values"].astype(np.float64) - fx["values64"]).max())
        top = np.sort(fx["values64"].reshape(3, -1), axis=1)
        close += int(((top[:, -1] - top[:, -2]) <= 2e-5).sum())
        print(f"\n{case}: max |reference fp32 - float64| = {err:.2e}")
        assert err <= VALUE_TOL
    assert close <= 1


def test_model_reduction_rules():
    v = np.array([[1.0, 3.0, 3.0, -2.0], [0.0, -0.0, -1.0, -1.0], [1.0, np.nan, 5.0, np.nan]], dtype=np.float32)
    vmax, vmin, arg = vm.reduce(v)
    assert arg.tolist() == [1, 0, 1] and vmax[0] == 3.0 and vmin[0] == -2.0 and vmin[1] == -1.0 and np.isnan(vmax[2]) and np.isnan(vmin[2])
    rows = vm.expand(np.arange(12, dtype=np.float32).reshape(2, 6), [-1.0, 1.0], [10.0, 20.0, 30.0], [(0, 0, 1), (4, 1, -1), (5, 1, 1)])
    assert rows.shape == (12, 6) and rows[1 * 6 + 1 * 3 + 2].tolist() == [6.0 + 1.0, 7.0, 8.0, 9.0, 10.0 - 30.0, 11.0 + 30.0]


def _params(**kw):
    """every pointer poisoned with a small non-NULL value: nothing may be dereferenced on the host, and every call below is refused first"""
    P = abi.ValueMapParams()
    P.A, P.obs_dim, P.nx, P.ny, P.cap_rows, P.n_shifts = 3, 40, 21, 21, 500, 2
    P.shift_col[0], P.shift_axis[0], P.shift_sign[0] = 0, 0, 1
    P.shift_col[1], P.shift_axis[1], P.shift_sign[1] = 1, 1, 1
    for name in ("obs", "rows", "values", "vmax", "vmin", "argmax"):
        setattr(P, name, 4096)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(P, k)[v[0]] = v[1]
        else:
            setattr(P, k, v)
    return P


def _critic(**kw):
    E = abi.EncParams()
    E.obs_dim, E.head_dim, E.head_w, E.head_b = 40, 1, 4096, 4096
    for k, v in kw.items():
        setattr(E, k, v)
    return E


def test_refusals_come_before_any_launch():
    """every -1 case of include/quadswarm_valuemap.h, with a NULL stream and poisoned device pointers (there is no GPU here: a launch, or a
    host dereference of 4096, would not return -1 with a message)"""
    policy.build()
    lib = C.CDLL(policy.ENC_LIB_PATH)
    abi.bind(lib, abi.QUADSWARM_VALUEMAP_H + [r for r in abi.QUADSWARM_ENCODER_H if r[0] == "qs_enc_last_error"])
    bad_map = [dict(obs=None), dict(rows=None), dict(values=None), dict(nx=0), dict(nx=65), dict(ny=0), dict(ny=65), dict(ny=-1), dict(A=0), dict(A=-2),
               dict(obs_dim=0), dict(obs_dim=4097), dict(cap_rows=0), dict(cap_rows=-5), dict(n_shifts=65), dict(n_shifts=-1),
               dict(shift_col=(1, 40)), dict(shift_col=(0, -1)), dict(shift_col=(1, 0)), dict(shift_axis=(0, 2)), dict(shift_sign=(1, 0)), dict(shift_sign=(1, 2))]
    for kw in bad_map:
        P, E = _params(**kw), _critic()
        assert lib.qs_value_map(C.byref(P), C.byref(E), None) == -1, kw
        assert lib.qs_enc_last_error().startswith(b"qs_value_map: "), kw
        if "values" not in kw:
            assert lib.qs_value_map_expand(C.byref(P), 0, 100, None) == -1 and lib.qs_enc_last_error().startswith(b"qs_value_map_expand: "), kw
    for kw in (dict(head_dim=0), dict(head_dim=2), dict(head_w=None), dict(head_b=None), dict(obs_dim=41)):
        P, E = _params(), _critic(**kw)
        assert lib.qs_value_map(C.byref(P), C.byref(E), None) == -1 and lib.qs_enc_last_error().startswith(b"qs_value_map: "), kw
    P = _params()
    assert lib.qs_value_map(None, C.byref(_critic()), None) == -1 and lib.qs_value_map(C.byref(P), None, None) == -1
    for row0, n in ((-1, 10), (0, 0), (0, 501), (3 * 441 - 5, 6), (3 * 441, 1)):     # outside the map, or more than cap_rows
        assert lib.qs_value_map_expand(C.byref(P), row0, n, None) == -1, (row0, n)
    assert lib.qs_value_map_expand(None, 0, 1, None) == -1
    for kw in (dict(values=None), dict(nx=0), dict(ny=65), dict(A=0)):
        assert lib.qs_value_map_reduce(C.byref(_params(**kw)), None) == -1 and lib.qs_enc_last_error().startswith(b"qs_value_map_reduce: "), kw
    assert lib.qs_value_map_reduce(None, None) == -1
    assert lib.qs_value_map_reduce(C.byref(_params(vmax=None, vmin=None, argmax=None)), None) == 0    # nothing asked for: no launch at all


def test_the_flag_alone_changes_nothing():
    """make_quadrotor_env wraps only with a value_critic= AND --visualize_v_value; the wrapper's surface without a GPU"""
    import inspect
    from quad_swarm_rl_amd import sf_env
    assert inspect.signature(sf_env.make_quadrotor_env).parameters["value_critic"].default is None
    for name in ("reset", "step", "render", "get_v_value_map_2d"):
        assert callable(getattr(value_map.V_ValueMapWrapper, name))

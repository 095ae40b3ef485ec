"""The dynamic-LDS layout of the step / reset workgroups (csrc/qs_lds_layout.h), without a GPU: the header is compiled alone with the host
compiler, and the layouts the library reports (qs_debug_lds_bytes, qs_tape_lds_bytes) and the header computes are the ones recorded from
the commit before the layout moved into a header of its own - totals for the cases of tests/test_hip_parity.py, two layouts field by field."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from quad_swarm_rl_amd import config as qcfg, native
from tests.test_hip_parity import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quad-swarm-rl_amd", "csrc")

# LdsLayout's fields in declaration order: the order of the words of qs_spec_lw in a generated spec header
FIELDS = """off_mask off_omap off_si off_sr off_envflag off_scratch off_pos off_vel off_zax off_om off_goal off_obst off_metric off_obs goal_rows
total off_t_rot off_t_goal off_t_prox off_t_col off_t_dw off_t_ohit off_t_ri off_t_near off_topk off_t_redo off_self off_rows rows_per_pass
scr_cap off_cur""".split()

# lds_layout's arguments from the command line, the fields by name
MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "qs_lds_layout.h"
int main(int argc, char **argv) {
    if (argc != 11) return 2;
    int a[10];
    for (int k = 0; k < 10; ++k) a[k] = atoi(argv[1 + k]);
    const int real_size = a[0], N = a[1], obs_dim = a[2], num_obst = a[3], K = a[4], team = a[5], full = a[6], tape = a[7], scenario = a[8],
        rows_per_pass = a[9];
    const LdsLayout L = lds_layout(real_size, 64, N, 64 / N, obs_dim, num_obst, K, team, full != 0, tape != 0, scenario, rows_per_pass);
    static_assert(sizeof(LdsLayout) == %d * sizeof(int), "a field was added or removed: qs_spec_lw is bit-cast to this struct");
#define F(name) printf(#name " %%d\n", L.name);
    %s
    return 0;
}
""" % (len(FIELDS), " ".join(f"F({name})" for name in FIELDS))

# (case, precision) -> qs_debug_lds_bytes at num_envs = 8 for (team, spec) = (0, 0), (0, 1), (4, either), (8, either), then qs_tape_lds_bytes
TOTALS = {
    ("c2_n8_dw", "f32"): (16288, 9376, 29888, 30912, 16320),
    ("c2_n8_dw", "f64"): (32480, 18656, 57344, 59392, 32512),
    ("c3_n8_obst", "f32"): (13408, 10592, 28800, 29824, 13440),
    ("c3_n8_obst", "f64"): (26720, 19296, 53376, 55424, 26752),
    ("c4_n32_svs", "f32"): (16176, 9264, 57344, 91136, 16192),
    ("c4_n32_svs", "f64"): (32320, 18496, 98000, 149200, 32336),
    ("e_n64_k20", "f32"): (54208, 54208, 66608, 84016, 54224),
    ("e_n64_k20", "f64"): (108320, 108320, 130800, 149232, 108336),
}
# (case, team) -> the words of qs_spec_lw in the header generated for the float32 configuration (num_envs = 8)
SPEC_LW = {
    ("c2_n8_dw", 8): (4512, 0, 0, 0, 0, 6560, 96, 864, 1632, 5024, 5792, 2400, 2464, 17088, 8, 30912, 7584, 9120, 9888, 6560, 7072, 11680,
                      12448, 11936, 17088, 17056, 17088, 21696, 64, 8, 0),
    ("c4_n32_svs", 0): (6960, 0, 0, 0, 0, 8688, 32, 800, 1568, 7472, 6960, 2336, 2352, 2352, 72, 9264, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2352, 6960,
                        16, 32, 0),
}
FAST_SCENARIOS = ("static_same_goal", "o_static_same_goal", "swarm_vs_swarm")   # every other one: the full scenario set (qs_env_plan.h)


@pytest.fixture(scope="module")
def layout_program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "a host C++ compiler (the code-object checker is built with one)"
    tmp = tmp_path_factory.mktemp("lds_layout")
    src, exe = tmp / "lds_layout.cpp", tmp / "lds_layout"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    # no HIP header, directly or through another include
    deps = subprocess.check_output([cxx, "-std=c++17", "-M", "-I", CSRC, str(src)], text=True)
    assert "hip" not in deps.lower(), deps
    return str(exe)


@pytest.fixture(scope="module")
def lib():
    native.build()
    lib = C.CDLL(native.LIB_PATH)
    lib.qs_debug_lds_bytes.argtypes = [C.POINTER(qcfg.QsConfig), C.c_int, C.c_int]
    lib.qs_tape_lds_bytes.argtypes = [C.POINTER(qcfg.QsConfig), C.c_int, C.c_int, C.c_int]
    lib.qs_obs_dim.argtypes = [C.POINTER(qcfg.QsConfig)]
    return lib


def _is_full(cfg):
    return int(cfg.scenario not in {qcfg.SCENARIOS[n] for n in FAST_SCENARIOS})


@pytest.mark.parametrize("case,precision", sorted(TOTALS))
def test_totals_are_the_recorded_ones(lib, monkeypatch, case, precision):
    monkeypatch.delenv("QS_OBS_RP", raising=False)
    cfg = qcfg.make_config(num_envs=8, precision=precision, **CASES[case])
    t00, t01, t4, t8, tape = TOTALS[(case, precision)]
    got = {(team, spec): lib.qs_debug_lds_bytes(C.byref(cfg), team, spec) for team in (0, 4, 8) for spec in (0, 1)}
    assert got == {(0, 0): t00, (0, 1): t01, (4, 0): t4, (4, 1): t4, (8, 0): t8, (8, 1): t8}
    assert lib.qs_tape_lds_bytes(C.byref(cfg), lib.qs_obs_dim(C.byref(cfg)), _is_full(cfg), 8 if precision == "f64" else 4) == tape


@pytest.mark.parametrize("case,team", sorted(SPEC_LW))
def test_layout_field_by_field(lib, layout_program, case, team):
    """the header alone, given the arguments handle_layout (quadswarm_hip.hip) passes for the specialised kernels: complete rows for a
    team, 16 rows per pass for a single wave whose other columns fit its registers"""
    cfg = qcfg.make_config(num_envs=8, precision="f32", **CASES[case])
    args = [4, cfg.num_agents, lib.qs_obs_dim(C.byref(cfg)), cfg.num_obstacles, cfg.num_neighbors, team, _is_full(cfg), 0, cfg.scenario,
            64 if team else 16]
    out = subprocess.check_output([layout_program] + [str(a) for a in args], text=True).split()
    assert out[0::2] == FIELDS
    assert dict(zip(FIELDS, map(int, out[1::2]))) == dict(zip(FIELDS, SPEC_LW[(case, team)]))
    assert int(out[1::2][FIELDS.index("total")]) == lib.qs_debug_lds_bytes(C.byref(cfg), team, 1)


@pytest.mark.parametrize("case,precision", sorted(TOTALS))
def test_tape_argument_is_the_tape_layout(lib, layout_program, case, precision):
    """`tape` (once an #ifdef of the noise-tape unit): the generic single-wave layout plus a cursor per environment"""
    cfg = qcfg.make_config(num_envs=8, precision=precision, **CASES[case])
    args = [8 if precision == "f64" else 4, cfg.num_agents, lib.qs_obs_dim(C.byref(cfg)), cfg.num_obstacles, cfg.num_neighbors, 0,
            _is_full(cfg), 1, cfg.scenario, 64]
    got = dict(zip(FIELDS, map(int, subprocess.check_output([layout_program] + [str(a) for a in args], text=True).split()[1::2])))
    assert got["off_cur"] > 0 and got["total"] == TOTALS[(case, precision)][4]
    args[7] = 0
    got = dict(zip(FIELDS, map(int, subprocess.check_output([layout_program] + [str(a) for a in args], text=True).split()[1::2])))
    assert got["off_cur"] == 0 and got["total"] == TOTALS[(case, precision)][0]

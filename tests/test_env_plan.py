"""The small rules the host side of the environment stepper decides by (csrc/qs_env_plan.h), without a GPU: the header is compiled alone with
the host compiler and its answers are compared with the rules restated here.  The same file pins the dynamic LDS bytes of every layout
the host asks for (qs_debug_lds_bytes): the values read back from the library before the layout calls went through one helper."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import pytest

from quad_swarm_rl_amd import config as qcfg, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quad-swarm-rl_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include "qs_env_plan.h"
int main() {
    for (int s = 0; s < QS_SCENARIO_COUNT; ++s) printf("full %d %d\n", s, scenario_is_full(s) ? 1 : 0);
    const int agents[4] = {1, 8, 9, 64};
    for (int n : agents) printf("waves %d %d\n", n, spec_team_waves(n));
    // the boundary blocks * waves == 8 * cus and one block past it, for both team widths
    printf("team_default %d %d %d %d\n", team_default(256, 256, 8) ? 1 : 0, team_default(257, 256, 8) ? 1 : 0,
           team_default(512, 256, 32) ? 1 : 0, team_default(513, 256, 32) ? 1 : 0);
    for (int r = 0; r < 3; ++r) printf("self %d %d\n", r, qs_self_dim(r));
    return 0;
}
"""


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "a host C++ compiler (the code-object checker is built with one)"
    tmp = tmp_path_factory.mktemp("env_plan")
    src, exe = tmp / "env_plan.cpp", tmp / "env_plan"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)], text=True).splitlines()


def _lines(program_output, key):
    return [line.split()[1:] for line in program_output if line.startswith(key + " ")]


def test_the_small_rules(program_output):
    count = int(re.search(r"QS_SCENARIO_COUNT = (\d+)", open(os.path.join(ROOT, "include", "quadswarm.h")).read()).group(1))
    assert count == len(qcfg.SCENARIOS) == len(_lines(program_output, "full"))
    fast = {qcfg.SCENARIOS[n] for n in ("static_same_goal", "o_static_same_goal", "swarm_vs_swarm")}
    assert {int(s): int(v) for s, v in _lines(program_output, "full")} == {s: int(s not in fast) for s in range(count)}
    assert _lines(program_output, "waves") == [["1", "8"], ["8", "8"], ["9", "4"], ["64", "4"]]
    # <= 8 waves per CU: 256 blocks of 8 waves on 256 CUs is the last batch that takes the team kernels, 512 blocks of 4 waves likewise
    assert _lines(program_output, "team_default") == [["1", "0", "1", "0"]]
    assert _lines(program_output, "self") == [["0", "18"], ["1", "19"], ["2", "24"]]
    assert [qcfg.OBS_REPR_DIM[k] for k in sorted(qcfg.OBS_REPR_DIM, key=lambda k: qcfg.OBS_REPR[k])] == [18, 19, 24]


# (precision, N, visible neighbours, obstacles) -> qs_debug_lds_bytes for (team, spec) = (0, 0), (0, 1), (4, 0), (4, 1), (8, 0), (8, 1)
LDS_BYTES = {
    ('f32', 1, 0, 0): (10496, 10496, 21504, 21504, 22528, 22528),
    ('f32', 1, 0, 1): (30464, 30464, 43776, 43776, 44800, 44800),
    ('f32', 8, 0, 0): (8352, 8352, 18624, 18624, 19648, 19648),
    ('f32', 8, 6, 0): (16288, 9376, 29888, 29888, 30912, 30912),
    ('f32', 8, 7, 0): (17824, 9760, 29376, 29376, 30400, 30400),
    ('f32', 8, 0, 1): (10336, 10336, 23424, 23424, 24448, 24448),
    ('f32', 8, 6, 1): (19296, 10656, 34688, 34688, 35712, 35712),
    ('f32', 8, 7, 1): (20832, 11040, 34176, 34176, 35200, 35200),
    ('f32', 16, 0, 0): (8272, 8272, 18528, 18528, 19552, 19552),
    ('f32', 16, 6, 0): (16208, 9296, 56416, 56416, 90208, 90208),
    ('f32', 16, 15, 0): (30032, 30032, 41568, 41568, 42592, 42592),
    ('f32', 16, 0, 1): (9648, 9136, 22208, 22208, 23232, 23232),
    ('f32', 16, 6, 1): (18864, 10224, 60096, 60096, 93888, 93888),
    ('f32', 16, 15, 1): (32688, 32688, 45248, 45248, 46272, 46272),
    ('f32', 32, 0, 0): (8240, 8240, 18496, 18496, 19520, 19520),
    ('f32', 32, 6, 0): (16176, 9264, 56384, 56384, 90176, 90176),
    ('f32', 32, 31, 0): (54576, 54576, 66112, 66112, 67136, 67136),
    ('f32', 32, 0, 1): (9440, 8672, 21744, 21744, 22768, 22768),
    ('f32', 32, 6, 1): (18656, 10016, 59632, 59632, 93424, 93424),
    ('f32', 32, 31, 1): (57056, 57056, 69360, 69360, 70384, 70384),
    ('f64', 1, 0, 0): (20224, 20224, 39680, 39680, 41728, 41728),
    ('f64', 1, 0, 1): (45824, 45824, 69888, 69888, 71936, 71936),
    ('f64', 8, 0, 0): (16096, 16096, 34816, 34816, 36864, 36864),
    ('f64', 8, 6, 0): (32480, 18656, 57344, 57344, 59392, 59392),
    ('f64', 8, 7, 0): (35552, 19424, 56320, 56320, 58368, 58368),
    ('f64', 8, 0, 1): (20064, 18784, 42624, 42624, 44672, 44672),
    ('f64', 8, 6, 1): (38496, 21216, 65152, 65152, 67200, 67200),
    ('f64', 8, 7, 1): (41568, 21984, 64128, 64128, 66176, 66176),
    ('f64', 16, 0, 0): (15984, 15984, 34688, 34688, 36736, 36736),
    ('f64', 16, 6, 0): (32368, 18544, 96128, 96128, 147328, 147328),
    ('f64', 16, 15, 0): (60016, 60016, 80768, 80768, 82816, 82816),
    ('f64', 16, 0, 1): (19248, 17200, 41024, 41024, 43072, 43072),
    ('f64', 16, 6, 1): (37680, 20400, 102464, 102464, 153664, 153664),
    ('f64', 16, 15, 1): (65328, 65328, 87104, 87104, 89152, 89152),
    ('f64', 32, 0, 0): (15936, 15936, 34640, 34640, 36688, 36688),
    ('f64', 32, 6, 0): (32320, 18496, 96080, 96080, 147280, 147280),
    ('f64', 32, 31, 0): (109120, 109120, 129872, 129872, 131920, 131920),
    ('f64', 32, 0, 1): (18848, 16544, 40368, 40368, 42416, 42416),
    ('f64', 32, 6, 1): (37280, 20000, 101808, 101808, 153008, 153008),
    ('f64', 32, 31, 1): (114080, 114080, 135600, 135600, 137648, 137648),
}
OBST = dict(use_obstacles=True, obst_density=0.2, obst_size=0.6, obst_spawn_area=(8.0, 8.0), quads_mode="o_static_same_goal")


def test_every_layout_asks_for_the_bytes_it_always_did(monkeypatch):
    monkeypatch.delenv("QS_OBS_RP", raising=False)
    native.build()
    lib = C.CDLL(native.LIB_PATH)
    lib.qs_debug_lds_bytes.argtypes = [C.POINTER(qcfg.QsConfig), C.c_int, C.c_int]
    seen = 0
    for precision, N, obst in itertools.product(("f32", "f64"), (1, 8, 16, 32), (False, True)):
        for K in sorted({0, 6, N - 1}):
            if K > N - 1:      # validate: "Incorrect number of neigbors"
                continue
            cfg = qcfg.make_config(num_envs=4, num_agents=N, neighbor_visible_num=K, neighbor_obs_type="pos_vel" if K else "none",
                                   precision=precision, **(OBST if obst else {}))
            # validate's other condition on this grid: the largest layout qs_create may pick fits the 160 KiB of a CU
            assert lib.qs_debug_lds_bytes(C.byref(cfg), 8 if N <= 8 else 4, 0) <= 160 * 1024
            got = tuple(lib.qs_debug_lds_bytes(C.byref(cfg), team, spec) for team in (0, 4, 8) for spec in (0, 1))
            assert got == LDS_BYTES[(precision, N, K, int(obst))], (precision, N, K, obst)
            seen += 1
    assert seen == len(LDS_BYTES) == 40

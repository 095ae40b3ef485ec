"""The code-object verifier of the library (include/quadswarm.h: qs_spec_verify), on the CPU: hipcc cross-compiles and
llvm-objdump disassembles without a GPU.

Round 5 ended with one float32 parity case of the single-wave kernels failing under a scheduler flag and nobody knowing why.  Round 6 found
it on the GPU from a memory-fault trace (the environment index of `p.counters[q * E + e]` held a float) and in the ISA: a VGPR spill in front of the
`s_or_b64 exec, exec, s[0:1]` of a join block - ROCm 7.2's register allocator, not the kernel source.  These tests pin the defence:
the scanner flags exactly that object, the repair (the exec restore moved in front of the spills) makes it clean by permuting a few dozen bytes,
qs_spec_build() never hands out an object that shows the pattern, and what the build step left in the cache (and the libraries themselves) is
verified.  The checker is one plain C++ unit (csrc/qs_codeobj_check.cpp) behind two doors - the library's C ABI and the program
qs_spec_check, which the Python build runs instead of loading a library - and both are held to the same answers here."""
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

from quad_swarm_rl_amd import config as qcfg, native
from tests import test_hip_parity as thp

TRACKERS = "-mllvm -amdgpu-use-amdgpu-trackers"


def n17_cfg():
    return qcfg.make_config(num_envs=7, precision="f32", **thp.CASES["e_n17_kall_obst"])


def test_the_scanner_flags_round5s_object(tmp_path, monkeypatch):
    """the single-wave float32 object of e_n17_kall_obst built with the RP-tracker flag: `scratch_store ...; s_or_b64 exec, exec, s[..]` at a join"""
    monkeypatch.setenv("QS_SPEC_CACHE", str(tmp_path))
    monkeypatch.setenv("QS_SPEC_SINGLE_FLAGS", TRACKERS)
    monkeypatch.setenv("QS_SPEC_VERIFY", "0")          # take the object as the compiler delivers it
    path = native.spec_build(n17_cfg(), 0)
    assert not os.path.exists(path.replace(".hsaco", ".ok"))
    rc, report = native.spec_verify(path)
    assert rc == 1, "the compiler no longer produces the pattern for this object: re-derive the test case (csrc/qs_spec_check verify over a cache)"
    assert "qs_spec_step <L" in report and "scratch_store_" in report and report.rstrip().endswith("]") and "s_or_b64 exec, exec, s[" in report


def test_the_repair_moves_the_restore_in_front_of_the_spills(tmp_path, monkeypatch):
    """qs_spec_repair on round 5's object: same bytes, the `s_or_b64 exec` first in its block prologue - and nothing else changed"""
    monkeypatch.setenv("QS_SPEC_CACHE", str(tmp_path))
    monkeypatch.setenv("QS_SPEC_SINGLE_FLAGS", TRACKERS)
    monkeypatch.setenv("QS_SPEC_VERIFY", "0")
    path = native.spec_build(n17_cfg(), 0)
    before = open(path, "rb").read()
    fixed, left = native.spec_repair(path)
    assert fixed >= 1 and left == "", (fixed, left)
    after = open(path, "rb").read()
    assert native.spec_verify(path)[0] == 0
    assert len(after) == len(before) and sorted(before) == sorted(after)                       # a permutation of the same bytes ...
    diff = [k for k in range(len(before)) if before[k] != after[k]]
    assert 0 < len(diff) and diff[-1] - diff[0] < 256 * fixed                                    # ... inside a few block prologues
    assert native.spec_repair(path) == (0, "")                                                   # nothing left to do


def test_a_flagged_object_is_repaired_or_rebuilt_before_it_is_used(tmp_path, monkeypatch):
    monkeypatch.setenv("QS_SPEC_CACHE", str(tmp_path))
    monkeypatch.setenv("QS_SPEC_SINGLE_FLAGS", TRACKERS)
    path = native.spec_build(n17_cfg(), 0)             # verification on (the default)
    stamp = open(path.replace(".hsaco", ".ok")).read()
    assert "exec restores moved" in stamp or "the configured ones were rejected" in stamp, stamp
    assert native.spec_verify(path)[0] == 0
    # ... and an unverified object that got into the cache (QS_SPEC_VERIFY=0 above, an older tree) is checked when it is asked for
    os.remove(path.replace(".hsaco", ".ok"))
    assert native.spec_build(n17_cfg(), 0) == path and os.path.exists(path.replace(".hsaco", ".ok"))


def test_the_libraries_and_the_prebuilt_cache_are_clean():
    from quad_swarm_rl_amd import policy
    for lib in (native.LIB_PATH, policy.ENC_LIB_PATH):
        if os.path.exists(lib):
            rc, report = native.spec_verify(lib)
            assert rc == 0, f"{lib}:\n{report}"
    cache = os.path.join(native.CSRC, "spec_cache")
    objs = sorted(glob.glob(os.path.join(cache, "*.hsaco")))
    if not objs:
        pytest.skip("no prebuilt cache (run __graft_entry__.build())")
    missing = [o for o in objs if not os.path.exists(o.replace(".hsaco", ".ok"))]
    assert not missing, f"{len(missing)} cached objects without a verification stamp, e.g. {missing[:3]}"
    for o in objs[::max(1, len(objs) // 10)]:          # a sample, re-checked here (the build verified each when it wrote the stamp)
        assert native.spec_verify(o)[0] == 0, o


def flagged_object(tmp_path, monkeypatch):
    """round 5's object as the compiler delivers it (the one test_the_scanner_flags_round5s_object pins)"""
    monkeypatch.setenv("QS_SPEC_CACHE", str(tmp_path))
    monkeypatch.setenv("QS_SPEC_SINGLE_FLAGS", TRACKERS)
    monkeypatch.setenv("QS_SPEC_VERIFY", "0")
    return native.spec_build(n17_cfg(), 0)


def tool(*args):
    return subprocess.run([native.build_check_tool(), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_the_tool_gives_the_c_abis_answers(tmp_path, monkeypatch):
    path = flagged_object(tmp_path, monkeypatch)
    rc, report = native.spec_verify(path)
    res = tool("verify", path)
    assert rc == 1 and res.returncode == 1 and res.stdout == report, (res.returncode, res.stdout, report)
    res = tool("repair", path)
    assert res.returncode == 0 and res.stdout == "", (res.returncode, res.stdout, res.stderr)
    assert tool("verify", path).returncode == 0 and native.spec_verify(path) == (0, "")
    assert tool("verify", str(tmp_path / "no_such.hsaco")).returncode == 2


def test_paths_with_a_space_and_a_quote(tmp_path, monkeypatch):
    """the checker starts llvm-objcopy / clang-offload-bundler / llvm-objdump from argument vectors, not through a shell"""
    path = flagged_object(tmp_path, monkeypatch)
    odd = tmp_path / "it's a cache"
    odd.mkdir()
    by_tool, by_abi = str(odd / "tool.hsaco"), str(odd / "abi.hsaco")
    shutil.copy(path, by_tool), shutil.copy(path, by_abi)
    rc, report = native.spec_verify(by_abi)
    res = tool("verify", by_tool)
    assert rc == 1 and res.returncode == 1 and res.stdout == report and "qs_spec_step <L" in report
    fixed, left = native.spec_repair(by_abi)
    assert fixed >= 1 and left == "" and tool("repair", by_tool).returncode == 0
    assert native.spec_verify(by_abi) == (0, "") and tool("verify", by_tool).returncode == 0
    assert open(by_tool, "rb").read() == open(by_abi, "rb").read() != open(path, "rb").read()
    res = tool("verify", str(odd))                                                               # a directory: every object in it
    assert res.returncode == 0 and "2 files, 0 with" in res.stderr, res.stderr


CHILD = """
import sys
from quad_swarm_rl_amd import native
native.finish_library(sys.argv[1])
maps = open("/proc/self/maps").read()
mapped = [n for n in ("libquadswarm_hip", "libamdhip64", "libhsa-runtime64") if n in maps]
sys.exit(f"mapped: {mapped}" if mapped else 0)
"""


def finish_in_a_fresh_process(lib, tmp_path, **env):
    copy = str(tmp_path / os.path.basename(lib))
    shutil.copy(lib, copy)
    res = subprocess.run([sys.executable, "-c", CHILD, copy], env=dict(os.environ, **env), cwd=os.path.dirname(native.HERE),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0 and os.path.exists(copy), res.stdout


def test_the_python_build_checks_a_library_without_loading_one(tmp_path):
    """native.finish_library runs the checker as a program: afterwards the process has mapped neither the stepper library nor a HIP runtime"""
    finish_in_a_fresh_process(native.LIB_PATH, tmp_path)


def test_the_encoder_library_is_checked_when_the_stepper_library_does_not_exist(tmp_path):
    """policy.build() in a tree without libquadswarm_hip.so"""
    enc = os.path.join(native.CSRC, "libquadswarm_encoder.so")
    finish_in_a_fresh_process(enc if os.path.exists(enc) else native.LIB_PATH, tmp_path, QS_LIB=str(tmp_path / "not_built" / "libquadswarm_hip.so"))


def test_the_staleness_check_covers_every_file_the_library_is_compiled_from():
    """native.build() rebuilds when a file of native.SOURCES is newer than the library: every translation unit and every file of this tree
    one of them includes, directly or not, has to be in it (qs_step_sem.h and qs_xchg_dev.h were not, for three rounds)."""
    listed = {os.path.realpath(f) for f in native.SOURCES}
    seen, todo = set(), [os.path.realpath(u) for u in native.UNITS]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        for inc in re.findall(r'#include "([^"]+)"', open(path).read()):
            if os.path.exists(os.path.join(os.path.dirname(path), inc)):
                todo.append(os.path.realpath(os.path.join(os.path.dirname(path), inc)))
    assert not seen - listed, f"not part of native.SOURCES: {sorted(seen - listed)}"
    names = {os.path.basename(f) for f in listed}
    assert {"qs_step_sem.h", "qs_xchg_dev.h", "qs_codeobj_check.cpp", "qs_codeobj_check.h", "quadswarm.h", "quadswarm_exchange.h"} <= names

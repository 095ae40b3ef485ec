"""The generic step / reset kernels are named ONCE on the host side (kStepKernels / kResetKernels, csrc/quadswarm_hip.hip): what raises
the dynamic-LDS limit and what launches both go through the tables.  A source-level check, like the spec cache key's in test_c_abi.py:
every kernel the two step bodies can emit for the generic flavour is in the table exactly once and nowhere else in the host unit."""
import itertools
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "quad-swarm-rl_amd", "csrc")


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _code(text):
    """without comments and string literals (file names, error texts)"""
    return re.sub(r'//[^\n]*|"(?:[^"\\\n]|\\.)*"', "", text)


def _generic_kernels():
    """the names behind `__global__` in the step bodies, outside their QS_SPEC branch (the tape flavour renames two of them with #define)"""
    names = []
    for body in ("qs_step_kernel.inc", "qs_step_team.inc"):
        found = re.findall(r"^(?:extern \"C\" )?__global__ void .*?\b(qs_\w+)\(QS_KARGS", _read(body), flags=re.M)
        assert found, body
        names += [n for n in found if not n.startswith("qs_spec_")]
    return names


def _host_unit():
    host = _read("quadswarm_hip.hip")
    parts = [n for n in re.findall(r'#include "(qs_\w+\.inc)"', host)]
    return host, _code(host) + "".join(_code(_read(n)) for n in parts)


def test_the_flavours_include_both_bodies_for_both_scenario_sets():
    generic = _read("qs_step_flavours.inc").split("#else   // ---- generic kernels")[1]
    assert re.findall(r'#define QS_SCEN_FULL (\d)[^\n]*\n#include "(\w+\.inc)"', generic) == [
        ("0", "qs_step_kernel_modes.inc"), ("1", "qs_step_kernel_modes.inc"), ("0", "qs_step_team_modes.inc"), ("1", "qs_step_team_modes.inc")]
    assert re.findall(r"#define (QS_MULTI|QS_GATED) (\d)|#include \"(\w+\.inc)\"", _read("qs_step_kernel_modes.inc")) == [
        ("QS_MULTI", "0", ""), ("", "", "qs_step_kernel.inc"), ("QS_MULTI", "1", ""), ("", "", "qs_step_kernel.inc")]
    assert re.findall(r"#define (QS_MULTI|QS_GATED) (\d)|#include \"(\w+\.inc)\"", _read("qs_step_team_modes.inc")) == [
        ("QS_MULTI", "0", ""), ("", "", "qs_step_team.inc"), ("QS_MULTI", "1", ""), ("", "", "qs_step_team.inc"),
        ("QS_GATED", "1", ""), ("", "", "qs_step_team.inc")]


def test_every_generic_kernel_is_in_the_table_once_and_nowhere_else():
    kernels = _generic_kernels()
    expected = [f"qs_{mode}_{body}{full}" for mode, body, full in itertools.product(("step", "rollout"), ("kernel", "team"), ("", "_full"))]
    assert sorted(kernels) == sorted(expected + ["qs_gated_team", "qs_gated_team_full"])
    host, code = _host_unit()
    table = re.search(r"kStepKernels(?:\[\w+\])+ = \{(.*?)\};", host, flags=re.S).group(1)
    assert sorted(re.findall(r"\bqs_\w+", _code(table))) == sorted(kernels)
    resets = re.search(r"kResetKernels(?:\[\w+\])+ = \{(.*?)\};", host, flags=re.S).group(1)
    assert sorted(re.findall(r"qs_reset_kernel<(\w+), (\w+)>", resets)) == sorted(itertools.product(("double", "float"), ("false", "true")))
    for name in kernels:
        assert len(re.findall(r"\b%s\b" % name, code)) == 1, name
    assert len(re.findall(r"\bqs_reset_kernel\b", code)) == 4


def test_every_compile_time_switch_named_outside_csrc_exists_in_it():
    """A `-DQS_...` in the documents, the build's job list, a test or a tool is a switch somebody is told to build with: it has to be an
    identifier of the kernel sources (a removed switch would be accepted silently by the compiler and change nothing)."""
    import glob
    files = [os.path.join(REPO, n) for n in ("INTEGRATION.md", "DESIGN.md", "README.md", "__graft_entry__.py")]
    files += sorted(glob.glob(os.path.join(REPO, "tests", "*.py"))) + sorted(f for f in glob.glob(os.path.join(REPO, "tools", "*")) if os.path.isfile(f))
    named = {}
    for path in files:
        for name in re.findall(r"-D(QS_[A-Z0-9_]+)", open(path, errors="replace").read()):
            named.setdefault(name, os.path.relpath(path, REPO))
    assert {"QS_SERIAL_PAIR_RESPONSES", "QS_SN_STASH", "QS_XCHG_INLINE", "QS_TIMING"} <= set(named), sorted(named)
    identifiers = set()
    for path in glob.glob(os.path.join(CSRC, "*")):
        if path.endswith((".h", ".inc", ".hip", ".cpp")):
            identifiers |= set(re.findall(r"\bQS_[A-Z0-9_]+\b", open(path).read()))
    missing = {name: where for name, where in named.items() if name not in identifiers}
    assert not missing, missing


def test_the_lds_limit_is_raised_on_the_tables():
    host, code = _host_unit()
    assert code.count("hipFuncAttributeMaxDynamicSharedMemorySize") == 1
    raiser = re.search(r"static bool raise_lds_limit\(const KernelEntry \*k, size_t count, int bytes\) \{(.*?)\n\}", host, flags=re.S).group(1)
    assert "for (; count--; ++k)" in raiser and "hipFuncSetAttribute(k->fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)" in raiser
    create = host[host.index("int qs_create("):host.index("int qs_is_specialized(")]
    assert "raise_lds_limit(&kStepKernels[0][0][0][0], sizeof kStepKernels / sizeof(KernelEntry), h->lds.total)" in create
    assert "raise_lds_limit(&kResetKernels[0][0], sizeof kResetKernels / sizeof(KernelEntry), h->lds.total)" in create

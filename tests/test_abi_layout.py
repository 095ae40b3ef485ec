"""quad_swarm_rl_amd/abi.py against the four public headers.  ONE C program that includes them (compiled as C, the way a foreign caller would)
prints sizeof / offsetof of every field of the eight mirrored structs and the value of every constant abi.py restates; the prototype tables are
compared with the declarations in the header text.  A wrong mirror does not raise at run time - it reads or writes the wrong device address -
so every struct, not only its size, is checked here.  No GPU, no library."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from quad_swarm_rl_amd import abi, config as qcfg, native, policy

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
STRUCTS = {"qs_config": abi.QsConfig, "qs_buffers": abi.QsBuffers, "qs_gate_info_t": abi.GateInfo, "qs_pilot_params": abi.PilotParams,
           "qs_wire_q8": abi.WireQ8, "qs_enc_layer": abi.EncLayer, "qs_enc_params": abi.EncParams, "qs_rollout_targets_params": abi.RolloutTargetsParams}
HEADERS = {"quadswarm.h": abi.QUADSWARM_H, "quadswarm_exchange.h": abi.QUADSWARM_EXCHANGE_H, "quadswarm_control.h": abi.QUADSWARM_CONTROL_H,
           "quadswarm_encoder.h": abi.QUADSWARM_ENCODER_H}
CONSTANTS = sorted(n for n, v in vars(abi).items() if n.startswith("QS_") and isinstance(v, int))
REQUIRED = """QS_MAX_AGENTS QS_MAX_OBSTACLES QS_MAX_DR_CHOICES QS_STATE_STRIDE QS_REW_COUNT QS_RI_COUNT QS_CNT_COUNT QS_EPS_COUNT QS_SUM_ACT QS_SUM_ACT2
    QS_SUM_COUNT QS_REPLAY_STATS QS_OK QS_ERR_NAN_REWARD QS_XCHG_EXPORT_BYTES QS_WIRE_F32 QS_WIRE_BF16 QS_WIRE_Q8 QS_ENC_NBR_MEAN_EMBED
    QS_ENC_NBR_ATTENTION QS_ENC_NBR_MLP QS_ENC_NBR_NONE QS_ENC_MODEL_MHA QS_ENC_MODEL_S2R""".split()
# the ctypes type a declared return type must be bound as (restype None would be `void`: no header function returns that)
RESTYPE = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "const char *": C.c_char_p, "void *": C.c_void_p}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """{"S <struct>": [sizeof, offsetof ...], "C <constant>": [value]} as the C compiler sees the headers"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler (the oracle is built with one)"
    tmp = tmp_path_factory.mktemp("abi")
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + [f'#include "{h}"' for h in HEADERS] + ["int main(void) {"]
    for cname, mirror in STRUCTS.items():
        lines.append(f'    printf("S {cname} %zu", sizeof({cname}));')
        lines += [f'    printf(" %zu", offsetof({cname}, {f[0]}));' for f in mirror._fields_]
        lines.append('    printf("\\n");')
    lines += [f'    printf("C {n} %lld\\n", (long long)({n}));' for n in CONSTANTS] + ["    return 0;", "}"]
    (tmp / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-I", INCLUDE, str(tmp / "layout.c"), "-o", str(tmp / "layout")])
    out = subprocess.check_output([str(tmp / "layout")], text=True)
    return {" ".join(ln.split()[:2]): [int(x) for x in ln.split()[2:]] for ln in out.splitlines()}


@pytest.mark.parametrize("cname", STRUCTS)
def test_struct_has_the_headers_layout(compiled, cname):
    mirror = STRUCTS[cname]
    names = [f[0] for f in mirror._fields_]
    assert len(set(names)) == len(names)
    # every field of the header's struct is mirrored: the body's declarators, comments stripped, in order
    text = strip_comments("".join(open(os.path.join(INCLUDE, h)).read() for h in HEADERS))
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), text, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\w+\])*\s*[,;]", body) == names
    assert compiled[f"S {cname}"] == [C.sizeof(mirror)] + [getattr(mirror, n).offset for n in names]


def test_constants_have_the_headers_values(compiled):
    assert not set(REQUIRED) - set(CONSTANTS)
    assert {n: compiled[f"C {n}"] for n in CONSTANTS} == {n: [getattr(abi, n)] for n in CONSTANTS}
    assert len(qcfg.REW_INFO_KEYS) == abi.QS_RI_COUNT and len(qcfg.COUNTER_KEYS) == abi.QS_CNT_COUNT
    assert len(qcfg.EPS_KEYS) == abi.QS_EPS_COUNT and len(qcfg.REW_COEFF_KEYS) == abi.QS_REW_COUNT
    assert qcfg.REW_INFO_KEYS_NO_OBST == [k for k in qcfg.REW_INFO_KEYS if "obstacle" not in k]
    assert (qcfg.QS_MAX_AGENTS, qcfg.QS_MAX_OBSTACLES, qcfg.QS_STATE_STRIDE) == (abi.QS_MAX_AGENTS, abi.QS_MAX_OBSTACLES, abi.QS_STATE_STRIDE)
    assert sorted(qcfg.OBS_REPR_ID_DIM) == sorted(qcfg.OBS_REPR.values())


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def declared(header):
    """{name: (return type, parameter count)} of every qs_* function `header` declares (a declaration may span lines)"""
    text = strip_comments(open(os.path.join(INCLUDE, header)).read())
    found = re.findall(r"^((?:const )?\w+(?: \*)?)\s*(qs_\w+)\(([^)]*)\)\s*;", text, flags=re.M)
    assert {f[1] for f in found} == set(re.findall(r"\b(qs_\w+)\([^)]*\)\s*;", text)), "a declaration the line-start pattern does not see"
    return {name: (ret, 0 if args.strip() == "void" else args.count(",") + 1) for ret, name, args in found}


@pytest.mark.parametrize("header", HEADERS)
def test_prototype_table_is_the_headers_declarations(header):
    table, decl = HEADERS[header], declared(header)
    assert len(decl) >= 3
    assert sorted(abi.names(table)) == sorted(decl) and len(set(abi.names(table))) == len(table)
    for name, restype, argtypes in table:
        ret, nargs = decl[name]
        assert len(argtypes) == nargs, f"{name}: {nargs} parameters declared"
        assert restype is RESTYPE[ret], f"{name} returns {ret}"


def test_symbol_lists_and_the_undeclared_table():
    assert native.EXPORTED_SYMBOLS == abi.names(abi.QUADSWARM_H) and native.EXCHANGE_SYMBOLS == abi.names(abi.QUADSWARM_EXCHANGE_H)
    assert native.CONTROL_SYMBOLS == abi.names(abi.QUADSWARM_CONTROL_H)
    everywhere = set().union(*(declared(h) for h in HEADERS))
    assert abi.names(abi.ENCODER_UNDECLARED) == ["qs_rollout_set_targets_chunks"] and not everywhere & set(abi.names(abi.ENCODER_UNDECLARED))
    assert (policy.EncLayer, policy.EncParams, policy.RolloutTargetsParams) == (abi.EncLayer, abi.EncParams, abi.RolloutTargetsParams)
    assert (qcfg.QsConfig, native.QsBuffers, native.GateInfo, native.PilotParams, native.WireQ8) == (
        abi.QsConfig, abi.QsBuffers, abi.GateInfo, abi.PilotParams, abi.WireQ8)

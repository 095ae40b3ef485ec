#!/usr/bin/env python
"""The ISA of the config-specialised kernels of a bench workload (no GPU needed).
  python tools/spec_asm.py c2 [team] [out.s]
      emit the assembly and a per-barrier-region instruction histogram of qs_spec_step / qs_spec_rollout
  python tools/spec_asm.py --sums [--precision f32|f64] [--team N] <workload | file.hsaco> ...
  python tools/spec_asm.py --sums --library [libquadswarm_hip.so]
      per kernel: instruction count, sha256 of the normalised disassembly, sha256 of its sorted instruction lines (equal = the same
      instructions in another order).  For comparing two source trees: run it in each and diff.  Normalised = the text in front of `//`
      (no addresses, no encodings), and the literals of an `s_getpc_b64` address computation masked (they change when a NEIGHBOURING
      kernel changes size).  A library's kernels: its .hip_fatbin section, first bundle (quadswarm_hip.hip's)."""
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LLVM_BIN = os.environ.get("QS_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def workload_object(wl, team=-1, precision="f32"):
    import bench
    from quad_swarm_rl_amd import config as qcfg, native
    kw = dict(bench.WORKLOADS[wl]["kw"])
    cfg = qcfg.make_config(num_envs=bench.WORKLOADS[wl]["num_envs"], seed=0, write_rew_info=False, precision=precision, **kw)
    return native.spec_build(cfg, team)


def disassemble(path, tmp):
    """{kernel name (demangled): [normalised instruction line, ...]} of an offload bundle (.hsaco of the spec cache) or a shared library"""
    bundle = path
    if open(path, "rb").read(4) == b"\x7fELF":   # a library: the bundles are its .hip_fatbin section
        bundle = os.path.join(tmp, "fatbin")
        subprocess.check_call([os.path.join(LLVM_BIN, "llvm-objcopy"), f"--dump-section=.hip_fatbin={bundle}", path, os.path.join(tmp, "rest")])
    elf = os.path.join(tmp, "object.elf")
    subprocess.check_call([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={bundle}",
                           f"--output={elf}"])
    text = subprocess.check_output([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", "--demangle", elf], text=True)
    out = {}
    for m in re.finditer(r"^[0-9a-f]+ <([^\n]+)>:\n(.*?)(?=^[0-9a-f]+ <[^\n]+>:\n|\Z)", text, flags=re.S | re.M):
        lines, pcrel = [], 0
        for line in m.group(2).split("\n"):
            if not line.startswith("\t"):
                continue
            ins = line.split("//")[0].strip()
            if ins.startswith("s_getpc_b64"):
                pcrel = 2   # s_add_u32 lo, lo, <literal>; s_addc_u32 hi, hi, <literal>
            elif pcrel and re.match(r"s_(add|addc|sub|subb)_u32 ", ins):
                ins, pcrel = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <pcrel>", ins), pcrel - 1
            lines.append(ins)
        out[m.group(1)] = lines
    return out


def sums(paths):
    sha = lambda lines: hashlib.sha256("\n".join(lines).encode()).hexdigest()
    for path in paths:
        with tempfile.TemporaryDirectory() as tmp:
            kernels = disassemble(path, tmp)
        print(f"# {os.path.basename(path)}: kernel, instructions, sha256(normalised disassembly), sha256(sorted instruction lines)")
        for name, lines in kernels.items():
            print(f"{name}  {len(lines)}  {sha(lines)}  {sha(sorted(lines))}")


def cls(k):
    if k in ("v_readlane_b32", "v_writelane_b32"): return "spill"
    if re.match(r"v_(sqrt|rcp|rsq|sin|cos|log|exp)_f(32|64)", k): return "trans"
    if re.match(r"v_(mul_lo_u32|mul_hi_u32|mad_u64_u32)", k): return "imul"
    if k.startswith("v_accvgpr"): return "agpr"
    if k.startswith("v_mov") or k.startswith("v_pk_mov"): return "vmov"
    if k.startswith("v_"): return "valu"
    if k.startswith("s_cbranch") or k.startswith("s_branch"): return "branch"
    if k.startswith("s_waitcnt"): return "wait"
    if k.startswith("s_nop"): return "nop"
    if k.startswith("s_load"): return "sload"
    if k.startswith("s_"): return "salu"
    if k.startswith("ds_"): return "lds"
    if k.split("_")[0] in ("global", "buffer", "flat", "scratch"): return "vmem"
    return "other"


def histogram(wl, team, out):
    from quad_swarm_rl_amd import native
    hdr = workload_object(wl, team).replace(".hsaco", ".h")
    subprocess.check_call(f"/opt/rocm/bin/hipcc --genco --offload-arch=gfx950 -O3 -std=c++17 -S -DQS_SPEC_FILE='\"{hdr}\"' "
                          f"{native.CSRC}/qs_spec_kernels.hip -o {out} 2>/dev/null", shell=True)
    lines = open(out).read().split("\n")
    for kern in ("qs_spec_step", "qs_spec_rollout"):
        start = next(i for i, l in enumerate(lines) if l.startswith(kern + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".section"))
        tot, cur, n = collections.Counter(), collections.Counter(), 0
        print(kern)
        for l in lines[start:end]:
            if not l.startswith("\t"):
                continue
            t = l.strip()
            if not t or t[0] in ".;":
                continue
            k = t.split()[0]
            if k == "s_barrier":
                print("  region", n, sum(cur.values()), dict(cur)); n += 1; cur = collections.Counter(); continue
            cur[cls(k)] += 1; tot[cls(k)] += 1
        print("  region", n, sum(cur.values()), dict(cur))
        print("  total", sum(tot.values()), dict(tot))
    print(out)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--sums" in args:
        args.remove("--sums")
        opt = {"--precision": "f32", "--team": "-1"}
        for key in opt:
            if key in args:
                opt[key] = args.pop(args.index(key) + 1)
                args.remove(key)
        if "--library" in args:
            args.remove("--library")
            if not args:
                from quad_swarm_rl_amd import native
                args = [native.LIB_PATH]
        sums([a if os.path.isfile(a) else workload_object(a, int(opt["--team"]), opt["--precision"]) for a in args])
    else:
        wl = args[0] if args else "c2"
        histogram(wl, int(args[1]) if len(args) > 1 else -1, args[2] if len(args) > 2 else f"/tmp/spec_{wl}.s")

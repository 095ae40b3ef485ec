"""The tail of the one-step team kernel, read off the ISA of the bench objects (hipcc cross-compiles for gfx950, llvm-objdump disassembles:
no GPU needed).

The fused observation exchange is a kernel of its own (`qs_spec_step_x`, qs_step_team_modes.inc).  While its epilogue was inlined into
`qs_spec_step` behind a run-time test, the waitcnt pass merged the rarely taken branch's pending memory operations into the join: wave 0 sat in
`s_waitcnt vmcnt(0)` - stores count in vmcnt on gfx950 - until every observation and output store had been acknowledged, and only then issued
its state stores, on every step of a handle that exchanges nothing.  What is pinned here for the C2 and C3 objects:
  * `qs_spec_step` has exactly the six workgroup barriers of the step (the epilogue brought three more);
  * between its last barrier and the `s_endpgm` behind it in address order - the fall-through path of wave 0's outputs and state stores; the
    cold blocks (auto-reset, responses) lie behind that `s_endpgm` or in front of the barrier - no `s_waitcnt` names vmcnt;
  * `qs_spec_step_x` exists and has more barriers;
  * on the same path the 16 per-environment rows are stored through their own buffer resource behind the state stores, and nothing behind
    the observation copy-out computes a 64-bit address (the typed pointers cost a v_ashrrev / v_lshl_add_u64 chain per row there).
"""
import os
import re
import subprocess

import pytest

LLVM_BIN = os.environ.get("QS_LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def _kernels(workload, tmp_path):
    """{kernel name: [instruction text, ...]} of the workload's config-specialised bench object, in address order"""
    import bench
    from quad_swarm_rl_amd import config as qcfg, native
    wl = bench.WORKLOADS[workload]
    cfg = qcfg.make_config(num_envs=wl["num_envs"], seed=0, write_rew_info=False, **wl["kw"])
    path = native.spec_build(cfg, -1)
    elf = str(tmp_path / "object.elf")
    subprocess.check_call([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={path}", f"--output={elf}"])
    text = subprocess.check_output([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", elf], text=True)
    out = {}
    for m in re.finditer(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <\w+>:|\Z)", text, flags=re.S | re.M):
        out[m.group(1)] = [line.split("//")[0].strip() for line in m.group(2).split("\n") if line.startswith("\t")]
    return out


@pytest.mark.parametrize("workload", ["c2", "c3"])
def test_the_step_kernel_has_no_exchange_code_and_no_memory_wait_behind_its_last_barrier(workload, tmp_path):
    k = _kernels(workload, tmp_path)
    assert "qs_spec_step" in k and "qs_spec_step_x" in k, sorted(k)
    step, step_x = k["qs_spec_step"], k["qs_spec_step_x"]
    barriers = [n for n, ins in enumerate(step) if ins.startswith("s_barrier")]
    barriers_x = sum(ins.startswith("s_barrier") for ins in step_x)
    print(f"{workload}: qs_spec_step {len(step)} instructions, {len(barriers)} barriers; qs_spec_step_x {len(step_x)} instructions, {barriers_x} barriers")
    assert len(barriers) == 6, len(barriers)
    end = next(n for n in range(barriers[-1], len(step)) if step[n].startswith("s_endpgm"))
    tail = step[barriers[-1] + 1:end]
    waits = [ins for ins in tail if ins.startswith("s_waitcnt") and "vmcnt" in ins]
    print(f"{workload}: {len(tail)} instructions between the last barrier and s_endpgm, "
          f"{sum(bool(re.match(r'(buffer|global|flat)_store', ins)) for ins in tail)} of them stores")
    assert any(re.match(r"buffer_store_dwordx4", ins) for ins in tail), "the state stores are on this path"
    assert not waits, waits
    assert barriers_x > len(barriers), (barriers_x, len(barriers))
    # The per-environment rows (3 collision id sets: 64-bit; 11 counters, tick, noise-stream position) leave through their buffer resource as
    # the LAST 16 stores of the path, behind every 12- / 16-byte state store, and behind the observation copy-out (whose pointer loop is the
    # only 64-bit address arithmetic of the path) nothing builds a 64-bit address any more: one scalar row offset per store.
    stores = [(n, ins.split()[0]) for n, ins in enumerate(tail) if ins.startswith("buffer_store_")]
    rows = stores[-16:]
    assert sorted(kind for _, kind in rows) == ["buffer_store_dword"] * 13 + ["buffer_store_dwordx2"] * 3, rows
    wide = [n for n, kind in stores if kind in ("buffer_store_dwordx3", "buffer_store_dwordx4")]
    assert len(wide) == 11 and max(wide) < rows[0][0], (wide, rows[0])
    resources = {re.search(r"s\[\d+:\d+\]", tail[n]).group(0) for n, _ in rows}
    assert len(resources) == 1 and resources != {re.search(r"s\[\d+:\d+\]", tail[wide[0]]).group(0)}, resources
    copy_out = max(n for n, ins in enumerate(tail) if ins.startswith("global_store_"))
    loop_end = next(n for n in range(copy_out, len(tail)) if tail[n].startswith("s_cbranch"))   # (the copy-out loop's backward branch)
    chains = [ins for ins in tail[loop_end:] if re.match(r"v_lshl_add_u64|v_ashrrev_i32|v_lshlrev_b64|global_store_|flat_store_", ins)]
    assert not chains, chains

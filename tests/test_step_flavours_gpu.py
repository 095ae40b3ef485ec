"""The one-step team kernel without the exchange epilogue, and its per-environment rows through the buffer resource, compute the same BITS
as the forms they replace - and the exchange still runs, in the kernel of its own.

(1) `-DQS_XCHG_INLINE=1` restores the single body with the run-time test on the exchange descriptor (qs_step_team_modes.inc);
    `-DQS_ENV_ROWS_FLAT=0` restores the typed pointers for the counters, tick, noise-stream position and collision id sets (qs_step_team.inc).
    Neither touches an arithmetic instruction: every output and state array is compared bit for bit after every control step of a free-running
    rollout with the crafted events of the parity suite (tests/test_object_identity_gpu.py identical_rollout, exact).  8 drones on the 8-wave
    lane-major kernels (with downwash / with obstacles), 32 on the 4-wave row kernels, and 5 and 12 drones: idle lanes, a partly filled last
    workgroup (7 environments), both team widths.
(2) A world-size-1 exchange attached to a 16-environment handle: the handle reports and launches `qs_spec_step_x`, computes what a handle
    without exchange computes, and returns to `qs_spec_step` when the exchange is detached.
"""
import numpy as np
import pytest

from tests import test_hip_parity as thp
from tests.test_object_identity_gpu import _bits, identical_rollout

pytestmark = pytest.mark.gpu

FLAVOUR_CASES = ["c2_n8_dw", "c3_n8_obst", "c4_n32_svs", "c2_n5_kall_short", "c4_n12_svs_short"]   # 8, 8, 32, 5, 12 drones
FLAVOUR_FLAGS = ["-DQS_XCHG_INLINE=1", "-DQS_ENV_ROWS_FLAT=0"]
XCHG_ENVS = 16


@pytest.mark.parametrize("flag", FLAVOUR_FLAGS)
@pytest.mark.parametrize("case", FLAVOUR_CASES)
def test_default_build_equals_the_form_it_replaces(case, flag, monkeypatch):
    assert thp.CASES[case]["num_agents"] == {"c2_n8_dw": 8, "c3_n8_obst": 8, "c4_n32_svs": 32, "c2_n5_kall_short": 5, "c4_n12_svs_short": 12}[case]
    monkeypatch.setenv("QS_TEAM", "1")
    identical_rollout(case, 7, 45, "QS_SPEC_EXTRA_FLAGS", flag, expect_team=True, precision="f32", exact=True)


def test_an_attached_exchange_runs_the_kernel_with_the_epilogue_and_changes_no_result():
    import torch
    from quad_swarm_rl_amd import config as qcfg, native, parallel
    from tests import xchg_worker as xw
    E, steps = XCHG_ENVS, 20
    cfg = qcfg.make_config(num_envs=E, seed=7, precision="f32", write_rew_info=False, **xw.KW)
    acts = torch.as_tensor(xw.global_actions(steps, E, cfg.num_agents)).cuda()
    ref = native.Stepper(cfg, device=0)
    st = native.Stepper(cfg, device=0)
    assert ref.specialized and st.specialized and st.team, (ref.spec_note, st.spec_note)
    assert st.kernel_name == "qs_spec_step" and ref.kernel_name == "qs_spec_step"
    ex = parallel.ObsExchange(st, 1, 0, transport="fused", wire="f32")
    ex.reset()
    ref.reset()
    assert st.kernel_name == "qs_spec_step_x" and ref.kernel_name == "qs_spec_step"
    for t in range(steps):
        ex.step(acts[t].data_ptr())
        ref.step(acts[t].data_ptr())
        torch.cuda.synchronize()
        for nm in ("obs", "reward", "done"):
            a, b = ref.to_host(nm), st.to_host(nm)
            assert np.array_equal(_bits(a), _bits(b)), (nm, t)
        assert torch.equal(ex.latest().reshape(-1), ref.tensor("obs").reshape(-1)), t   # (and the rows did travel: the f32 wire is bit-exact)
    assert ex.status()["error"] == 0
    ex.pause()
    assert st.kernel_name == "qs_spec_step"
    st.step(acts[0].data_ptr()); ref.step(acts[0].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ref.to_host("obs")), _bits(st.to_host("obs")))
    st.check_errors(); ref.check_errors()
    ex.close()
    st.close()
    ref.close()

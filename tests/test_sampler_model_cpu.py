"""tests/sampler_model.py (the float64 specification of the rollout's Gaussian sampler) against published Philox vectors and the normal
distribution; the inputs of tests/test_encoder_epilogues_gpu.py against the model's mutants; its case table against the encoder's kernel table.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_model as sm  # noqa: E402
from tests import encoder_epilogue_cases as cases  # noqa: E402
from tests import test_enc_select as sel  # noqa: E402
from tests.test_encoder_epilogues_gpu import SAMPLER_Z_TOL, SAMPLER_Z_TOL_CAP  # noqa: E402

# Random123 (tests/kat_vectors): philox4x32-10, counter, key -> output
KNOWN_ANSWERS = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def test_philox_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        assert [int(x) for x in sm.philox4x32_10(np.array(counter), np.array(key))] == want
    # vectorised over leading axes: the three at once
    got = sm.philox4x32_10(np.array([c for c, _, _ in KNOWN_ANSWERS]), np.array([k for _, k, _ in KNOWN_ANSWERS]))
    assert got.tolist() == [w for _, _, w in KNOWN_ANSWERS]
    assert sm.philox4x32_10(np.array(KNOWN_ANSWERS[2][0]), np.array(KNOWN_ANSWERS[2][1]), rounds=9).tolist() != KNOWN_ANSWERS[2][2]


N_AGENTS = 1 << 17     # x 8 components = 2^20 draws per pass


@pytest.fixture(scope="module")
def draws():
    seed, counter = 0x243F6A8885A308D3, 41
    return {"u": sm.uniforms(seed, counter, 0, N_AGENTS, 8), "z": sm.normals(seed, counter, 0, N_AGENTS, 8), "z_next": sm.normals(seed, counter, 1, N_AGENTS, 8)}


def test_uniforms_are_strictly_inside_the_unit_interval(draws):
    ua, ub = draws["u"]
    assert ua.min() > 0.0 and ub.min() > 0.0 and ua.max() < 1.0 and ub.max() < 1.0
    # and at the ends of the 23-bit range: word 0 and word 0xffffffff
    to_u = lambda w: ((w >> 9) + 0.5) / 8388608.0
    assert to_u(0) == 2.0 ** -24 and to_u(0xffffffff) == 1.0 - 2.0 ** -24
    assert abs(ua.mean() - 0.5) < 5.0 / np.sqrt(12.0 * ua.size) and abs(ub.mean() - 0.5) < 5.0 / np.sqrt(12.0 * ub.size)


def test_draws_are_standard_normal(draws):
    from scipy import stats
    z = draws["z"].ravel()
    n = z.size
    assert n >= 1 << 20 and np.isfinite(z).all()
    assert abs(z.mean()) < 5.0 / np.sqrt(n)                        # five standard errors of the mean ...
    assert abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)             # ... and of the variance of a normal sample
    assert stats.kstest(z, stats.norm.cdf).pvalue > 1e-3
    for h in range(8):                                             # every component by itself as well
        assert stats.kstest(draws["z"][:, h], stats.norm.cdf).pvalue > 1e-4, h


def test_components_and_consecutive_counters_are_uncorrelated(draws):
    z, z_next = draws["z"], draws["z_next"]
    lim = 5.0 / np.sqrt(z.shape[0])                                # five standard errors of a sample correlation of independent draws
    c = np.corrcoef(z, rowvar=False)
    assert np.abs(c - np.eye(8)).max() < lim                       # the 28 pairs of one agent, the two halves of a Box-Muller pair among them
    cross = np.corrcoef(np.concatenate((z, z_next), axis=1), rowvar=False)[:8, 8:]
    assert np.abs(cross).max() < lim                               # counter c against counter c + 1, same and different components
    assert abs(np.corrcoef(z[:-1].ravel(), z[1:].ravel())[0, 1]) < 5.0 / np.sqrt(z.size - 8)    # agent a against agent a + 1
    # squares too: a Box-Muller pair shares its radius only through independent angles
    assert np.abs(np.corrcoef(z ** 2, rowvar=False) - np.eye(8)).max() < lim


_true = {}


def discriminated(inp, mutant, z_tol):
    """does some draw of `inp` differ between the model and its mutant by more than the GPU bound, whatever the means (|mean| <= HEAD_ABS_MAX)"""
    sigma = np.array(cases.SIGMAS[:inp.head_dim])[None, :]
    if inp not in _true:
        _true[inp] = sm.normals(inp.seed, inp.counter, inp.step, inp.agents, inp.head_dim)
    z = _true[inp]
    zm = sm.normals(inp.seed, inp.counter, inp.step, inp.agents, inp.head_dim, mutant)
    allowed = sm.bound(cases.HEAD_ABS_MAX, sigma, z, z_tol)
    return bool((~(np.abs(sigma * (zm - z)) <= allowed)).any())   # (a nan / inf from a mutant differs)


def test_the_bound_is_what_the_issue_allows():
    assert 0.0 < SAMPLER_Z_TOL <= SAMPLER_Z_TOL_CAP == 1e-4


@pytest.mark.parametrize("mutant", sm.MUTANTS)
def test_the_gpu_inputs_separate_the_model_from_every_mutant(mutant):
    """per code site that draws (the encoders' epilogue, qs_rollout_pre): at least one (seed, counter, step, B, head_dim) the GPU tests run
    on that site puts the mutant above their bound - at the bound's cap, so also at any smaller measured constant"""
    inputs = cases.sampler_inputs()
    not_applicable = {"pre": {"step_ignored", "group_zero"}}      # qs_rollout_pre has no step and one group (head_dim == 4)
    for site in ("epilogue", "pre"):
        if mutant in not_applicable.get(site, ()):
            continue
        hits = [inp for inp in inputs if inp.site == site and discriminated(inp, mutant, SAMPLER_Z_TOL_CAP)]
        assert hits, (site, mutant)


def test_every_input_of_the_matrix_is_its_own():
    inputs = [i for i in cases.sampler_inputs() if i.site == "epilogue"]
    keys = {(i.seed, (i.counter + i.step) & 0xFFFFFFFF) for i in inputs}
    n_matrix = len(cases.CONFIGS) * len(cases.SHAPES) + len(cases.TAIL_CONFIGS)
    assert len({(i.seed, i.counter, i.step) for i in inputs[:n_matrix]}) == n_matrix and len(keys) >= n_matrix
    assert any(i.step == 0 for i in inputs[:n_matrix]) and any(i.step > 0 for i in inputs[:n_matrix])
    assert all(i.seed >> 32 and i.seed & 0xFFFFFFFF for i in inputs[:n_matrix])


def test_the_case_table_reaches_every_kernel_of_the_encoder():
    """every configuration selects the kernels it names - by the selection rule tests/test_enc_select.py holds the host code to - at every
    batch size of the matrix, and together they are the 25 kernels of the table: a kernel added there without an epilogue case fails here"""
    reached = set()
    assert len({c.name for c in cases.CONFIGS}) == len(cases.CONFIGS)
    for c in cases.CONFIGS:
        for B, _ in cases.SHAPES + ([cases.TAIL_SHAPE] if c.name in cases.TAIL_CONFIGS else []):
            assert sel.expected(c.precision, c.model, c.num_nbr, c.obst_dim, c.pingpong, 1 if c.wide else 0, B) == c.kernels, (c.name, B)
        reached.update(f"qs_encoder{'_' if k else ''}{k}_kernel" for k in c.kernels)
    assert reached == set(sel.KERNELS) and len(reached) == 25
    assert all(name in [c.name for c in cases.CONFIGS] for name in cases.TAIL_CONFIGS + cases.COUNTER_CONFIGS)

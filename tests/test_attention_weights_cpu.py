"""The attention probe without a GPU (include/quadswarm_attention.h, quad_swarm_rl_amd/attention.py): the torch statement of the weights against
what the REFERENCE classes computed (tests/golden/attnw_*.npz, taken with forward hooks by tools/capture_attention_weights.py), the two helpers of
the paper's figure against numpy by hand, the new prototypes against the header text and the library's exports, and every refusal of
qs_attn_weights / qs_attn_row_elems before anything could be launched.

The -2 of a failed launch is not provoked here: on a machine with a GPU the same call would be a launch on poisoned pointers."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import attention_weights_cases as awc
from tests import test_abi_layout as tal

from quad_swarm_rl_amd import abi, attention, policy

HEADER = "quadswarm_attention.h"
ATT, MHA, S2R = abi.QS_ENC_NBR_ATTENTION, abi.QS_ENC_MODEL_MHA, abi.QS_ENC_MODEL_S2R


def test_fixtures_present():
    assert awc.CASES == sorted(awc.EXPECTED)
    for case, (cls, H, K, obst, B) in awc.EXPECTED.items():
        g = np.load(os.path.join(awc.GOLDEN, f"attnw_{case}.npz"))
        assert (str(g["cls"]), int(g["rnn_size"]), int(g["num_nbr"]), int(g["obst_dim"]), g["obs"].shape[0]) == (cls, H, K, obst, B)
        assert B <= 37 and g["weights"].dtype == np.float32
        assert g["weights"].shape == {"multi": (B, K), "mha": (B, 4, 2, 2), "s2r": (B, 2, 2)}[cls]


@pytest.mark.parametrize("case", sorted(awc.EXPECTED))
def test_reference_statement_reproduces_the_reference_class(case):
    """attention_weights_reference of the seeded restatement == the weights hooked out of the reference class, to 1e-6; rows sum to 1"""
    import torch
    from tests.test_encoder_fixtures import reference_names
    g, m = awc.load(case)
    sums = np.array([[float(v.double().sum()), float(v.double().abs().sum())] for _, v in sorted(reference_names(m).items())])
    np.testing.assert_allclose(sums, g["weight_sums"], rtol=1e-12, atol=1e-12, err_msg="the fixture's weights are not reproduced on this torch build")
    obs = torch.from_numpy(g["obs"])
    w = attention.attention_weights_reference(m, obs)
    assert w.dtype == torch.float32 and tuple(w.shape) == g["weights"].shape
    err = float(np.abs(w.numpy() - g["weights"]).max())
    with torch.no_grad():
        err_out = float(np.abs(m(obs).numpy() - g["out"]).max())
    print(f"\n{case}: max |reference statement - reference class| = {err:.2e} (weights), {err_out:.2e} (output); row sums off by "
          f"{awc.row_sum_error(w.numpy()):.2e} / {awc.row_sum_error(g['weights']):.2e}")
    assert err <= awc.RESTATEMENT_TOL and err_out <= awc.RESTATEMENT_TOL
    assert awc.row_sum_error(w.numpy()) <= awc.ROW_SUM_TOL and awc.row_sum_error(g["weights"]) <= awc.ROW_SUM_TOL
    import copy
    w64 = attention.attention_weights_reference(copy.deepcopy(m).double(), obs.double())     # the module's dtype
    assert w64.dtype == torch.float64 and float((w64 - w.double()).abs().max()) <= 1e-5
    assert next(m.parameters()).dtype == torch.float32


def test_modules_without_attention_are_refused():
    import torch
    for kind in ("mean_embed", "mlp", "no_encoder"):
        m = policy.make_reference_encoder(nbr_encoder=kind, num_nbr=2)
        with pytest.raises(NotImplementedError):
            attention.AttentionProbe(m)
        with pytest.raises(NotImplementedError):
            attention.attention_weights_reference(m, torch.zeros(2, 30))
    with pytest.raises(NotImplementedError):                                   # an attention encoder without neighbours has no neighbour encoder
        attention.AttentionProbe(policy.make_reference_encoder(nbr_encoder="attention", num_nbr=0))
    with pytest.raises(NotImplementedError):                                   # widths FusedQuadEncoder does not take
        attention.AttentionProbe(policy.make_reference_encoder(nbr_encoder="attention", num_nbr=2, hidden=128))
    with pytest.raises(NotImplementedError):
        attention.AttentionProbe(policy.make_reference_sim2real_encoder(hidden=48))
    with pytest.raises(NotImplementedError):                                   # narrow widths are the Sim2Real class's alone
        attention.AttentionProbe(policy.make_reference_mha_encoder(hidden=32))


def test_zero_neighbor_velocity_by_hand():
    import torch
    self_dim, K = 5, 3
    obs = np.arange(1, 2 * (self_dim + 6 * K + 4) + 1, dtype=np.float32).reshape(2, -1)
    want = obs.copy()
    for k in range(K):
        for c in (3, 4, 5):
            want[:, self_dim + 6 * k + c] = 0.0
    got = attention.zero_neighbor_velocity(obs, self_dim, K)
    assert got is not obs and np.array_equal(got, want) and obs[0, self_dim + 3] != 0.0      # a copy: the rows themselves are untouched
    assert int((got == 0).sum()) == 2 * 3 * K
    t = torch.from_numpy(obs)
    got_t = attention.zero_neighbor_velocity(t, self_dim, K)
    assert got_t is not t and np.array_equal(got_t.numpy(), want) and np.array_equal(t.numpy(), obs)
    assert np.array_equal(attention.zero_neighbor_velocity(obs, self_dim, 0), obs)


def test_attention_matrix_by_hand():
    import torch
    E, N = 2, 4
    w = np.arange(1, E * N * (N - 1) + 1, dtype=np.float32).reshape(E * N, N - 1)
    want = np.zeros((E, N, N), dtype=np.float32)
    for e in range(E):
        for i in range(N):
            others = [j for j in range(N) if j != i]                                           # quadrotor_multi.py:250
            for s, j in enumerate(others):
                want[e, i, j] = w[e * N + i, s]
    got = attention.attention_matrix(w, N)
    assert got.shape == (E, N, N) and got.dtype == np.float32 and np.array_equal(got, want)
    assert all(got[e, i, i] == 0 for e in range(E) for i in range(N))
    got_t = attention.attention_matrix(torch.from_numpy(w), N)
    assert isinstance(got_t, torch.Tensor) and np.array_equal(got_t.numpy(), want)
    for bad, n in ((w, 5), (w, 3), (w[:7], 4), (w.reshape(-1), 4), (w, 1)):                    # K != N - 1, rows not whole environments, not a matrix
        with pytest.raises(ValueError):
            attention.attention_matrix(bad, n)


def test_prototypes_header_and_exports():
    table, decl = abi.QUADSWARM_ATTENTION_H, tal.declared(HEADER)
    assert sorted(abi.names(table)) == sorted(decl) == ["qs_attn_row_elems", "qs_attn_weights"]
    for name, restype, argtypes in table:
        ret, nargs = decl[name]
        assert len(argtypes) == nargs and restype is tal.RESTYPE[ret], name
    text = tal.strip_comments(open(os.path.join(tal.INCLUDE, HEADER)).read())
    assert "#define QS_" not in text and "typedef" not in text                                 # no constant, no struct: nothing else to mirror
    enc = open(os.path.join(tal.INCLUDE, "quadswarm_encoder.h")).read()
    assert enc.index('#include "quadswarm_valuemap.h"') < enc.index(f'#include "{HEADER}"')    # part of the library's one header
    policy.build()
    lib = C.CDLL(policy.ENC_LIB_PATH)
    for name in abi.names(table):
        assert hasattr(lib, name), name
    assert any(os.path.basename(s) == "qs_attn_weights.inc" for s in policy.ENC_SOURCES) and any(os.path.basename(s) == HEADER for s in policy.ENC_SOURCES)


POISON = 4096   # a small non-NULL value: nothing may be dereferenced on the host, and every call below is refused before a launch


def _layer(M, K, bias=True):
    return abi.EncLayer(POISON, POISON if bias else None, M, K)


def _params(model, H=256, K=2, **kw):
    """the fields the weights depend on, valid and poisoned; everything else zero"""
    P = abi.EncParams()
    P.self_dim, P.nbr_dim, P.num_nbr, P.obst_dim, P.nbr_encoder, P.precision = 18, 6, K, 0 if model == ATT else 9, model, 1
    P.obs_dim = P.self_dim + P.nbr_dim * K + P.obst_dim
    kn = -(-6 * K // 32) * 32
    if model == ATT:
        P.n1, P.n2, P.a1e, P.a1m, P.a2 = _layer(256, 32), _layer(256, 256), _layer(256, 256), _layer(256, 256, bias=False), _layer(256, 256)
        P.a3w, P.ebuf, P.gbuf = POISON, POISON, POISON
    elif model == MHA:
        P.n1, P.n2, P.o1, P.o2 = _layer(256, kn), _layer(256, 256), _layer(256, 32), _layer(256, 256)
        P.mq, P.mk = _layer(1024, 256, bias=False), _layer(1024, 256, bias=False)
    else:
        kh = -(-H // 32) * 32
        P.n1, P.o1, P.mq, P.mk = _layer(H, kn), _layer(H, 32), _layer(H, kh, bias=False), _layer(H, kh, bias=False)
    for k, v in kw.items():
        if "." in k:
            layer, field = k.split(".")
            setattr(getattr(P, layer), field, v)
        else:
            setattr(P, k, v)
    return P


def test_refusals_come_before_any_launch():
    """every -1 and -4 of include/quadswarm_attention.h with a NULL stream and poisoned device pointers: a launch, or a host dereference of 4096,
    would not return the code with a message"""
    policy.build()
    lib = C.CDLL(policy.ENC_LIB_PATH)
    abi.bind(lib, abi.QUADSWARM_ATTENTION_H + [r for r in abi.QUADSWARM_ENCODER_H if r[0] == "qs_enc_last_error"])

    def call(P, obs=POISON, B=17, weights=POISON):
        rc = lib.qs_attn_weights(obs, B, C.byref(P) if P is not None else None, weights, None)
        assert rc != 0 and lib.qs_enc_last_error().startswith(b"qs_attn_weights: "), (rc, lib.qs_enc_last_error())
        return rc

    # the valid blocks themselves answer their row sizes (no pointer is looked at) ...
    assert lib.qs_attn_row_elems(C.byref(_params(ATT, K=6))) == 6 and lib.qs_attn_row_elems(C.byref(_params(ATT, K=1))) == 1
    assert lib.qs_attn_row_elems(C.byref(_params(MHA))) == 16 and lib.qs_attn_row_elems(C.byref(_params(MHA, K=6))) == 16
    for H in (16, 32, 64, 256):
        assert lib.qs_attn_row_elems(C.byref(_params(S2R, H=H, K=6))) == 4
    assert lib.qs_attn_row_elems(None) == -1 and lib.qs_enc_last_error().startswith(b"qs_attn_row_elems: ")
    # -1: a NULL required pointer, B < 1
    for model in (ATT, MHA, S2R):
        P = _params(model)
        assert call(P, obs=None) == -1 and call(P, weights=None) == -1 and call(P, B=0) == -1 and call(P, B=-5) == -1
    assert call(None) == -1
    required = {ATT: ["n1.w", "n1.b", "n2.w", "n2.b", "a1e.w", "a1e.b", "a1m.w", "a2.w", "a2.b", "a3w", "ebuf", "gbuf"],
                MHA: ["n1.w", "n1.b", "n2.w", "n2.b", "o1.w", "o1.b", "o2.w", "o2.b", "mq.w", "mk.w"],
                S2R: ["n1.w", "n1.b", "o1.w", "o1.b", "mq.w", "mk.w"]}
    for model, fields in required.items():
        for f in fields:
            assert call(_params(model, **{f: None})) == -1, (model, f)
    assert call(_params(S2R, H=16, K=6, **{"mk.w": None})) == -1
    # -4: encoders without attention, attention without neighbours, another precision
    for model in (abi.QS_ENC_NBR_MEAN_EMBED, abi.QS_ENC_NBR_MLP, abi.QS_ENC_NBR_NONE, -1, 6):
        P = _params(ATT, nbr_encoder=model)
        assert call(P) == -4 and lib.qs_attn_row_elems(C.byref(P)) == -4, model
    assert call(_params(ATT, num_nbr=0)) == -4
    for model in (ATT, MHA, S2R):
        for precision in (0, 2):
            assert call(_params(model, precision=precision)) == -4, (model, precision)
    # -4: the shapes qs_enc_forward refuses
    bad = [(ATT, dict(num_nbr=9)), (ATT, dict(self_dim=27)), (ATT, dict(nbr_dim=33)), (ATT, dict(self_dim=33)), (MHA, dict(num_nbr=9)),
           (MHA, dict(nbr_dim=11, num_nbr=6)), (MHA, dict(obst_dim=0)), (MHA, dict(num_nbr=0)), (MHA, dict(obst_dim=33)), (S2R, dict(obst_dim=0)),
           (S2R, dict(num_nbr=0)), (ATT, dict(obs_dim=20))]
    for model, kw in bad:
        P = _params(model, **kw)
        assert call(P) == -4 and lib.qs_attn_row_elems(C.byref(P)) == -4, (model, kw)
    # -4: widths that are not built, layers that disagree
    for H in (8, 48, 128, 512):
        assert call(_params(S2R, H=H)) == -4, H
    for kw in ({"o1.M": 32}, {"mq.M": 32}, {"mk.M": 64}, {"mq.K": 64}, {"mk.K": 0}, {"n1.K": 64}):
        assert call(_params(S2R, H=16, K=2, **kw)) == -4, kw
    for model, kw in ((ATT, {"n1.K": 64}), (ATT, {"a2.M": 128}), (ATT, {"a1m.K": 512}), (MHA, {"mq.M": 256}), (MHA, {"n1.K": 64}), (MHA, {"o2.M": 0}),
                      (S2R, {"mq.M": 1024})):
        assert call(_params(model, **kw)) == -4, (model, kw)
    # -4: a batch whose scratch offsets do not fit 32 bits
    assert call(_params(ATT, K=8), B=1 << 19) == -4
    # what is ignored may be anything: the refusals above do not depend on it, and a valid block stays valid
    P = _params(MHA)
    P.head_dim, P.sample_step, P.s1.M, P.f.K = 99, 7, 3, 5
    assert lib.qs_attn_row_elems(C.byref(P)) == 16

"""lfgpu_eval_quad_batch256: ProverLayers::eval_quad (nc = 1) over Fp256Base for nb statements of one quad.  Every statement's
outputs must equal the Python-integer model's V[g] = sum k W[h1] W[h0] (tests/p256_layer_model.py) and lfgpu_eval_quad on that
statement alone; ok[b] is 0 only for the statement whose wires break an assert-zero term, and the others are unaffected.

Shapes (logv, logw, terms, nv, nw): `tiny` (2, 3, 8, 3, 5) and `wide` (2, 6, 300, 3, 64), whose three gates have about a
hundred terms each -- more than the 64 lanes of a wave, so a gate's run crosses waves and blocks.  ldw and ldv are padded."""
import numpy as np
import pytest

import p256_layer_model as M
from oracle_lib import FP
from test_sumcheck_layer_random import make_layer_vec

P256 = 1
SHAPES = {"tiny": (2, 3, 8, 3, 5), "wide": (2, 6, 300, 3, 64)}
MAX_B = 64
PAD_WORD = 0xA5A5A5A5A5A5A5A5
_problems = {}


def problem(name):
    """the layer, with two assert-zero terms (vi = 0, kvec[0] = 0), and MAX_B wire vectors that satisfy them; plus one
    vector that does not.  Per statement the model's outputs, computed once."""
    if name not in _problems:
        logv, logw, nterms, nv, nw = SHAPES[name]
        rng = np.random.default_rng(2560 + nterms)
        L = make_layer_vec(rng, FP, logv, logw, nterms, 9, nv, nw)
        L["kvec"] = M.rand_images(rng, 9)
        L["kvec"][0] = 0
        del L["W"]
        zt = [0, L["n"] // 2]  # the assert-zero terms
        L["vi"] = L["vi"].copy()
        L["vi"][zt] = 0
        Ws = []
        for _ in range(MAX_B):
            W = M.rand_images(rng, nw)
            W[L["h0"][zt]] = 0  # one factor of each assert-zero product vanishes
            Ws.append(W)
        Wbad = M.rand_images(rng, nw)
        assert all(Wbad[L["h0"][t]].any() and Wbad[L["h1"][t]].any() for t in zt)
        want = []
        for W in Ws:
            V, ok = M.eval_quad(M.P256, L, L["kvec"], W)
            assert ok
            want.append(V)
        assert not M.eval_quad(M.P256, L, L["kvec"], Wbad)[1]
        if name == "wide":
            assert np.bincount(L["g"]).max() > 64
        _problems[name] = (L, Ws, Wbad, want)
    return _problems[name]


def run_batch(q, L, Ws, pad_w=3, pad_v=2):
    import gpu_util as G
    B, nw, nv = len(Ws), L["nw"], L["nv"]
    Wb = np.full((B, nw + pad_w, 4), PAD_WORD, dtype=np.uint64)
    for b in range(B):
        Wb[b, :nw] = Ws[b]
    dW = G.to_dev(Wb)
    dV = G.to_dev(np.full((B, nv + pad_v, 4), PAD_WORD, dtype=np.uint64))
    ok = q.eval_quad_batch256(B, nw, dW.data_ptr(), nw + pad_w, dV.data_ptr(), nv + pad_v)
    V = G.from_dev(dV, np.uint64, (B, nv + pad_v, 4))
    assert (V[:, nv:] == PAD_WORD).all(), "the padding of d_V was written"
    assert (G.from_dev(dW, np.uint64, Wb.shape) == Wb).all()
    return ok, V[:, :nv]


def run_single(q, L, W):
    import gpu_util as G
    dW, dV = G.to_dev(W), G.to_dev(np.zeros((L["nv"], 4), dtype=np.uint64))
    ok = q.eval(L["nw"], dW.data_ptr(), dV.data_ptr())
    return ok, G.from_dev(dV, np.uint64, (L["nv"], 4))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_model_and_single_call(name, B):
    import gpu_util as G
    L, Ws, _, want = problem(name)
    q = G.pkg.Quad(G.gpu(), P256, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], L["nv"])
    ok, V = run_batch(q, L, Ws[:B])
    assert ok == [True] * B
    for b in range(B):
        assert (V[b] == want[b]).all(), "statement %d vs the model" % b
    for b in sorted({0, B // 2, B - 1}):
        sok, sV = run_single(q, L, Ws[b])
        assert sok and (sV == V[b]).all(), "statement %d vs lfgpu_eval_quad" % b
    q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_failing_statement_leaves_the_others_alone(name):
    import gpu_util as G
    L, Ws, Wbad, want = problem(name)
    B, bad = 3, 1
    q = G.pkg.Quad(G.gpu(), P256, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], L["nv"])
    ok, V = run_batch(q, L, [Ws[0], Wbad, Ws[2]])
    assert ok == [b != bad for b in range(B)]
    for b in (0, 2):
        assert (V[b] == want[b]).all(), "statement %d vs the model" % b
    assert run_single(q, L, Wbad)[0] is False
    q.close()


@pytest.mark.gpu
def test_argument_errors():
    import gpu_util as G
    from oracle_lib import GF
    L, Ws, _, want = problem("tiny")
    nw, nv = L["nw"], L["nv"]
    q = G.pkg.Quad(G.gpu(), P256, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], nv)
    qgf = G.pkg.Quad(G.gpu(), GF, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"][:, :2].copy(), nv)
    dW, dV = G.to_dev(np.zeros((65, nw + 1, 4), dtype=np.uint64)), G.to_dev(np.zeros((65, nv + 1, 4), dtype=np.uint64))
    hmax = int(max(L["h0"].max(), L["h1"].max()))
    for bad, B, n, ldw, ldv in ((q, 0, nw, nw, nv), (q, 65, nw, nw, nv), (q, 3, nw, nw - 1, nv), (q, 3, hmax, nw, nv), (q, 3, nw, nw, nv - 1), (qgf, 3, nw, nw, nv)):
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):  # LFGPU_ERR_ARG
            bad.eval_quad_batch256(B, n, dW.data_ptr(), ldw, dV.data_ptr(), ldv)
        ok, V = run_batch(q, L, Ws[:3])  # a valid call passes afterwards
        assert ok == [True] * 3 and all((V[b] == want[b]).all() for b in range(3))
    qgf.close()
    q.close()

"""lfgpu_sumcheck_layer256 -- the Fp256Base sumcheck layer that lfgpu_zk_prove runs, reached on its own through the kernel
ABI -- against the Python-integer model of ProverLayers::layer (tests/p256_layer_model.py): every round-hand's three
evaluations, wc_out, bound_quad, the challenges handed back as g_out, the callback order, and d_W left intact.

Shapes: `one`, `tiny`, `small` and `cross` of tests/test_sumcheck_layer_batch256.py (shared, so the model runs once per
statement), and `grid` (11, 13, 9000): its HQUAD and wires start above the resident grid's default hand-off (2048 entries),
so the layer opens on the per-launch kernels and then hands over."""
import numpy as np
import pytest

import p256_layer_model as M
import test_sumcheck_layer_batch256 as T
from oracle_lib import FP
from test_sumcheck_layer_random import make_layer_vec

GRID_HANDOFF = 2048  # the default of LFGPU_P256_GRID_MAX (csrc/zk256.hip)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "tiny", "small", "cross"])
def test_single_layer_equals_the_model(name):
    q = T.new_quad(name)
    got = T.run_single(q, name, 0)  # also checks that the wires come back unchanged
    q.close()
    T.check_statement(name, 0, got, single=False)


@pytest.mark.gpu
def test_layer_that_starts_above_the_grid_handoff():
    import gpu_util as G
    logv, logw, nterms = 11, 13, 9000
    rng = np.random.default_rng(11139000)
    L = make_layer_vec(rng, FP, logv, logw, nterms)
    kvec = M.rand_images(rng, 9)
    kvec[0] = 0
    W, G0, G1 = M.rand_images(rng, L["nw"]), M.rand_images(rng, logv), M.rand_images(rng, logv)
    alpha, beta = (T._tup(M.rand_images(rng, 1)[0]) for _ in range(2))
    wc_in = [T._tup(e) for e in M.rand_images(rng, 2)]
    chal = [T._tup(e) for e in M.rand_images(rng, 2 * logw)]
    want_ev, want_wc, want_bq, nh0 = M.layer(M.P256, L, kvec, W, logv, G0, G1, alpha, beta, wc_in, chal)
    assert nh0 > GRID_HANDOFF and L["nw"] > GRID_HANDOFF
    q = G.pkg.Quad(G.gpu(), T.P256, L["g"], L["h0"], L["h1"], L["vi"], kvec, L["nv"])
    dW = G.to_dev(W)
    got, order = [], []

    def cb(hand, rnd, ev):
        got.append(tuple(T._tup(e) for e in ev))
        order.append((rnd, hand))
        return chal[len(got) - 1]

    wc, ch, bq = q.sumcheck_layer256(logv, G0, G1, alpha, beta, logw, L["nw"], dW.data_ptr(), wc_in, cb)
    q.close()
    assert order == [(r, h) for r in range(logw) for h in (0, 1)]
    for i, (x, y) in enumerate(zip(got, want_ev)):
        assert x == y, "round-hand %d" % i
    assert len(got) == len(want_ev) == 2 * logw
    assert [T._tup(w) for w in wc] == want_wc and T._tup(bq) == want_bq
    assert [[T._tup(c) for c in ch[h]] for h in (0, 1)] == [[chal[2 * r + h] for r in range(logw)] for h in (0, 1)]
    assert (G.from_dev(dW, np.uint64, W.shape) == W).all(), "lfgpu_sumcheck_layer256 modified d_W"


@pytest.mark.gpu
def test_a_quad_of_a_16_byte_field_is_an_argument_error():
    import gpu_util as G
    from oracle_lib import GF
    name = "tiny"
    L, st, logv, logw = T.problem(name)
    q = T.new_quad(name, GF)
    dW = G.to_dev(np.zeros((L["nw"], 4), dtype=np.uint64))
    one = (1, 0, 0, 0)
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):
        q.sumcheck_layer256(logv, st[0]["G0"], st[0]["G1"], one, one, logw, L["nw"], dW.data_ptr(), [one, one], lambda h, r, ev: one)
    q.close()

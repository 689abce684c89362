"""Pins tests/p256_layer_model.py, the expectation of the Fp256Base sumcheck-layer tests (CPU only, no device):
 - run over the Fp128 modulus 2^128 - 2^108 + 1 with R = 2^128 it must give, byte for byte, what the oracle's step-by-step
   replay (oracle_layer of test_sumcheck_layer_random.py, itself pinned to the compiled reference) gives: every round-hand's
   evaluations, wc_out, bound_quad and the HQUAD size after bind_g, on the shapes `tiny`, `one` and `small`;
 - over the P-256 modulus its products and sums equal lfo_p256_mul / _add / _sub on edge values."""
import itertools

import numpy as np
import pytest

import oracle_lib as ol
import p256_layer_model as M
from oracle_lib import FP
from test_sumcheck_layer_random import make_layer_vec, oracle_layer

SHAPES = {"tiny": (2, 3, 8, 3, 5), "one": (0, 1, 1, 1, 2), "small": (5, 6, 300)}


def _tup(e):
    return tuple(int(x) for x in e)


@pytest.mark.parametrize("name", list(SHAPES))
def test_model_over_fp128_equals_the_oracle_replay(name):
    logv, logw, nterms, *shape = SHAPES[name]
    rng = np.random.default_rng(4242 + logw)
    L = make_layer_vec(rng, FP, logv, logw, nterms, *([9] + shape if shape else []))
    G0, G1 = ol.rand_elts(rng, max(1, logv), FP), ol.rand_elts(rng, max(1, logv), FP)
    alpha, beta = (_tup(ol.rand_elts(rng, 1, FP)[0]) for _ in range(2))
    wc_in = [_tup(e) for e in ol.rand_elts(rng, 2, FP)]
    chal = [_tup(e) for e in ol.rand_elts(rng, 2 * logw, FP)]
    want_ev, want_wc, want_bq, want_nh0 = oracle_layer(FP, L, logv, G0, G1, alpha, beta, wc_in, chal)
    ev, wc, bq, nh0 = M.layer(M.FP128, L, L["kvec"], L["W"], logv, G0, G1, alpha, beta, wc_in, chal)
    assert nh0 == want_nh0
    assert len(ev) == len(want_ev) == 2 * logw
    for i, (a, b) in enumerate(zip(ev, want_ev)):
        assert a == tuple(_tup(e) for e in b), "round-hand %d" % i
    assert wc == [_tup(w) for w in want_wc]
    assert bq == _tup(want_bq)


def test_model_eval_quad_over_fp128_equals_the_oracle():
    rng = np.random.default_rng(77)
    L = make_layer_vec(rng, FP, 5, 6, 300)
    o = ol.oracle()
    want = np.zeros((L["nv"], 2), dtype=np.uint64)
    ok = o.lfo_eval_quad(FP, L["n"], ol.P(L["g"]), ol.P(L["h0"]), ol.P(L["h1"]), ol.P(L["vi"]), ol.P(L["kvec"]), L["nv"], ol.P(L["W"]), ol.P(want))
    got, gok = M.eval_quad(M.FP128, L, L["kvec"], L["W"])
    assert bool(ok) == gok and (got == want).all()


def test_p256_arithmetic_equals_the_oracle_on_edge_values():
    o, F = ol.oracle(), M.P256
    edge = [0, 1, F.p - 1, F.R % F.p]  # each is < p, hence the canonical image of some residue
    words = [tuple((v >> (64 * k)) & (2**64 - 1) for k in range(4)) for v in edge]
    for a, b in itertools.product(words, repeat=2):
        x, y = F.from_image(a), F.from_image(b)
        assert F.to_image(x * y % F.p) == _tup(ol.arr32(o.lfo_p256_mul(ol.e32(a), ol.e32(b))))
        assert F.to_image((x + y) % F.p) == _tup(ol.arr32(o.lfo_p256_add(ol.e32(a), ol.e32(b))))
        assert F.to_image((x - y) % F.p) == _tup(ol.arr32(o.lfo_p256_sub(ol.e32(a), ol.e32(b))))
    assert F.to_image(1) == _tup(ol.arr32(o.lfo_p256_of_scalar(1)))

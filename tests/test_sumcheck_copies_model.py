"""Pins tests/copies_model.py -- the expected values of the GPU tests of the sumcheck over nc copies -- without a GPU:
against the reference's bytes where one copy is the whole circuit (the flatsha fixture), against a second formulation of
the copy rounds that shares no code with the first, against the verifier's identities, and against the oracle's field
arithmetic."""
import os

import numpy as np
import pytest

import copies_model as cm
import oracle_lib as ol
from oracle_lib import FP, GF, P, arr, elt

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _img(rng, field):
    return tuple(int(x) for x in ol.rand_elts(rng, 1, field)[0])


def test_model_reproduces_reference_proof_nb1_with_one_copy():
    """logc = 0, nc = 1: the model's layer() yields the reference prover's bytes for the flatsha-1 circuit"""
    import sumcheck_driver as sd
    circ, W, proof, _ = sd.load_fixture(GOLD, 1)
    assert cm.prove_circuit(circ, W) == proof


def _edge_images(field):
    if field == GF:
        return [(0, 0), (1, 0), (2**64 - 1, 2**64 - 1), (0, 1 << 63)]
    pm1 = cm.FP_P - 1
    return [(0, 0), (1, 0), (pm1 & (2**64 - 1), pm1 >> 64), (2**64 - 1, 0xFFFFEFFFFFFFFFFF)]  # 0, 1/R, p - 1, all ones below p


@pytest.mark.parametrize("field", [GF, FP])
def test_model_field_matches_oracle(field):
    """add / sub / mul of the model (on images) == the oracle's, on random and edge values; inverses; evaluation points"""
    o, F = ol.oracle(), cm.ModelField(field)
    rng = np.random.default_rng(5 + field)
    vals = _edge_images(field) + [_img(rng, field) for _ in range(40)]
    for e in vals:
        assert F.img(F.of_img(e)) == e
    for a in vals:
        for b in vals[:8] + vals[-8:]:
            for name, fn in (("add", o.lfo_add), ("sub", o.lfo_sub), ("mul", o.lfo_mul)):
                want = tuple(int(x) for x in arr(fn(field, elt(a), elt(b))))
                assert F.img(getattr(F, name)(F.of_img(a), F.of_img(b))) == want, (name, a, b)
    for a in vals[4:12]:
        x = F.of_img(a)
        assert F.mul(x, F.inv(x)) == F.one
    for k in range(4):
        want = o.lfo_gf_poly_evaluation_point(ol.gf_ctx(4), k) if field == GF else o.lfo_fp_of_scalar(k)
        assert F.img(F.pts[k]) == tuple(int(x) for x in arr(want))


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 13])
def test_filleq_is_the_product_formula_and_raw_eq2_with_alpha_zero(field, n):
    o, F = ol.oracle(), cm.ModelField(field)
    rng = np.random.default_rng(n + field)
    logn = max(1, (n - 1).bit_length()) + (n % 2)  # also more variables than the entries need
    Qi = ol.rand_elts(rng, logn, field)
    Q = F.of_array(Qi)
    eq = cm.filleq(F, logn, n, Q)
    for i in range(n):
        bits = [F.one if (i >> l) & 1 else F.zero for l in range(logn)]
        assert eq[i] == cm.eq_product(F, logn, Q, bits)
    want = np.zeros((n, 2), dtype=np.uint64)
    o.lfo_raw_eq2(field, logn, n, P(Qi), P(Qi), elt((0, 0)), P(want))
    assert (F.array(eq) == want).all()


def _random_terms(rng, F, field, nw, nc, nterms):
    W = [F.of_array(ol.rand_elts(rng, nc, field)) for _ in range(nw)]
    hc = [(int(a), int(b)) for a, b in rng.integers(0, nw, size=(nterms, 2))]
    hc[0] = (hc[0][0], hc[0][0])  # a term with h0 == h1
    vc = F.of_array(ol.rand_elts(rng, nterms, field))
    return W, hc, vc


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("nc", [2, 3, 5, 8])
def test_copy_round_polynomial_two_formulations(field, nc):
    """the four values of every copy-round polynomial: Karatsuba accumulators + reconstructed coefs[1] (prover_layers.h:415-496)
    == the definition with EQ and W bound at each evaluation point"""
    F = cm.ModelField(field)
    rng = np.random.default_rng(100 * nc + field)
    logc = (nc - 1).bit_length()
    W, hc, vc = _random_terms(rng, F, field, 12, nc, 40)
    EQ = cm.filleq(F, logc, nc, F.of_array(ol.rand_elts(rng, logc, field)))
    for rnd in range(logc):
        direct = cm.evaluations_c_direct(F, EQ, W, hc, vc)
        s = F.add(direct[0], direct[1])  # the claim the prover carries into the round
        assert cm.evaluations_c(F, EQ, W, hc, vc, s) == direct, "round %d" % rnd
        r = F.of_img(_img(rng, field))
        assert cm.evaluations_c_direct(F, EQ, W, hc, vc, [r]) == [F.eval_lagrange(direct, r)]  # the cubic through the four values
        EQ, W = cm.bind_row(F, EQ, r), cm.bind_rows(F, W, r)
    assert len(EQ) == 1


def _synthetic_chain(rng, field, shapes, nterms):
    """layers[0] is the output layer; layer k's nw wires are layer k + 1's outputs"""
    import quad_util as qu
    layers, logv = [], shapes[0][0]
    for logv_, logw in shapes:
        assert logv_ == logv
        layers.append(qu.make_layer(rng, field, logv, logw, min(nterms, (1 << logv) * 3 if logw == 1 else nterms)))
        logv = logw
    return layers


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("nc", [1, 3, 4])
def test_verifier_identities_over_a_chain(field, nc):
    """for every layer: p(0) + p(1) == the running claim in every copy and hand round, and at the end
    sum == eq(Q, C) * bind_gh_all(G, alpha, beta, R, L) * wc0 * wc1 (prover_layers.h:268-269 as the verifier checks it)"""
    o, F = ol.oracle(), cm.ModelField(field)
    rng = np.random.default_rng(40 + nc + field)
    logc = (nc - 1).bit_length() + (1 if nc == 1 else 0)  # nc = 1 with one copy variable: the tail-only rounds
    layers = _synthetic_chain(rng, field, [(3, 5), (5, 4), (4, 1)], 120)
    logv = 3
    # a consistent chain: random inputs at the bottom, every layer's wires are the outputs of the one below
    Ws = [None] * len(layers)
    Ws[-1] = ol.rand_elts(rng, layers[-1]["nw"] * nc, field)
    for k in range(len(layers) - 1, 0, -1):
        ok, Ws[k - 1] = cm.eval_quad_copies(F, layers[k], nc, Ws[k])
        assert ok
    ok, V = cm.eval_quad_copies(F, layers[0], nc, Ws[0])
    Q = [_img(rng, field) for _ in range(logc)]
    G0, G1 = ol.rand_elts(rng, logv, field), ol.rand_elts(rng, logv, field)
    # the true claims on the outputs at (G0, Q) and (G1, Q)
    wc = [cm.mle_claim(F, V, nc, Q, [tuple(int(x) for x in g) for g in G]) for G in (G0, G1)]
    for L, W in zip(layers, Ws):
        alpha, beta = _img(rng, field), _img(rng, field)
        evs = []

        def rc(rnd, ev):
            evs.append(ev)
            return _img(rng, field)

        def rh(hand, rnd, ev):
            evs.append(ev)
            return _img(rng, field)

        res = cm.layer(F, L, logc, nc, Q, logv, G0, G1, alpha, beta, W, wc, rc, rh)
        assert len(evs) == len(res["sums"]) == logc + 2 * L["logw"]
        for ev, s in zip(evs, res["sums"]):
            assert F.img(F.add(F.of_img(ev[0]), F.of_img(ev[1]))) == s
        H0 = np.array(res["g"][0], dtype=np.uint64).reshape(-1, 2)
        H1 = np.array(res["g"][1], dtype=np.uint64).reshape(-1, 2)
        bgh = o.lfo_quad_bind_gh_all(field, L["n"], P(L["g"]), P(L["h0"]), P(L["h1"]), P(L["vi"]), P(L["kvec"]), logv, L["nv"], P(G0), P(G1),
                                     elt(alpha), elt(beta), L["logw"], L["nw"], P(H0), P(H1))
        assert (bgh.l[0], bgh.l[1]) == res["bound_quad"]
        eqqc = cm.eq_product(F, logc, [F.of_img(x) for x in Q], [F.of_img(x) for x in res["q"]])
        if nc == 1 << logc:  # all 2^logc copies present: EQ->scalar() is eq(Q, C)
            assert F.img(eqqc) == res["eq0"]
        want = F.mul(F.of_img(res["eq0"]), F.mul(F.of_img((bgh.l[0], bgh.l[1])), F.mul(F.of_img(res["wc"][0]), F.of_img(res["wc"][1]))))
        assert F.img(want) == res["final_sum"]
        # next layer: its claims, its Q and G
        wc, Q = res["wc"], res["q"]
        G0, G1, logv = H0, H1, L["logw"]


@pytest.mark.parametrize("field", [GF, FP])
def test_eval_quad_copies_is_eval_quad_per_copy(field):
    """the model's eval_quad over copies == the oracle's single-copy eval_quad on every copy's column"""
    import quad_util as qu
    o, F = ol.oracle(), cm.ModelField(field)
    rng = np.random.default_rng(9 + field)
    L = qu.make_layer(rng, field, 4, 5, 150, n_assert=6)
    nc = 3
    W = np.ascontiguousarray(np.repeat(L["W"], nc, axis=0))  # the satisfying assignment in every copy
    W[1::nc] = ol.rand_elts(rng, L["nw"], field)  # copy 1: random wires ...
    for h in L["h0"][L["vi"] == 0]:
        W[int(h) * nc + 1] = 0  # ... that keep the assert-zero terms satisfied
    ok, V = cm.eval_quad_copies(F, L, nc, W)
    assert ok
    for c in range(nc):
        Vc = np.zeros((L["nv"], 2), dtype=np.uint64)
        Wc = np.ascontiguousarray(W[c::nc])
        assert o.lfo_eval_quad(field, L["n"], P(L["g"]), P(L["h0"]), P(L["h1"]), P(L["vi"]), P(L["kvec"]), L["nv"], P(Wc), P(Vc))
        assert (V[c::nc] == Vc).all()
    h = int(L["h0"][L["vi"] == 0][0])
    h1 = int(L["h1"][L["vi"] == 0][0])
    W[h * nc + 2], W[h1 * nc + 2] = (1, 0), (1, 0)
    assert not cm.eval_quad_copies(F, L, nc, W)[0]

"""lfgpu_sumcheck_layer_batch (K14): B statements of one quad in lock-step.  Statement b of the batch must be byte-identical
to (A) the oracle's step-by-step replay of ProverLayers::layer for statement b (evaluations of every round-hand, wc_out,
bound_quad) and (B) lfgpu_sumcheck_layer on the GPU for statement b alone with the same challenges (the same, plus g_out).
Every statement has its own W, G0, G1, alpha, beta, wc_in and challenges from a seeded generator; all share one layer.

Shapes (logv, logw, terms, nv, nw):
  one    0, 1, 1, 1, 2                    a single term, no output variable
  tiny   2, 3, 8, 3, 5                    a single wave, odd at every halving
  small  5, 6, 300                        fused steps from the first round-hand, up to the cap of 64 statements
  cross  11, 15, 20000, 1025, 2^14 + 1    starts on the large (per-launch) kernels -- nh0 > 8192 and nw > 8192 --, crosses to
                                          the fused steps after two halvings, odd sizes throughout"""
import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import FP, GF
from test_sumcheck_layer_random import make_layer_vec, oracle_layer

SMALL_MAX = 8192  # LF_SC_SMALL_MAX (csrc/ctx.h): the largest array the fused single-workgroup step takes
SHAPES = {
    "one": (0, 1, 1, 1, 2),
    "tiny": (2, 3, 8, 3, 5),
    "small": (5, 6, 300),
    "cross": (11, 15, 20000, 1025, (1 << 14) + 1),
}
CASES = [("one", 1), ("one", 3), ("tiny", 1), ("tiny", 3), ("tiny", 16), ("small", 16), ("small", 64), ("cross", 3)]
MAX_B = {"one": 3, "tiny": 16, "small": 64, "cross": 3}

_problems, _oracle, _single = {}, {}, {}


def _tup(e):
    return tuple(int(x) for x in e)


def problem(field, name):
    """the layer and MAX_B statements over it; statement b is the same whatever the batch size"""
    key = (field, name)
    if key not in _problems:
        logv, logw, nterms, *shape = SHAPES[name]
        rng = np.random.default_rng(97 * field + 1000 * logw + logv)
        L = make_layer_vec(rng, field, logv, logw, nterms, *([9] + shape if shape else []))
        st = []
        for _ in range(MAX_B[name]):
            st.append(dict(W=ol.rand_elts(rng, L["nw"], field), G0=ol.rand_elts(rng, max(1, logv), field), G1=ol.rand_elts(rng, max(1, logv), field),
                           alpha=_tup(ol.rand_elts(rng, 1, field)[0]), beta=_tup(ol.rand_elts(rng, 1, field)[0]),
                           wc_in=[_tup(e) for e in ol.rand_elts(rng, 2, field)], chal=[_tup(e) for e in ol.rand_elts(rng, 2 * logw, field)]))
        _problems[key] = (L, st, logv, logw)
    return _problems[key]


def want_oracle(field, name, b):
    """expectation A, computed once per statement: (evals per round-hand, wc_out, bound_quad, nh0)"""
    key = (field, name, b)
    if key not in _oracle:
        L, st, logv, _ = problem(field, name)
        s = st[b]
        _oracle[key] = oracle_layer(field, dict(L, W=s["W"]), logv, s["G0"], s["G1"], s["alpha"], s["beta"], s["wc_in"], s["chal"])
    return _oracle[key]


def run_single(q, field, name, b):
    """lfgpu_sumcheck_layer on statement b -> (evals, wc_out, bound_quad, g_out)"""
    import gpu_util as G
    L, st, logv, logw = problem(field, name)
    s = st[b]
    dW = G.to_dev(s["W"])
    got = []

    def cb(hand, rnd, ev):
        got.append(tuple((int(e[0]), int(e[1])) for e in ev))
        return s["chal"][len(got) - 1]

    wc, ch, bq = q.sumcheck_layer(logv, s["G0"], s["G1"], s["alpha"], s["beta"], logw, L["nw"], dW.data_ptr(), s["wc_in"], cb)
    return got, [_tup(w) for w in wc], _tup(bq), [[_tup(c) for c in ch[h]] for h in (0, 1)]


def want_single(field, name, b):
    """expectation B, computed once per statement on a quad of its own"""
    import gpu_util as G
    key = (field, name, b)
    if key not in _single:
        L = problem(field, name)[0]
        q = G.pkg.Quad(G.gpu(), field, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], L["nv"])
        _single[key] = run_single(q, field, name, b)
        q.close()
    return _single[key]


def run_batch(q, field, name, B, pad=0, order=None):
    """lfgpu_sumcheck_layer_batch on statements 0..B-1 -> per statement (evals, wc_out, bound_quad, g_out)"""
    import gpu_util as G
    L, st, logv, logw = problem(field, name)
    nw, ldw = L["nw"], L["nw"] + pad
    Wb = np.full((B, ldw, 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)  # the padding after each statement's wires holds a pattern
    for b in range(B):
        Wb[b, :nw] = st[b]["W"]
    dW = G.to_dev(Wb)
    G0 = np.concatenate([st[b]["G0"][:logv] for b in range(B)]) if logv else np.zeros((1, 2), dtype=np.uint64)
    G1 = np.concatenate([st[b]["G1"][:logv] for b in range(B)]) if logv else np.zeros((1, 2), dtype=np.uint64)
    got = [[] for _ in range(B)]
    calls = []

    def cb(hand, rnd, evals):
        calls.append((rnd, hand, len(evals)))
        for b in range(B):
            got[b].append(tuple((int(e[0]), int(e[1])) for e in evals[b]))
        return [st[b]["chal"][len(calls) - 1] for b in range(B)]

    wc, ch, bq = q.sumcheck_layer_batch(logv, G0, G1, [st[b]["alpha"] for b in range(B)], [st[b]["beta"] for b in range(B)], logw, nw,
                                        dW.data_ptr(), ldw, [st[b]["wc_in"] for b in range(B)], cb)
    if order is not None:
        order.extend(calls)
    return [(got[b], [_tup(w) for w in wc[b]], _tup(bq[b]), [[_tup(c) for c in ch[b][h]] for h in (0, 1)]) for b in range(B)]


def check_statement(field, name, b, got, single=True):
    ev, wc, bq, g = got
    logw = SHAPES[name][1]
    st = problem(field, name)[1][b]
    want_ev, want_wc, want_bq, _ = want_oracle(field, name, b)
    assert len(ev) == len(want_ev) == 2 * logw
    for i, (x, y) in enumerate(zip(ev, want_ev)):
        assert x == y, "statement %d, round-hand %d vs the oracle" % (b, i)
    assert wc == want_wc and bq == want_bq, "statement %d vs the oracle" % b
    assert g == [[st["chal"][2 * r + h] for r in range(logw)] for h in (0, 1)]
    if single:
        assert (ev, wc, bq, g) == want_single(field, name, b), "statement %d vs lfgpu_sumcheck_layer" % b


def new_quad(field, name):
    import gpu_util as G
    L = problem(field, name)[0]
    return G.pkg.Quad(G.gpu(), field, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], L["nv"])


@pytest.mark.gpu
@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("case", CASES, ids=["%s-B%d" % c for c in CASES])
def test_batch_equals_oracle_and_single_call(field, case):
    name, B = case
    logw = SHAPES[name][1]
    q = new_quad(field, name)
    order = []
    got = run_batch(q, field, name, B, order=order)
    q.close()
    # one callback per round-hand for ALL statements, in (round, hand) order
    assert order == [(r, h, B) for r in range(logw) for h in (0, 1)]
    if name == "cross":  # it is there for the large kernels: both the HQUAD and the wires start above the fused step's bound
        assert want_oracle(field, name, 0)[3] > SMALL_MAX and problem(field, name)[0]["nw"] > SMALL_MAX
    for b in range(B):
        check_statement(field, name, b, got[b])


@pytest.mark.gpu
@pytest.mark.parametrize("field", [GF, FP])
def test_shared_bind_shape_records_serve_both_entry_points(field):
    """single, batch, single on one quad; batch, single on a fresh one: the batch records the quad's bind shapes through the
    same path as the single call, and every result equals the oracle's"""
    name, B = "cross", 3
    q = new_quad(field, name)
    check_statement(field, name, 1, run_single(q, field, name, 1))
    for b, got in enumerate(run_batch(q, field, name, B)):
        check_statement(field, name, b, got)
    check_statement(field, name, 2, run_single(q, field, name, 2))
    q.close()
    q = new_quad(field, name)
    for b, got in enumerate(run_batch(q, field, name, B)):
        check_statement(field, name, b, got)
    check_statement(field, name, 0, run_single(q, field, name, 0))
    q.close()


@pytest.mark.gpu
@pytest.mark.parametrize("field", [GF, FP])
def test_wire_stride(field):
    """ldw = nw + 3: the three elements after each statement's wires are not part of it"""
    name, B = "cross", 3
    q = new_quad(field, name)
    got = run_batch(q, field, name, B, pad=3)
    q.close()
    for b in range(B):
        check_statement(field, name, b, got[b])


@pytest.mark.gpu
def test_argument_errors_leave_the_context_usable():
    import gpu_util as G
    name, field = "tiny", GF
    L, st, logv, logw = problem(field, name)
    q = new_quad(field, name)
    nw = L["nw"]
    dW = G.to_dev(np.zeros((65, nw, 2), dtype=np.uint64))
    G0 = np.zeros((65 * max(1, logv), 2), dtype=np.uint64)

    def call(B, ldw):
        return q.sumcheck_layer_batch(logv, G0, G0, [(1, 0)] * B, [(1, 0)] * B, logw, nw, dW.data_ptr(), ldw, [[(0, 0), (0, 0)]] * B,
                                      lambda hand, rnd, ev: [(1, 0)] * len(ev))

    for B, ldw in ((0, nw), (65, nw), (3, nw - 1)):
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):  # LFGPU_ERR_ARG
            call(B, ldw)
        for b, got in enumerate(run_batch(q, field, name, 3)):  # a valid call passes afterwards
            check_statement(field, name, b, got, single=False)
    q.close()
    # Fp256Base layers run inside the ZK driver: LFGPU_ERR_UNSUPPORTED, as lfgpu_sumcheck_layer
    kvec = np.zeros((len(L["kvec"]), 4), dtype=np.uint64)
    kvec[:, 0] = np.arange(len(kvec))
    q = G.pkg.Quad(G.gpu(), G.pkg.FIELD_P256, L["g"], L["h0"], L["h1"], L["vi"], kvec, L["nv"])
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 3:"):
        call(3, nw)
    q.close()

"""lfgpu_sumcheck_layer_batch256: B statements of one Fp256Base quad in lock-step.  Statement b of the batch must be
byte-identical to (A) the Python-integer model of ProverLayers::layer (tests/p256_layer_model.py, pinned to the oracle by
tests/test_p256_layer_model.py) for statement b -- evaluations of every round-hand, wc_out, bound_quad -- and (B)
lfgpu_sumcheck_layer256 on the GPU for statement b alone with the same challenges (the same, plus g_out).  Every statement
has its own W, G0, G1, alpha, beta, wc_in and challenges from a seeded generator; all share one layer.

Shapes (logv, logw, terms, nv, nw):
  one    0, 1, 1, 1, 2                    a single term, no output variable
  tiny   2, 3, 8, 3, 5                    a single wave, odd at every halving
  small  5, 6, 300                        the fused step from the first round-hand, up to the cap of 64 statements
  cross  12, 14, 40000, 2049, 2^13 + 1    starts on the three launches -- nh0 and nw above the hand-off bound --, crosses to
                                          the fused step within the layer, odd sizes throughout"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import p256_layer_model as M
from oracle_lib import FP, GF
from test_sumcheck_layer_random import make_layer_vec

P256 = 1  # LFGPU_FIELD_P256
SHAPES = {
    "one": (0, 1, 1, 1, 2),
    "tiny": (2, 3, 8, 3, 5),
    "small": (5, 6, 300),
    "cross": (12, 14, 40000, 2049, (1 << 13) + 1),
}
CASES = [("one", 1), ("one", 3), ("tiny", 1), ("tiny", 3), ("tiny", 16), ("small", 16), ("small", 64), ("cross", 3)]
MAX_B = {"one": 3, "tiny": 16, "small": 64, "cross": 3}
PAD_WORD = 0xA5A5A5A5A5A5A5A5

_problems, _model, _single = {}, {}, {}


def _tup(e):
    return tuple(int(x) for x in e)


def problem(name):
    """the layer and MAX_B statements over it; statement b is the same whatever the batch size"""
    if name not in _problems:
        logv, logw, nterms, *shape = SHAPES[name]
        rng = np.random.default_rng(256000 + 1000 * logw + logv)
        L = make_layer_vec(rng, FP, logv, logw, nterms, *([9] + shape if shape else []))  # the structure; the elements follow
        L["kvec"] = M.rand_images(rng, 9)
        L["kvec"][0] = 0
        del L["W"]
        st = []
        for _ in range(MAX_B[name]):
            st.append(dict(W=M.rand_images(rng, L["nw"]), G0=M.rand_images(rng, max(1, logv)), G1=M.rand_images(rng, max(1, logv)),
                           alpha=_tup(M.rand_images(rng, 1)[0]), beta=_tup(M.rand_images(rng, 1)[0]),
                           wc_in=[_tup(e) for e in M.rand_images(rng, 2)], chal=[_tup(e) for e in M.rand_images(rng, 2 * logw)]))
        _problems[name] = (L, st, logv, logw)
    return _problems[name]


def want_model(name, b):
    """expectation A, computed once per statement: (evals per round-hand, wc_out, bound_quad, nh0)"""
    if (name, b) not in _model:
        L, st, logv, _ = problem(name)
        s = st[b]
        _model[(name, b)] = M.layer(M.P256, L, L["kvec"], s["W"], logv, s["G0"], s["G1"], s["alpha"], s["beta"], s["wc_in"], s["chal"])
    return _model[(name, b)]


def run_single(q, name, b):
    """lfgpu_sumcheck_layer256 on statement b -> (evals, wc_out, bound_quad, g_out); the wires must come back unchanged"""
    import gpu_util as G
    L, st, logv, logw = problem(name)
    s = st[b]
    dW = G.to_dev(s["W"])
    got = []

    def cb(hand, rnd, ev):
        got.append(tuple(_tup(e) for e in ev))
        return s["chal"][len(got) - 1]

    wc, ch, bq = q.sumcheck_layer256(logv, s["G0"], s["G1"], s["alpha"], s["beta"], logw, L["nw"], dW.data_ptr(), s["wc_in"], cb)
    assert (G.from_dev(dW, np.uint64, s["W"].shape) == s["W"]).all(), "lfgpu_sumcheck_layer256 modified d_W"
    return got, [_tup(w) for w in wc], _tup(bq), [[_tup(c) for c in ch[h]] for h in (0, 1)]


def want_single(name, b):
    """expectation B, computed once per statement on a quad of its own"""
    if (name, b) not in _single:
        q = new_quad(name)
        _single[(name, b)] = run_single(q, name, b)
        q.close()
    return _single[(name, b)]


def run_batch(q, name, B, pad=0, order=None):
    """lfgpu_sumcheck_layer_batch256 on statements 0..B-1 -> per statement (evals, wc_out, bound_quad, g_out)"""
    import gpu_util as G
    L, st, logv, logw = problem(name)
    nw, ldw = L["nw"], L["nw"] + pad
    Wb = np.full((B, ldw, 4), PAD_WORD, dtype=np.uint64)  # the padding after each statement's wires holds a pattern
    for b in range(B):
        Wb[b, :nw] = st[b]["W"]
    dW = G.to_dev(Wb)
    G0 = np.concatenate([st[b]["G0"][:logv] for b in range(B)]) if logv else np.zeros((1, 4), dtype=np.uint64)
    G1 = np.concatenate([st[b]["G1"][:logv] for b in range(B)]) if logv else np.zeros((1, 4), dtype=np.uint64)
    got = [[] for _ in range(B)]
    calls = []

    def cb(hand, rnd, evals):
        calls.append((rnd, hand, len(evals)))
        for b in range(B):
            got[b].append(tuple(_tup(e) for e in evals[b]))
        return [st[b]["chal"][len(calls) - 1] for b in range(B)]

    wc, ch, bq = q.sumcheck_layer_batch256(logv, G0, G1, [st[b]["alpha"] for b in range(B)], [st[b]["beta"] for b in range(B)], logw, nw,
                                           dW.data_ptr(), ldw, [st[b]["wc_in"] for b in range(B)], cb)
    assert (G.from_dev(dW, np.uint64, Wb.shape) == Wb).all(), "d_W (or its padding) was modified"
    if order is not None:
        order.extend(calls)
    return [(got[b], [_tup(w) for w in wc[b]], _tup(bq[b]), [[_tup(c) for c in ch[b][h]] for h in (0, 1)]) for b in range(B)]


def check_statement(name, b, got, single=True):
    ev, wc, bq, g = got
    logw = SHAPES[name][1]
    st = problem(name)[1][b]
    want_ev, want_wc, want_bq, _ = want_model(name, b)
    assert len(ev) == len(want_ev) == 2 * logw
    for i, (x, y) in enumerate(zip(ev, want_ev)):
        assert x == y, "statement %d, round-hand %d vs the model" % (b, i)
    assert wc == want_wc and bq == want_bq, "statement %d vs the model" % b
    assert g == [[st["chal"][2 * r + h] for r in range(logw)] for h in (0, 1)]
    if single:
        assert (ev, wc, bq, g) == want_single(name, b), "statement %d vs lfgpu_sumcheck_layer256" % b


def new_quad(name, field=P256):
    import gpu_util as G
    L = problem(name)[0]
    kvec = L["kvec"] if field == P256 else L["kvec"][:, :2].copy()
    return G.pkg.Quad(G.gpu(), field, L["g"], L["h0"], L["h1"], L["vi"], kvec, L["nv"])


def results_digest(cases):
    """SHA-256 over every statement's results of the given (name, B) cases, for the A/B comparison across processes"""
    h = hashlib.sha256()
    for name, B in cases:
        q = new_quad(name)
        for got in run_batch(q, name, B):
            h.update(repr(got).encode())
        q.close()
    return h.hexdigest()


AB_CASES = [("tiny", 3), ("small", 16), ("cross", 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["%s-B%d" % c for c in CASES])
def test_batch_equals_model_and_single_call(case):
    import gpu_util as G
    name, B = case
    logw = SHAPES[name][1]
    q = new_quad(name)
    order = []
    got = run_batch(q, name, B, order=order)
    q.close()
    # one callback per round-hand for ALL statements, in (round, hand) order
    assert order == [(r, h, B) for r in range(logw) for h in (0, 1)]
    if name == "cross":  # it is there for the three launches: both the HQUAD and the wires start above the fused step's bound
        assert want_model(name, 0)[3] > G.pkg.P256_BATCH_SMALL_MAX and problem(name)[0]["nw"] > G.pkg.P256_BATCH_SMALL_MAX
    for b in range(B):
        check_statement(name, b, got[b])


@pytest.mark.gpu
def test_shared_bind_shape_records_serve_both_entry_points():
    """single, batch, single on one quad; batch, single on a fresh one: the batch records the quad's bind shapes through the
    same path as the single call, and every result equals the model's"""
    name, B = "cross", 3
    q = new_quad(name)
    check_statement(name, 1, run_single(q, name, 1))
    for b, got in enumerate(run_batch(q, name, B)):
        check_statement(name, b, got)
    check_statement(name, 2, run_single(q, name, 2))
    q.close()
    q = new_quad(name)
    for b, got in enumerate(run_batch(q, name, B)):
        check_statement(name, b, got)
    check_statement(name, 0, run_single(q, name, 0))
    q.close()


@pytest.mark.gpu
def test_wire_stride():
    """ldw = nw + 3: the three elements after each statement's wires are not part of it (and stay as they were)"""
    name, B = "cross", 3
    q = new_quad(name)
    got = run_batch(q, name, B, pad=3)
    q.close()
    for b in range(B):
        check_statement(name, b, got[b])


@pytest.mark.gpu
def test_argument_errors_leave_the_context_usable():
    import gpu_util as G
    name = "tiny"
    L, st, logv, logw = problem(name)
    nw = L["nw"]
    dW = G.to_dev(np.zeros((65, nw, 4), dtype=np.uint64))
    G0 = np.zeros((65 * max(1, logv), 4), dtype=np.uint64)
    one = (1, 0, 0, 0)

    def call(q, B, ldw):
        return q.sumcheck_layer_batch256(logv, G0, G0, [one] * B, [one] * B, logw, nw, dW.data_ptr(), ldw, [[one, one]] * B,
                                         lambda hand, rnd, ev: [one] * len(ev))

    q = new_quad(name)
    qgf = new_quad(name, GF)  # a quad of a 16-byte field
    for bad, B, ldw in ((q, 0, nw), (q, 65, nw), (q, 3, nw - 1), (qgf, 3, nw)):
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):  # LFGPU_ERR_ARG
            call(bad, B, ldw)
        for b, got in enumerate(run_batch(q, name, 3)):  # a valid call passes afterwards
            check_statement(name, b, got, single=False)
    qgf.close()
    q.close()


@pytest.mark.gpu
def test_three_launches_throughout_give_the_same_bytes():
    """LFGPU_P256_BATCH_SMALL=0 (read once per process, so in a fresh child): the A/B switch must not change a byte"""
    env = dict(os.environ, LFGPU_P256_BATCH_SMALL="0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=env,
                         cwd=os.path.dirname(os.path.abspath(__file__)))
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "digest " + results_digest(AB_CASES)


if __name__ == "__main__":  # the child of the A/B test
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("digest " + results_digest(AB_CASES))

"""The sumcheck over nc copies of a circuit on the GPU (lfgpu_eval_quad_copies, lfgpu_sumcheck_evaluations_c,
lfgpu_dense_bind_rows, lfgpu_eqs, lfgpu_sumcheck_layer_copies) byte for byte against tests/copies_model.py, which
tests/test_sumcheck_copies_model.py pins without a GPU."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import copies_chain as cc
import copies_model as cm
import oracle_lib as ol
import quad_util as qu
from oracle_lib import FP, GF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _img(rng, field):
    return tuple(int(x) for x in ol.rand_elts(rng, 1, field)[0])


def _pm1(field):
    x = cm.FP_P - 1
    return (2**64 - 1, 2**64 - 1) if field == GF else (x & (2**64 - 1), x >> 64)


# ---------------------------------------------------------------- eval_quad over copies
@functools.lru_cache(maxsize=None)
def _eval_layer(field):
    rng = np.random.default_rng(300 + field)
    L = qu.make_layer(rng, field, 4, 5, 120, n_assert=6)  # six assert-zero terms on wires that are zero in L["W"]
    return L, cm.ModelField(field)


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("nc", [1, 2, 3, 64, 130])
def test_eval_quad_copies(field, nc):
    import gpu_util as G
    L, F = _eval_layer(field)
    rng = np.random.default_rng(nc)
    nw, az = L["nw"], L["vi"] == 0
    W = ol.rand_elts(rng, nw * nc, field).reshape(nw, nc, 2)
    W[:, 0] = L["W"]  # copy 0: the layer's own assignment; the others random ...
    for h in set(L["h0"][az].tolist()):
        W[h, :] = 0  # ... with one factor of every assert-zero term zero in ALL copies
    W = np.ascontiguousarray(W.reshape(nw * nc, 2))
    q = G.pkg.Quad(G.gpu(), field, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], L["nv"])
    dW, dV = G.to_dev(W), G.to_dev(np.zeros((L["nv"] * nc, 2), dtype=np.uint64))
    ok, V = cm.eval_quad_copies(F, L, nc, W)
    assert ok and q.eval_copies(nc, nw, dW.data_ptr(), dV.data_ptr())
    assert (G.from_dev(dV, np.uint64, (L["nv"] * nc, 2)) == V).all()
    # violated in exactly one copy (the last): both factors of one assert-zero term non-zero there
    t = int(np.flatnonzero(az)[0])
    W[int(L["h0"][t]) * nc + nc - 1] = (1, 0)
    W[int(L["h1"][t]) * nc + nc - 1] = (1, 0)
    assert not cm.eval_quad_copies(F, L, nc, W)[0]
    assert not q.eval_copies(nc, nw, G.to_dev(W).data_ptr(), dV.data_ptr())
    q.close()


# ---------------------------------------------------------------- Dense::bind over rows, Eqs
@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("n0,nrows", [(1, 5), (2, 1), (3, 7), (129, 33), (1024, 4)])
def test_dense_bind_rows(field, n0, nrows):
    import gpu_util as G
    F = cm.ModelField(field)
    rng = np.random.default_rng(n0 + nrows + field)
    A = ol.rand_elts(rng, n0 * nrows, field)
    A[::5] = 0
    A[2::9] = _pm1(field)
    r = _img(rng, field)
    Ai = F.of_array(A)
    want = F.array([x for i in range(nrows) for x in cm.bind_row(F, Ai[i * n0:(i + 1) * n0], F.of_img(r))])
    nout = (n0 + 1) // 2
    dA, dB = G.to_dev(A), G.to_dev(np.zeros((nout * nrows, 2), dtype=np.uint64))
    assert G.gpu().dense_bind_rows(field, n0, nrows, r, dA.data_ptr(), dB.data_ptr()) == nout
    assert (G.from_dev(dB, np.uint64, (nout * nrows, 2)) == want).all()
    assert (G.from_dev(dA, np.uint64, (n0 * nrows, 2)) == A).all()  # out of place: the input is left alone
    # overlapping buffers (in place, and an output that starts inside the input) are refused
    L, h = G.gpu().L, G.gpu().h
    rr = (C.c_uint64 * 2)(*r)
    for off in (0, 16 * (n0 * nrows - 1)):
        assert L.lfgpu_dense_bind_rows(h, field, n0, nrows, rr, C.c_void_p(dA.data_ptr()), C.c_void_p(dA.data_ptr() + off)) == 1


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("logn,n", [(0, 1), (1, 1), (1, 2), (3, 5), (7, 65), (8, 256), (11, 1025)])
def test_eqs(field, logn, n):
    import gpu_util as G
    F = cm.ModelField(field)
    rng = np.random.default_rng(logn + n + field)
    Q = ol.rand_elts(rng, max(1, logn), field)
    dE = G.to_dev(np.zeros((n, 2), dtype=np.uint64))
    G.gpu().eqs(field, logn, n, Q, dE.data_ptr())
    assert (G.from_dev(dE, np.uint64, (n, 2)) == F.array(cm.filleq(F, logn, n, F.of_array(Q)))).all()


# ---------------------------------------------------------------- K13: the accumulators of evaluations_c
NROWS = 6  # few wires: the model folds over c once per distinct hand pair


def _evc_case(field, n0, nh):
    rng = np.random.default_rng(1000 * n0 + nh + field)
    W = ol.rand_elts(rng, NROWS * n0, field)
    W[::13] = 0
    W[5::17] = _pm1(field)
    EQ = ol.rand_elts(rng, n0, field)
    EQ[0] = _pm1(field)
    if n0 > 2:
        EQ[n0 - 1] = 0
    hc = rng.integers(0, NROWS, size=(nh, 2), dtype=np.uint32)
    hc[0] = (2, 2)  # h0 == h1
    vc = ol.rand_elts(rng, nh, field)
    return W, EQ, np.ascontiguousarray(hc), vc


EVC_SHAPES = [(n0, 257) for n0 in (1, 2, 3, 63, 64, 65, 130, 1025)] + [(n0, nh) for n0 in (3, 130) for nh in (1, 3, 5000)]


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("n0,nh", EVC_SHAPES)
def test_evaluations_c(field, n0, nh):
    """n0: the odd tail alone, one pair, pair + tail, fewer pairs than a wave, one pair past a wave (130: 65 pairs, EQ through
    LDS), more pairs than the LDS copy of EQ holds (1025: EQ from memory, nine passes of the lanes); nh: one term, sub-wave,
    across a workgroup, several workgroups with the final reduction.  W and EQ hold 0 and p - 1, term 0 has h0 == h1."""
    import gpu_util as G
    F = cm.ModelField(field)
    W, EQ, hc, vc = _evc_case(field, n0, nh)
    Wi = F.of_array(W)
    rows = [Wi[w * n0:(w + 1) * n0] for w in range(NROWS)]
    want = [F.img(x) for x in cm.accumulators_c(F, F.of_array(EQ), rows, [tuple(x) for x in hc.tolist()], F.of_array(vc))]
    dW, dE, dh, dv = G.to_dev(W), G.to_dev(EQ), G.to_dev(hc), G.to_dev(vc)
    got = G.gpu().sumcheck_evaluations_c(field, nh, dh.data_ptr(), dv.data_ptr(), n0, NROWS, dW.data_ptr(), dE.data_ptr())
    assert [tuple(int(x) for x in g) for g in got] == want


# ---------------------------------------------------------------- whole layers: a three-layer chain
@functools.lru_cache(maxsize=None)
def _chain_model(field, nc, logc=None):
    return cc.run_model(cc.make_chain(field, nc, logc))


CHAIN_NC = [2, 5, 64]
# nc <= 2^(logc - 1): one copy is left before the last copy round, so the later rounds (for nc = 1, all of them) are the odd tail alone
CHAIN_TAIL_ONLY = [(1, 1), (2, 3), (3, 4)]


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("nc", CHAIN_NC)
def test_layer_chain_matches_model(field, nc):
    """every callback value, wc_out, q_out, g_out and bound_quad of three chained layers (logw 6, 11, 1)"""
    import gpu_util as G
    got = cc.run_gpu(cc.make_chain(field, nc), G.pkg, G.gpu(), G.to_dev)
    want = _chain_model(field, nc)
    for k, (a, b) in enumerate(zip(got, want)):
        for key in b:
            assert a[key] == b[key], "layer %d %s" % (k, key)


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("nc,logc", CHAIN_TAIL_ONLY)
def test_layer_chain_tail_only_rounds(field, nc, logc):
    """more copy rounds than the copies need: EQ and every row of W are down to one entry while copy rounds remain"""
    import gpu_util as G
    got = cc.run_gpu(cc.make_chain(field, nc, logc), G.pkg, G.gpu(), G.to_dev)
    want = _chain_model(field, nc, logc)
    for k, (a, b) in enumerate(zip(got, want)):
        for key in b:
            assert a[key] == b[key], "layer %d %s" % (k, key)


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("mode", ["off", "launch", "resident"])
def test_layer_chain_under_sc_mode(field, mode):
    """the same bytes with the hand rounds on the per-launch kernels throughout / one fused launch per round-hand / the single
    resident workgroup, which takes over on the W the copy rounds left (the switch is read once per process: a child process
    per mode and field, all copy counts in it, and one tail-only shape)"""
    e = {k: v for k, v in os.environ.items() if not k.startswith(("LFGPU_SC_", "LFGPU_CU_", "LFGPU_EQ_"))}
    e["LFGPU_SC_MODE"] = mode
    cases = [(n, None) for n in CHAIN_NC] + [CHAIN_TAIL_ONLY[1]]
    args = [str(n) if lc is None else "%d:%d" % (n, lc) for n, lc in cases]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "copies_child.py"), str(field)] + args, env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESULT " in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(r.stdout[r.stdout.index("RESULT ") + 7:])
    for a, (nc, logc) in zip(args, cases):
        assert got[a] == _chain_model(field, nc, logc), "nc = %d, logc = %s" % (nc, logc)


# ---------------------------------------------------------------- one copy: the existing entry point
@pytest.mark.parametrize("field", [GF, FP])
def test_one_copy_is_sumcheck_layer(field):
    import gpu_util as G
    rng = np.random.default_rng(77 + field)
    logv, logw = 5, 9
    L = qu.make_layer(rng, field, logv, logw, 1500)
    G0, G1 = ol.rand_elts(rng, logv, field), ol.rand_elts(rng, logv, field)
    alpha, beta, wc_in = _img(rng, field), _img(rng, field), [_img(rng, field), _img(rng, field)]
    chal = [_img(rng, field) for _ in range(2 * logw)]
    q = G.pkg.Quad(G.gpu(), field, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], L["nv"])
    res = []
    for copies in (False, True):
        evs = []

        def round_h(hand, rnd, ev):
            evs.append([tuple(int(x) for x in e) for e in ev])
            return chal[2 * rnd + hand]

        dW = G.to_dev(L["W"])
        if copies:
            wc, qo, ch, bq = q.sumcheck_layer_copies(0, 1, np.zeros((0, 2), dtype=np.uint64), logv, G0, G1, alpha, beta, logw, L["nw"],
                                                     dW.data_ptr(), wc_in, None, round_h)
            assert qo == []
        else:
            wc, ch, bq = q.sumcheck_layer(logv, G0, G1, alpha, beta, logw, L["nw"], dW.data_ptr(), wc_in, round_h)
        res.append((evs, [tuple(w) for w in wc], ch, tuple(bq)))
    q.close()
    assert len(res[0][0]) == 2 * logw and res[0] == res[1]


# ---------------------------------------------------------------- the flatsha-1 circuit with its witness in four copies
def test_flatsha_replicated_witness():
    import gpu_util as G
    import sumcheck_driver as sd
    circ, W, _, _ = sd.load_fixture(GOLD, 1)
    nc, F = 4, cm.ModelField(GF)
    sc = sd.GpuSumcheck(G.pkg, G.gpu(), circ)
    ins1, V1 = sc.eval_circuit(W)
    assert ins1 is not None and (V1 == 0).all()
    nl = circ["nl"]
    ins = [None] * nl
    ins[nl - 1] = G.to_dev(np.repeat(W, nc, axis=0))  # W[wire * nc + c]: the same witness in every copy
    cur = ins[nl - 1]
    for l in range(nl - 1, -1, -1):
        nout = circ["layers"][l - 1]["nw"] if l > 0 else circ["nv"]
        V = G.to_dev(np.zeros((nout * nc, 2), dtype=np.uint64))
        assert sc.quads[l].eval_copies(nc, circ["layers"][l]["nw"], cur.data_ptr(), V.data_ptr())
        one = G.from_dev(ins1[l - 1], np.uint64, (nout, 2)) if l > 0 else V1
        assert (G.from_dev(V, np.uint64, (nout, nc, 2)) == one[:, None, :]).all(), "layer %d" % l
        if l > 0:
            ins[l - 1] = V
        cur = V
    # layer 0 proved over the copies
    lay = circ["layers"][0]
    L = dict(lay, kvec=circ["kvec"], n=len(lay["g"]), nv=circ["nv"])
    rng = np.random.default_rng(4)
    logc, logv = 2, circ["logv"]
    Q, G0, G1 = ol.rand_elts(rng, logc, GF), ol.rand_elts(rng, logv, GF), ol.rand_elts(rng, logv, GF)
    alpha, beta = _img(rng, GF), _img(rng, GF)
    chc, chh = [_img(rng, GF) for _ in range(logc)], [_img(rng, GF) for _ in range(2 * lay["logw"])]
    W0 = G.from_dev(ins[0], np.uint64, (lay["nw"] * nc, 2)).copy()
    both = []
    for gpu_run in (False, True):
        evs = []

        def rc(rnd, ev):
            evs.append([tuple(int(x) for x in e) for e in ev])
            return chc[rnd]

        def rh(hand, rnd, ev):
            evs.append([tuple(int(x) for x in e) for e in ev])
            return chh[2 * rnd + hand]

        if gpu_run:
            wc, qo, g, bq = sc.quads[0].sumcheck_layer_copies(logc, nc, Q, logv, G0, G1, alpha, beta, lay["logw"], lay["nw"],
                                                              G.to_dev(W0).data_ptr(), [(0, 0), (0, 0)], rc, rh)
        else:
            res = cm.layer(F, L, logc, nc, [tuple(int(x) for x in e) for e in Q], logv, G0, G1, alpha, beta, W0, [(0, 0), (0, 0)], rc, rh)
            wc, qo, g, bq = res["wc"], res["q"], res["g"], res["bound_quad"]
        both.append((evs, [tuple(w) for w in wc], [tuple(x) for x in qo], [[tuple(x) for x in gh] for gh in g], tuple(bq)))
    sc.close()
    assert both[0] == both[1]


# ---------------------------------------------------------------- error paths: a status, never an abort
def test_error_paths_return_err_arg():
    import gpu_util as G
    gpu = G.gpu()
    Lb, h = gpu.L, gpu.h
    rng = np.random.default_rng(1)
    L = qu.make_layer(rng, GF, 3, 4, 40)
    q = G.pkg.Quad(gpu, GF, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], L["nv"])
    nc = 2
    dW = G.to_dev(ol.rand_elts(rng, L["nw"] * nc, GF))
    dV = G.to_dev(np.zeros((L["nv"] * nc, 2), dtype=np.uint64))
    ok = C.c_int()
    vp, NULL = C.c_void_p, None
    ERR_ARG, UNSUPPORTED = 1, 3
    assert Lb.lfgpu_eval_quad_copies(NULL, nc, L["nw"], vp(dW.data_ptr()), vp(dV.data_ptr()), C.byref(ok)) == ERR_ARG
    assert Lb.lfgpu_eval_quad_copies(q.h, nc, L["nw"], NULL, vp(dV.data_ptr()), C.byref(ok)) == ERR_ARG
    assert Lb.lfgpu_eval_quad_copies(q.h, 0, L["nw"], vp(dW.data_ptr()), vp(dV.data_ptr()), C.byref(ok)) == ERR_ARG
    assert Lb.lfgpu_eval_quad_copies(q.h, nc, 1, vp(dW.data_ptr()), vp(dV.data_ptr()), C.byref(ok)) == ERR_ARG  # nw <= a hand index
    acc = (C.c_uint64 * 6)()
    r = (C.c_uint64 * 2)(1, 0)
    assert Lb.lfgpu_sumcheck_evaluations_c(h, GF, 4, NULL, NULL, 2, 4, vp(dW.data_ptr()), vp(dW.data_ptr()), acc) == ERR_ARG
    assert Lb.lfgpu_sumcheck_evaluations_c(h, GF, 4, vp(dW.data_ptr()), vp(dW.data_ptr()), 0, 4, vp(dW.data_ptr()), vp(dW.data_ptr()), acc) == ERR_ARG
    assert Lb.lfgpu_sumcheck_evaluations_c(h, 1, 4, vp(dW.data_ptr()), vp(dW.data_ptr()), 2, 4, vp(dW.data_ptr()), vp(dW.data_ptr()), acc) == UNSUPPORTED
    assert Lb.lfgpu_dense_bind_rows(h, GF, 2, 2, NULL, vp(dW.data_ptr()), vp(dV.data_ptr())) == ERR_ARG
    assert Lb.lfgpu_dense_bind_rows(h, GF, 2, 2, r, NULL, vp(dV.data_ptr())) == ERR_ARG
    assert Lb.lfgpu_dense_bind_rows(h, 1, 2, 2, r, vp(dW.data_ptr()), vp(dV.data_ptr())) == UNSUPPORTED
    assert Lb.lfgpu_eqs(h, GF, 2, 0, vp(dW.data_ptr()), vp(dV.data_ptr())) == ERR_ARG
    assert Lb.lfgpu_eqs(h, GF, 2, 5, vp(dW.data_ptr()), vp(dV.data_ptr())) == ERR_ARG  # n > 2^logn
    assert Lb.lfgpu_eqs(h, GF, 2, 4, NULL, vp(dV.data_ptr())) == ERR_ARG
    # the layer: null pointers, nc == 0, nc > 2^logc, logc > 40
    Qh = ol.rand_elts(rng, 41, GF)
    G0 = ol.rand_elts(rng, 3, GF)
    al = (C.c_uint64 * 2)(5, 0)
    wci, wco, qo, go, bq = (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * 82)(), (C.c_uint64 * 16)(), (C.c_uint64 * 2)()
    calls = []
    cfc = G.pkg.SC_ROUND_C_FN(lambda *a: calls.append(a))
    cfh = G.pkg.SC_ROUND_FN(lambda *a: calls.append(a))
    nullc, nullh = C.cast(None, G.pkg.SC_ROUND_C_FN), C.cast(None, G.pkg.SC_ROUND_FN)

    def layer(qh=q.h, logc=1, nc_=nc, Qp=vp(Qh.ctypes.data), dWp=vp(dW.data_ptr()), rc=cfc, rh=cfh, qop=qo):
        return Lb.lfgpu_sumcheck_layer_copies(qh, logc, nc_, Qp, 3, vp(G0.ctypes.data), vp(G0.ctypes.data), al, al, 4, L["nw"], dWp, wci, rc, rh,
                                              NULL, wco, qop, go, bq)

    assert layer(qh=NULL) == ERR_ARG
    assert layer(nc_=0) == ERR_ARG
    assert layer(nc_=3) == ERR_ARG  # nc > 2^logc
    assert layer(logc=0, nc_=2) == ERR_ARG
    assert layer(logc=41, nc_=2) == ERR_ARG
    assert layer(Qp=NULL) == ERR_ARG
    assert layer(dWp=NULL) == ERR_ARG
    assert layer(rc=nullc) == ERR_ARG
    assert layer(rh=nullh) == ERR_ARG
    assert layer(qop=NULL) == ERR_ARG
    assert calls == []
    q.close()

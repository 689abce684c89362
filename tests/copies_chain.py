"""A three-layer synthetic chain proved with nc copies, once by the model (copies_model.layer) and once on the GPU
(Quad.sumcheck_layer_copies), with the same predetermined challenges: q_out of one layer is Q of the next, g_out its G0 / G1,
wc_out its claims.  Shared by tests/test_sumcheck_copies_gpu.py and its child process tests/copies_child.py."""
import numpy as np

import copies_model as cm
import oracle_lib as ol
import quad_util as qu

# (logv, logw) from the output layer down: logw 6, 11 and 1; up to NTERMS terms a layer
SHAPES = [(4, 6), (6, 11), (11, 1)]
NTERMS = 2000


def _img(rng, field):
    return tuple(int(x) for x in ol.rand_elts(rng, 1, field)[0])


def make_chain(field, nc, logc=None):
    """logc: the number of copy rounds, nc <= 2^logc (None: the smallest that holds nc, at least 1; more than that leaves one
    copy before the last copy round, and the rest of them bind the odd tail alone)
    -> dict(layers, W (per layer, [nw * nc, 2] images), logc, Q, G0, G1, wc, alpha/beta per layer, chal_c / chal_h per layer)"""
    logc = max(1, (nc - 1).bit_length()) if logc is None else logc
    assert nc <= 1 << logc
    rng = np.random.default_rng(7000 + 10 * nc + field + 1000 * logc)
    layers, Ws, ab, cc, chh = [], [], [], [], []
    for logv, logw in SHAPES:
        L = qu.make_layer(rng, field, logv, logw, min(NTERMS, 3 << logv) if logw == 1 else NTERMS)
        W = ol.rand_elts(rng, L["nw"] * nc, field)
        W[::7] = 0  # edge values among the wires: zero and p - 1 (all ones for GF(2^128))
        pm1 = cm.FP_P - 1
        W[3::11] = (2**64 - 1, 2**64 - 1) if field == ol.GF else (pm1 & (2**64 - 1), pm1 >> 64)
        layers.append(L)
        Ws.append(W)
        ab.append((_img(rng, field), _img(rng, field)))
        cc.append([_img(rng, field) for _ in range(logc)])
        chh.append([_img(rng, field) for _ in range(2 * logw)])
    logv = SHAPES[0][0]
    return dict(layers=layers, W=Ws, logc=logc, nc=nc, field=field, Q=[_img(rng, field) for _ in range(logc)],
                G0=ol.rand_elts(rng, logv, field), G1=ol.rand_elts(rng, logv, field), wc=[_img(rng, field), _img(rng, field)], ab=ab,
                chal_c=cc, chal_h=chh)


def _canon(x):
    """nested tuples / lists of ints -> nested lists (what survives a JSON round trip)"""
    if isinstance(x, dict):
        return {k: _canon(x[k]) for k in sorted(x)}
    if isinstance(x, (list, tuple)):
        return [_canon(y) for y in x]
    return int(x)


def run(ch, layer_fn):
    """layer_fn(k, L, Q, logv, G0, G1, alpha, beta, W, wc, round_c, round_h) -> (wc, q, g, bound_quad); -> per layer every value
    the prover hands out: the evaluations of every callback in order, wc_out, q_out, g_out, bound_quad"""
    Q, G0, G1, wc, logv = ch["Q"], ch["G0"], ch["G1"], ch["wc"], SHAPES[0][0]
    out = []
    for k, L in enumerate(ch["layers"]):
        evc, evh, order = [], [], []

        def round_c(rnd, ev):
            evc.append(_canon(ev))
            order.append(("c", rnd))
            return ch["chal_c"][k][rnd]

        def round_h(hand, rnd, ev):
            evh.append(_canon(ev))
            order.append((hand, rnd))
            return ch["chal_h"][k][2 * rnd + hand]

        alpha, beta = ch["ab"][k]
        wc, q, g, bq = layer_fn(k, L, Q, logv, G0, G1, alpha, beta, ch["W"][k], wc, round_c, round_h)
        assert order == [("c", r) for r in range(ch["logc"])] + [(h, r) for r in range(L["logw"]) for h in (0, 1)]
        out.append(_canon(dict(evals_c=evc, evals_h=evh, wc=wc, q=q, g=g, bound_quad=bq)))
        Q = q
        G0 = np.array(g[0], dtype=np.uint64).reshape(-1, 2)
        G1 = np.array(g[1], dtype=np.uint64).reshape(-1, 2)
        logv = L["logw"]
    return out


def run_model(ch):
    F = cm.ModelField(ch["field"])

    def layer_fn(k, L, Q, logv, G0, G1, alpha, beta, W, wc, round_c, round_h):
        res = cm.layer(F, L, ch["logc"], ch["nc"], Q, logv, G0, G1, alpha, beta, W, wc, round_c, round_h)
        return res["wc"], res["q"], res["g"], res["bound_quad"]

    return run(ch, layer_fn)


def run_gpu(ch, pkg, gpu, to_dev):
    def layer_fn(k, L, Q, logv, G0, G1, alpha, beta, W, wc, round_c, round_h):
        q = pkg.Quad(gpu, ch["field"], L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], L["nv"])
        dW = to_dev(W)
        try:
            return q.sumcheck_layer_copies(ch["logc"], ch["nc"], np.array(Q, dtype=np.uint64), logv, G0, G1, alpha, beta, L["logw"], L["nw"],
                                           dW.data_ptr(), wc, round_c, round_h)
        finally:
            q.close()

    return run(ch, layer_fn)

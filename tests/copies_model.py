"""Model of the sumcheck prover over nc copies of a circuit, written from the definitions in Python integers: the expected
values of tests/test_sumcheck_copies_*.py.

What it restates (paths in the reference): ProverLayers::layer with its copy rounds and evaluations_c
(lib/sumcheck/prover_layers.h:196-271,415-496), ProverLayers::eval_quad over copies (:278-305), Dense::bind with n1 > 1
(lib/arrays/dense.h:70-87), Eqs::filleq (lib/arrays/eqs.h:104-134), Poly<4> (lib/algebra/poly.h).

Arithmetic.  Fp128: canonical integers mod p = 2^128 - 2^108 + 1; the 16-byte Montgomery images (R = 2^128) are converted
at the edges.  GF(2^128): polynomials over GF(2) mod x^128 + x^7 + x^2 + x + 1 as Python integers with the coefficients
8 bits apart, so that ONE integer product is the carry-less product (a coefficient of the product counts at most 128
overlaps < 2^8; its low bit is the GF(2) sum); packed to the 128-bit image at the edges.

The hand rounds stay on the oracle's array functions (bind_g, QW scatter, partial sums, binds), as OracleSumcheck in
sumcheck_driver.py keeps them; the copy rounds, the round polynomials and every scalar are the model's own.
"""
import ctypes as C

import numpy as np

import oracle_lib as ol
from oracle_lib import FP, GF, P, elt

FP_P = 2**128 - 2**108 + 1
_R = 1 << 128
_RINV = pow(_R, -1, FP_P)
_M128 = int.from_bytes(b"\x01" * 128, "big")  # 128 coefficient slots
_M255 = int.from_bytes(b"\x01" * 255, "big")
_LOW = (1 << 1024) - 1


class ModelField:
    """internal values: Fp128 -> int in [0, p); GF(2^128) -> spread polynomial (bit 8i = coefficient of x^i)"""

    def __init__(self, fid):
        assert fid in (GF, FP)
        self.fid = fid
        self.zero, self.one = 0, 1
        if fid == FP:
            self.pts = [0, 1, 2, 3]  # poly_evaluation_point (lib/algebra/fp_generic.h:114-121)
        else:  # 0, 1, g, g^2 (lib/gf2k/gf2_128.h:121-127); g from the oracle's context
            g = self.of_img(tuple(int(x) for x in ol.gf_ctx(4).g.l))
            self.pts = [0, 1, g, self.mul(g, g)]

    # --- edges: (lo, hi) images <-> internal
    def of_img(self, e):
        x = int(e[0]) | int(e[1]) << 64
        if self.fid == FP:
            assert x < FP_P
            return x * _RINV % FP_P
        return int.from_bytes(bin(x)[2:].encode(), "big") & _M128  # '0' / '1' characters: the low bit of every byte

    def img(self, v):
        x = v * _R % FP_P if self.fid == FP else int(v.to_bytes(128, "big").hex()[1::2], 2)
        return (x & (2**64 - 1), x >> 64)

    def of_array(self, a):
        a = np.asarray(a, dtype=np.uint64).reshape(-1, 2)
        return [self.of_img((int(lo), int(hi))) for lo, hi in a]

    def array(self, vs):
        return np.array([self.img(v) for v in vs], dtype=np.uint64).reshape(-1, 2)

    # --- arithmetic
    def add(self, a, b):
        return (a + b) % FP_P if self.fid == FP else a ^ b

    def sub(self, a, b):
        return (a - b) % FP_P if self.fid == FP else a ^ b

    def neg(self, a):
        return -a % FP_P if self.fid == FP else a

    def mul(self, a, b):
        if self.fid == FP:
            return a * b % FP_P
        p = (a * b) & _M255  # carry-less product, degree <= 254
        for _ in range(2):  # x^128 = x^7 + x^2 + x + 1; the second pass folds the <= 6 coefficients the first pushes out
            hi = p >> 1024
            p = (p & _LOW) ^ hi ^ (hi << 8) ^ (hi << 16) ^ (hi << 56)
        return p

    def inv(self, a):
        assert a != 0
        if self.fid == FP:
            return pow(a, -1, FP_P)
        r, e, b = 1, 2**128 - 2, a  # a^(2^128 - 2)
        while e:
            if e & 1:
                r = self.mul(r, b)
            b = self.mul(b, b)
            e >>= 1
        return r

    # --- Poly<N> (lib/algebra/poly.h): Horner; the interpolant through (pts[i], ev[i]) at x (unique, so any exact formula)
    def eval_monomial(self, coef, x):
        e = coef[-1]
        for c_ in reversed(coef[:-1]):
            e = self.add(self.mul(e, x), c_)
        return e

    def eval_lagrange(self, ev, x):
        n, acc = len(ev), 0
        for i in range(n):
            num = den = 1
            for j in range(n):
                if j != i:
                    num = self.mul(num, self.sub(x, self.pts[j]))
                    den = self.mul(den, self.sub(self.pts[i], self.pts[j]))
            acc = self.add(acc, self.mul(ev[i], self.mul(num, self.inv(den))))
        return acc


# ---------------------------------------------------------------- arrays
def filleq(F, logn, n, Q):
    """Eqs::filleq (eqs.h:104-134): eq[i] = EQ(Q, i), i < n, by the reference's doubling recursion"""
    assert 0 < n <= 1 << logn
    eq = [0] * n
    eq[0] = F.one

    def ceilshr(a, k):
        return 1 + ((a - 1) >> k)

    for l in range(logn - 1, -1, -1):
        nl = ceilshr(n, l)
        i = ceilshr(nl, 1)
        if 2 * i - 1 >= nl:
            i -= 1
            v = eq[i]
            eq[2 * i] = F.sub(v, F.mul(Q[l], v))
        while i > 0:
            i -= 1
            v = eq[i]
            qv = F.mul(Q[l], v)
            eq[2 * i], eq[2 * i + 1] = F.sub(v, qv), qv
    return eq


def eq_product(F, logn, Q, Cpt):
    """eq(Q, C) = prod_l (Q[l] C[l] + (1 - Q[l]) (1 - C[l]))"""
    acc = F.one
    for l in range(logn):
        acc = F.mul(acc, F.add(F.mul(Q[l], Cpt[l]), F.mul(F.sub(F.one, Q[l]), F.sub(F.one, Cpt[l]))))
    return acc


def bind_row(F, row, r):
    """Dense::bind of one row (dense.h:76-84): in[2i] + r (in[2i+1] - in[2i]); an odd last entry is paired with zero"""
    n0 = len(row)
    out = [F.add(row[2 * i], F.mul(r, F.sub(row[2 * i + 1], row[2 * i]))) for i in range(n0 // 2)]
    if n0 & 1:
        out.append(F.sub(row[-1], F.mul(r, row[-1])))
    return out


def bind_rows(F, rows, r):
    return [bind_row(F, row, r) for row in rows]


def accumulators_c(F, EQ, W, hc, vc):
    """the loop of evaluations_c (:418-477): acc[0], acc[2], acc[3] in the Karatsuba form of :438-457, odd tail :460-472.
    W: rows indexed by wire, each of n0 = len(EQ) entries; hc: (r, l) pairs; vc: values"""
    n0, add, sub, mul = len(EQ), F.add, F.sub, F.mul
    nodd = n0 // 2
    acc = [0, 0, 0]
    folded = {}  # the sums over c depend on the hand pair only: folded once per distinct pair
    for (r_, l_), v in zip(hc, vc):
        if (r_, l_) in folded:
            l0, l2, l3 = folded[(r_, l_)]
            acc = [add(acc[0], mul(l0, v)), add(acc[1], mul(l2, v)), add(acc[2], mul(l3, v))]
            continue
        wr, wl = W[r_], W[l_]
        l0 = l2 = l3 = 0
        for c in range(nodd):
            eq0, eq1 = EQ[2 * c], EQ[2 * c + 1]
            wr0, wr1, wl0, wl1 = wr[2 * c], wr[2 * c + 1], wl[2 * c], wl[2 * c + 1]
            a1, b1, c1 = sub(eq1, eq0), sub(wr1, wr0), sub(wl1, wl0)
            d0, d2 = mul(eq0, wr0), mul(a1, b1)
            d1 = sub(sub(mul(eq1, wr1), d0), d2)
            l0 = add(l0, mul(d0, wl0))
            l2 = add(l2, add(mul(d1, c1), mul(d2, wl0)))
            l3 = add(l3, mul(d2, c1))
        if 2 * nodd < n0:
            eq0, wr0, wl0 = EQ[2 * nodd], wr[2 * nodd], wl[2 * nodd]
            d0 = mul(eq0, wr0)
            l0 = add(l0, mul(d0, wl0))
            l2 = add(l2, mul(d0, add(wl0, add(wl0, wl0))))
            l3 = add(l3, mul(d0, F.neg(wl0)))
        folded[(r_, l_)] = (l0, l2, l3)
        acc = [add(acc[0], mul(l0, v)), add(acc[1], mul(l2, v)), add(acc[2], mul(l3, v))]
    return acc


def evaluations_c(F, EQ, W, hc, vc, s):
    """CPoly evaluations_c (:415-496): the round's cubic at poly_evaluation_point(0..3)"""
    c0, c2, c3 = accumulators_c(F, EQ, W, hc, vc)
    c1 = F.sub(F.sub(F.sub(F.sub(s, c0), c0), c2), c3)
    return [F.eval_monomial([c0, c1, c2, c3], F.pts[k]) for k in range(4)]


def evaluations_c_direct(F, EQ, W, hc, vc, pts=None):
    """the same four values from the definition: p(t) = sum_i v_i sum_c' EQ_t[c'] Wr_t[c'] Wl_t[c'] with EQ and W bound at
    t by Dense::bind's formula (t over the evaluation points, or over pts).  Shares no code with accumulators_c."""
    out = []
    for t in F.pts if pts is None else pts:
        eq_t = bind_row(F, EQ, t)
        rows = {}
        tot = 0
        for (r_, l_), v in zip(hc, vc):
            for w in (r_, l_):
                if w not in rows:
                    rows[w] = bind_row(F, W[w], t)
            inner = 0
            for e, x, y in zip(eq_t, rows[r_], rows[l_]):
                inner = F.add(inner, F.mul(e, F.mul(x, y)))
            tot = F.add(tot, F.mul(v, inner))
        out.append(tot)
    return out


def mle_claim(F, V, nc, Q, G):
    """V~(G, Q): the multilinear extension of V[g * nc + c] at copy point Q and gate point G (images in, image out)"""
    Vi = F.of_array(V)
    rows = [Vi[g * nc:(g + 1) * nc] for g in range(len(Vi) // nc)]
    for q in Q:
        rows = bind_rows(F, rows, F.of_img(q))
    col = [row[0] for row in rows]
    for g in G:
        col = bind_row(F, col, F.of_img(g))
    assert len(col) == 1
    return F.img(col[0])


def eval_quad_copies(F, L, nc, W):
    """ProverLayers::eval_quad (:278-305) over nc copies.  W: uint64[nw * nc, 2] images, W[wire * nc + c].
    -> (ok, V images [nv * nc, 2]); V is meaningless when ok is False (the reference stops at the first failing term)"""
    Wi = F.of_array(W)
    K = F.of_array(L["kvec"])
    V = [0] * (L["nv"] * nc)
    ok = True
    for g, h0, h1, vi in zip(L["g"].tolist(), L["h0"].tolist(), L["h1"].tolist(), L["vi"].tolist()):
        for c in range(nc):
            y = F.mul(Wi[nc * h1 + c], Wi[nc * h0 + c])
            if K[vi] == 0:
                ok = ok and y == 0
            else:
                V[nc * g + c] = F.add(V[nc * g + c], F.mul(K[vi], y))
    return ok, F.array(V)


# ---------------------------------------------------------------- one layer
def layer(F, L, logc, nc, Q, logv, G0, G1, alpha, beta, W, wc_in, round_c, round_h):
    """ProverLayers::layer with the Eqs constructor and bind_g in front of it (:155-157,185-271).
    L: layer dict (g, h0, h1, vi, kvec, nv, nw, logw, n); Q: logc images; G0 / G1: uint64[max(1, logv), 2] images;
    alpha, beta, wc_in[2]: images; W: uint64[nw * nc, 2] images, W[wire * nc + c].
    round_c(round, evals[4]) / round_h(hand, round, evals[3]) get images and return the challenge image.
    -> dict(wc, q, g, bound_quad, eq0, sums (the running claim before every round), final_sum, nh0), images throughout"""
    o, fid = ol.oracle(), F.fid
    n, nw, logw = L["n"], L["nw"], L["logw"]
    assert 0 < nc <= 1 << logc and len(W) == nw * nc
    hc = np.zeros((n, 2), dtype=np.uint32)
    vc = np.zeros((n, 2), dtype=np.uint64)
    G0, G1 = np.ascontiguousarray(G0, dtype=np.uint64), np.ascontiguousarray(G1, dtype=np.uint64)
    nh = o.lfo_quad_bind_g(fid, n, P(L["g"]), P(L["h0"]), P(L["h1"]), P(L["vi"]), P(L["kvec"]), logv, P(G0), P(G1), elt(alpha), elt(beta),
                           P(hc), P(vc))
    nh0 = nh
    al = F.of_img(alpha)
    s = F.add(F.of_img(wc_in[0]), F.mul(al, F.of_img(wc_in[1])))
    sums, qs = [], []
    # --- the copy rounds (:202-212)
    EQ = filleq(F, logc, nc, [F.of_img(x) for x in Q[:logc]])
    if logc:
        Wi = F.of_array(W)
        rows = [Wi[w * nc:(w + 1) * nc] for w in range(nw)]
        hcl = [tuple(x) for x in hc[:nh].tolist()]
        vcl = F.of_array(vc[:nh])
        for rnd in range(logc):
            sums.append(F.img(s))
            ev = evaluations_c(F, EQ, rows, hcl, vcl, s)
            r_img = tuple(int(x) for x in round_c(rnd, [F.img(e) for e in ev]))
            qs.append(r_img)
            r = F.of_img(r_img)
            EQ = bind_row(F, EQ, r)
            rows = bind_rows(F, rows, r)
            s = F.eval_lagrange(ev, r)
        assert len(EQ) == 1 and all(len(row) == 1 for row in rows)
        Wv = F.array([row[0] for row in rows])
    else:
        Wv = np.ascontiguousarray(W, dtype=np.uint64).reshape(nw, 2).copy()
    eq0 = EQ[0]
    # --- the hand rounds (:230-263) on the oracle's array functions
    WH, nW = [Wv, Wv.copy()], [nw, nw]
    gs = [[], []]
    for rnd in range(logw):
        for hand in (0, 1):
            sums.append(F.img(s))
            qw = np.zeros((nW[hand], 2), dtype=np.uint64)
            o.lfo_qw_scatter(fid, nh, P(hc), P(vc), hand, P(WH[1 - hand]), nW[hand], P(qw))
            a0, a2 = ol.Elt(), ol.Elt()
            o.lfo_sumcheck_partials(fid, nW[hand], P(qw), P(WH[hand]), C.byref(a0), C.byref(a2))
            c0 = F.mul(eq0, F.of_img((a0.l[0], a0.l[1])))
            c2 = F.mul(eq0, F.of_img((a2.l[0], a2.l[1])))
            c1 = F.sub(F.sub(F.sub(s, c0), c0), c2)
            ev = [F.eval_monomial([c0, c1, c2], F.pts[k]) for k in range(3)]
            r_img = tuple(int(x) for x in round_h(hand, rnd, [F.img(e) for e in ev]))
            gs[hand].append(r_img)
            s = F.eval_lagrange(ev, F.of_img(r_img))
            out = np.zeros(((nW[hand] + 1) // 2, 2), dtype=np.uint64)
            o.lfo_dense_bind(fid, nW[hand], elt(r_img), P(WH[hand]), P(out))
            WH[hand], nW[hand] = out, (nW[hand] + 1) // 2
            nh = o.lfo_hquad_bind_h(fid, nh, P(hc), P(vc), elt(r_img), hand)
    wc = [tuple(int(x) for x in WH[0][0]), tuple(int(x) for x in WH[1][0])]
    bq = tuple(int(x) for x in vc[0])
    # (the check of :268-269, sum == eq0 * quad * wl * wr, holds when wc_in are true claims on this layer's outputs: the
    # tests of the verifier's identities assert it; with arbitrary wc_in the rounds are still well defined)
    return dict(wc=wc, q=qs, g=gs, bound_quad=bq, eq0=F.img(eq0), sums=sums, final_sum=F.img(s), nh0=nh0)


# ---------------------------------------------------------------- a whole proof (Prover::prove, pad = nullptr), GF2_128
def prove_circuit(circ, W_host, seed=b"testing"):
    """The transmitted proof bytes of the reference's sumcheck prover for ONE copy (logc = 0), in the order of the flatsha
    fixtures -- the transcript handling of sumcheck_driver.SumcheckBase.prove, every layer through layer() above."""
    import sumcheck_driver as sd
    from fs_transcript import Transcript
    F = ModelField(GF)
    ins, _ = sd.OracleSumcheck(circ).eval_circuit(W_host)
    assert ins is not None
    ts = Transcript(seed)
    ts.write_array([bytes(W_host[i].tobytes()) for i in range(len(W_host))])
    Q = [sd._e(ts.elt_gf2128()) for _ in range(sd.KMAX)]  # begin_circuit: Q then G
    g0 = [sd._e(ts.elt_gf2128()) for _ in range(sd.KMAX)]
    G = [list(g0), list(g0)]
    logv, WC, out = circ["logv"], [(0, 0), (0, 0)], bytearray()

    def round_h(hand, rnd, ev):
        nonlocal out
        out += sd._b16(ev[0]) + sd._b16(ev[2])
        ts.write_elt(sd._b16(ev[0]))
        ts.write_elt(sd._b16(ev[2]))
        return sd._e(ts.elt_gf2128())

    for ly, lay in enumerate(circ["layers"]):
        alpha, beta = sd._e(ts.elt_gf2128()), sd._e(ts.elt_gf2128())
        L = dict(lay, kvec=circ["kvec"], n=len(lay["g"]), nv=None)
        G0 = np.array(G[0][:max(1, logv)], dtype=np.uint64)
        G1 = np.array(G[1][:max(1, logv)], dtype=np.uint64)
        res = layer(F, L, 0, 1, Q, logv, G0, G1, alpha, beta, ins[ly], WC, None, round_h)
        WC = res["wc"]
        out += sd._b16(WC[0]) + sd._b16(WC[1])
        ts.write_array([sd._b16(WC[0]), sd._b16(WC[1])])
        G = [res["g"][h] + [(0, 0)] * (sd.KMAX - lay["logw"]) for h in (0, 1)]
        logv = lay["logw"]
    return bytes(out)

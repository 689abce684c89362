"""A Python-integer model of one sumcheck layer, over a modulus parameter: ProverLayers::layer with logc = 0 and the
Quad::bind_g in front of it (reference lib/sumcheck/prover_layers.h:185-271, lib/sumcheck/quad.h:152-185), restated
directly -- residues mod p inside, Montgomery images (little-endian 64-bit words) at the boundary.  It is the expectation of
the Fp256Base layer tests: the C oracle has no P-256 sumcheck.  tests/test_p256_layer_model.py pins it, run over the Fp128
modulus, to the oracle's step-by-step replay (which is itself pinned to the compiled reference), and its P-256 arithmetic
to the oracle's.

TEST INFRASTRUCTURE: nothing outside tests/ imports this module."""
import numpy as np

P256_P = 2**256 - 2**224 + 2**192 + 2**96 - 1
FP128_P = 2**128 - 2**108 + 1
_M64 = 2**64 - 1


class ModField:
    """p and the Montgomery radix R = 2^rbits; elements cross the boundary as tuples of rbits / 64 words"""

    def __init__(self, p, rbits):
        self.p, self.R, self.nwords = p, 1 << rbits, rbits // 64
        self.Rinv = pow(self.R, -1, p)

    def from_image(self, words):
        v = 0
        for k, w in enumerate(words):
            v |= int(w) << (64 * k)
        assert v < self.p, "not a canonical image"
        return v * self.Rinv % self.p

    def to_image(self, x):
        v = x * self.R % self.p
        return tuple((v >> (64 * k)) & _M64 for k in range(self.nwords))

    def from_images(self, a):
        return [self.from_image(row) for row in np.asarray(a, dtype=np.uint64).reshape(-1, self.nwords)]

    def to_images(self, xs):
        return np.array([self.to_image(x) for x in xs], dtype=np.uint64).reshape(len(xs), self.nwords)


P256 = ModField(P256_P, 256)
FP128 = ModField(FP128_P, 128)


def rand_images(rng, n, F=P256):
    """n canonical images as uint64[n, nwords]: the top bit is cleared, and 2^(rbits - 1) < p for both moduli"""
    a = rng.integers(0, 2**64, size=(n, F.nwords), dtype=np.uint64)
    a[:, -1] &= np.uint64(0x7FFFFFFFFFFFFFFF)
    return np.ascontiguousarray(a)


def raw_eq2(p, logn, n, G0, G1, alpha):
    """Eqs::raw_eq2: eq[i] = EQ(G0, i) + alpha EQ(G1, i), EQ(G, i) = prod_l (bit_l(i) ? G[l] : 1 - G[l])"""
    eq = []
    for i in range(n):
        e0, e1 = 1, alpha
        for l in range(logn):
            if (i >> l) & 1:
                e0, e1 = e0 * G0[l] % p, e1 * G1[l] % p
            else:
                e0, e1 = e0 * (1 - G0[l]) % p, e1 * (1 - G1[l]) % p
        eq.append((e0 + e1) % p)
    return eq


def bind_g(p, L, kvec, logv, G0, G1, alpha, beta):
    """Quad::bind_g: one HQUAD entry per run of equal hand pairs in canonical order, its value the sum over the run of
    prep_v(v, beta) * eq[g] (prep_v: beta for a zero constant) -> (h0[], h1[], v[])"""
    eq = raw_eq2(p, logv, L["nv"], G0, G1, alpha)
    H0, H1, V = [], [], []
    g, h0, h1, vi = (L[k].tolist() for k in ("g", "h0", "h1", "vi"))
    for i in range(L["n"]):
        v = kvec[vi[i]] or beta
        t = v * eq[g[i]] % p
        if H0 and H0[-1] == h0[i] and H1[-1] == h1[i]:
            V[-1] = (V[-1] + t) % p
        else:
            H0.append(h0[i])
            H1.append(h1[i])
            V.append(t)
    return H0, H1, V


def dense_bind(p, W, r):
    """Dense::bind: out[i] = in[2i] + r (in[2i+1] - in[2i]); the odd tail in[n-1] (1 - r)"""
    n = len(W)
    out = [(W[2 * i] + r * (W[2 * i + 1] - W[2 * i])) % p for i in range(n // 2)]
    if n & 1:
        out.append(W[n - 1] * (1 - r) % p)
    return out


def bind_h(p, H, O, V, r):
    """HQuad::bind_h of the hand whose indices are H (O: the other hand's): an order-preserving merge.  Three cases: the
    pair (2j, 2j + 1) under one other-hand corner -> v0 + r (v1 - v0); a lone even index -> v0 (1 - r); a lone odd -> v1 r"""
    nH, nO, nV = [], [], []
    i, n = 0, len(H)
    while i < n:
        if i + 1 < n and O[i + 1] == O[i] and (H[i] & 1) == 0 and H[i + 1] == H[i] + 1:
            v = (V[i] + r * (V[i + 1] - V[i])) % p
            step = 2
        elif (H[i] & 1) == 0:
            v, step = V[i] * (1 - r) % p, 1
        else:
            v, step = V[i] * r % p, 1
        nH.append(H[i] >> 1)
        nO.append(O[i])
        nV.append(v)
        i += step
    return nH, nO, nV


def layer(F, L, kvec, W, logv, G0, G1, alpha, beta, wc_in, chal):
    """All arguments but L are images; L: the layer (g, h0, h1, vi in canonical order, n, nv, nw, logw).
    -> (evaluations per round-hand [(e0, e1, e2)], wc_out [2], bound_quad, nh0), images as tuples of words"""
    p = F.p
    kvec, W = F.from_images(kvec), F.from_images(W)
    G0, G1 = F.from_images(G0)[:logv], F.from_images(G1)[:logv]
    alpha, beta = F.from_image(alpha), F.from_image(beta)
    hh = [None, None]
    hh[0], hh[1], V = bind_g(p, L, kvec, logv, G0, G1, alpha, beta)
    nh0 = len(V)
    WH = [list(W), list(W)]
    s = (F.from_image(wc_in[0]) + alpha * F.from_image(wc_in[1])) % p
    evs, k = [], 0
    for _rnd in range(L["logw"]):
        for hand in (0, 1):
            Wh, Wo = WH[hand], WH[1 - hand]
            n = len(Wh)
            QW = [0] * n  # the scatter (prover_layers.h:239-243)
            for a, b, v in zip(hh[hand], hh[1 - hand], V):
                QW[a] = (QW[a] + v * Wo[b]) % p
            a0 = a2 = 0  # evaluations (:357-402)
            for i in range(n // 2):
                a0 += QW[2 * i] * Wh[2 * i]
                a2 += (QW[2 * i + 1] - QW[2 * i]) * (Wh[2 * i + 1] - Wh[2 * i])
            if n & 1:  # the odd tail (:381-388)
                t = QW[n - 1] * Wh[n - 1]
                a0 += t
                a2 += t
            c0, c2 = a0 % p, a2 % p
            c1 = (s - 2 * c0 - c2) % p  # coef[1] from the running sum (:390-396)
            evs.append(tuple(F.to_image((c0 + x * (c1 + x * c2)) % p) for x in (0, 1, 2)))
            r = F.from_image(chal[k])
            k += 1
            s = (c0 + r * (c1 + r * c2)) % p
            WH[hand] = dense_bind(p, Wh, r)
            hh[hand], hh[1 - hand], V = bind_h(p, hh[hand], hh[1 - hand], V, r)
    assert len(V) == 1
    return evs, [F.to_image(WH[0][0]), F.to_image(WH[1][0])], F.to_image(V[0]), nh0


def eval_quad(F, L, kvec, W):
    """ProverLayers::eval_quad (nc = 1): V[g] = sum kvec[vi] W[h1] W[h0]; a term with a zero constant must have a zero
    product.  -> (V as images uint64[nv, nwords], ok)"""
    p = F.p
    kvec, W = F.from_images(kvec), F.from_images(W)
    V, ok = [0] * L["nv"], True
    for g, h0, h1, vi in zip(*(L[k].tolist() for k in ("g", "h0", "h1", "vi"))):
        t = W[h1] * W[h0] % p
        if kvec[vi] == 0:
            ok = ok and t == 0
        else:
            V[g] = (V[g] + kvec[vi] * t) % p
    return F.to_images(V), ok

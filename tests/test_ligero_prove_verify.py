"""lfgpu_ligero_prove / lfgpu_ligero_verify: LigeroProver::prove and LigeroVerifier::verify behind the C ABI.

The reference's own known-answer vector (tests/golden/ligero_test_vector.bin: W, lqc, 1000 linear terms over nl = 15 constraints,
b, hash_of_statement, the root and the C++ prover's 55 768 proof bytes) is reproduced byte for byte and verified.  Synthetic
statements over GF(2^128) and Fp128 are checked against the existing single calls (low_degree_proof / dot_proof /
quadratic_proof / open) fed by tests/fs_transcript.py, with the matrix A of inner_product_vector built in Python through the
oracle's lfo_mul / lfo_add; the term lists are chosen to break the device accumulation (unsorted, duplicates, one hot wire, more
than one grid stride, Fp128 limb carries)."""
import ctypes as C

import numpy as np
import pytest

import ligero_fixture as lf
import oracle_lib as ol
from ligero_statement import FP_P, LLTERM, M64, Statement, _a2i, _elts, _i2a, _ints, fadd, fmul, rand_terms, records
from oracle_lib import FP, GF

pytestmark = pytest.mark.gpu

REFERENCE_WHY = {"merkle_check failed", "low_degree_check failed", "dot_check failed", "wrong dot product", "quadratic_check failed"}


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


NW, NQ, NREQ, BE = 700, 40, 12, 512  # as test_ligero_prove_pieces_vs_oracle: w = 73, so the last witness row and the quadratic rows are partial
_stmts = {}


def stmt(G, field, nq=NQ):
    key = (field, nq)
    if key not in _stmts:
        # GF: the first witness row holds subfield elements, so the opening has two-byte runs
        _stmts[key] = Statement(G, field, NW, nq, NREQ, BE, seed=300 + field + nq, subfield_boundary=73 if field == GF and nq else 0)
    return _stmts[key]


def pad_with_cancelling_pairs(rng, field, base, total, nl, nw):
    """`total` records whose sums are those of `base`: base plus pairs (c, w, k), (c, w, -k), all in random order"""
    npair = (total - len(base)) // 2
    assert len(base) + 2 * npair == total
    ll = np.zeros(total, dtype=LLTERM)
    c = rng.integers(0, nl, size=npair).astype(np.uint64)
    w = rng.integers(0, nw, size=npair).astype(np.uint64)
    k = ol.rand_elts(rng, npair, field)
    nk = k if field == GF else _elts([(FP_P - x) % FP_P for x in _ints(k)])
    ll["c"][:npair], ll["w"][:npair], ll["k"][:npair] = c, w, k
    ll["c"][npair:2 * npair], ll["w"][npair:2 * npair], ll["k"][npair:2 * npair] = c, w, nk
    ll[2 * npair:] = records(base)
    return np.ascontiguousarray(ll[rng.permutation(total)])


# ---------------------------------------------------------------- the reference's known-answer vector
@pytest.fixture(scope="module")
def vector(G):
    v = lf.load()
    pkg = G.pkg
    p = pkg.ligero_param(pkg.FIELD_GF2_128, v["nw"], v["nq"], 4, v["nreq"], 4096)
    pr = pkg.LigeroProver(G.gpu(), pkg.FIELD_GF2_128, p)
    root = pr.commit(v["W"], v["subfield_boundary"], v["lqc"], lf.LcgRng(100).bytes)
    assert root == v["root"]
    ts = pkg.FsTranscript(b"test")
    ts.write_bytes(root)
    ll = records([(c, w, _a2i(k)) for (c, w, k) in v["llterm"]])
    proof = pr.prove(ts, v["nl"], ll, v["hash_of_statement"], v["lqc"])
    ts.close()
    yield dict(v=v, p=p, ll=ll, proof=proof)
    pr.close()


def _verify_vector(G, vec, proof, b=None):
    v, pkg = vec["v"], G.pkg
    ts = pkg.FsTranscript(b"test")
    ts.write_bytes(v["root"])
    r = pkg.ligero_verify(G.gpu(), pkg.FIELD_GF2_128, vec["p"], v["root"], proof, ts, v["nl"], vec["ll"], v["hash_of_statement"],
                          v["b"] if b is None else b, v["lqc"])
    ts.close()
    return r


def test_reference_vector_proof_bytes(G, vector):
    want = vector["v"]["proof"]
    assert len(want) == 55768
    assert len(vector["proof"]) == len(want)
    assert vector["proof"] == want


def test_reference_vector_verifies(G, vector):
    assert _verify_vector(G, vector, vector["proof"]) == (True, "ok")
    assert _verify_vector(G, vector, vector["v"]["proof"]) == (True, "ok")


def _flip(d, off, bit=0):
    d = bytearray(d)
    d[off] ^= 1 << bit
    return bytes(d)


def test_reference_vector_rejections(G, vector):
    d = vector["v"]["proof"]
    o_ydot, o_q0, o_q2, o_nonce = 16 * 682, 16 * (682 + 1363), 16 * (682 + 1363 + 36), 16 * (682 + 1363 + 36 + 681)
    o_req = o_nonce + 32 * 36
    o_path = len(d) - 32 * 197
    assert _verify_vector(G, vector, _flip(d, o_path + 32 * 5 + 7)) == (False, "merkle_check failed")
    assert _verify_vector(G, vector, _flip(d, o_nonce + 32 * 3 + 1)) == (False, "merkle_check failed")
    b = vector["v"]["b"].copy()
    b[0, 0] ^= np.uint64(1)
    assert _verify_vector(G, vector, d, b=b) == (False, "wrong dot product")
    assert _verify_vector(G, vector, d[:-1]) == (False, "proof does not parse")
    assert _verify_vector(G, vector, d + b"\x00") == (False, "proof does not parse")
    for off in (16 * 10 + 3, o_ydot + 16 * 700 + 2, o_q0 + 16 * 4, o_q2 + 16 * 99 + 9, o_req + 4 + 16 * 17 + 5):  # y_ldt, y_dot, y_q0, y_q2, req
        ok, why = _verify_vector(G, vector, _flip(d, off, 3))
        assert not ok and why in REFERENCE_WHY, (off, why)


# ---------------------------------------------------------------- against the pieces
@pytest.mark.parametrize("field", [GF, FP])
def test_prove_matches_the_pieces(G, field):
    s = stmt(G, field)
    p = s.p
    rng = np.random.default_rng(11 + field)
    nl = 9
    terms = rand_terms(rng, field, 150, nl, NW)
    proof = s.check(nl, terms)
    o_req = 16 * (p.block + p.dblock + p.r + p.dblock - p.block) + 32 * NREQ
    run0, = np.frombuffer(proof, dtype="<u4", count=1, offset=o_req)
    if field == GF:  # three blinding rows at full width, then the subfield witness row as two-byte images
        run1, = np.frombuffer(proof, dtype="<u4", count=1, offset=o_req + 4 + 16 * int(run0))
        assert (run0, run1) == (3 * NREQ, NREQ)
    else:
        assert run0 == 0
    # a wrong right-hand side and a wrong root are refused
    b = s.b_of(nl, terms)
    b[3] = fadd(field, b[3], 1)
    assert s.verify(proof, nl, records(terms), bytes(range(32)), b) == (False, "wrong dot product")
    assert s.verify(proof, nl, records(terms), bytes(range(32)), s.b_of(nl, terms), root=bytes(32)) == (False, "merkle_check failed")


@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("case", ["none", "one", "hot_wire", "last_wire", "duplicates", "last_constraint", "lqc_target"])
def test_term_lists_small(G, field, case):
    s = stmt(G, field)
    rng = np.random.default_rng(1000 + field)
    nl = 6
    k1 = _ints(ol.rand_elts(rng, 1, field))[0]
    if case == "none":
        terms = []
    elif case == "one":
        terms = [(2, 17, k1)]
    elif case == "hot_wire":  # 5000 terms all on one w
        ks = _ints(ol.rand_elts(rng, 5000, field))
        terms = [(int(rng.integers(0, nl)), 123, ks[i]) for i in range(5000)]
    elif case == "last_wire":  # every term on w = nw - 1: the last, partial row (700 = 9 * 73 + 43)
        assert NW % s.p.w != 0
        terms = [(c, NW - 1, k) for (c, _, k) in rand_terms(rng, field, 300, nl, NW)]
    elif case == "duplicates":  # the same (c, w) pair again and again, between other terms
        t = rand_terms(rng, field, 40, nl, NW)
        terms = t + [(c, w, k1) for (c, w, _) in t] + t[:7] * 3
        terms = [terms[i] for i in rng.permutation(len(terms))]
    elif case == "last_constraint":
        terms = [(nl - 1, w, k) for (_, w, k) in rand_terms(rng, field, 200, nl, NW)]
    else:  # an lqc index that is also a target of linear terms
        x, y, z = s.lqc[3]
        terms = rand_terms(rng, field, 50, nl, NW) + [(0, x, k1), (1, z, k1), (5, y, k1), (2, z, k1)]
    s.check(nl, terms)


@pytest.mark.parametrize("field", [GF, FP])
def test_no_quadratic_constraints(G, field):
    s = stmt(G, field, nq=0)
    assert s.p.nqtriples == 0
    s.check(4, rand_terms(np.random.default_rng(5 + field), field, 100, 4, NW))


@pytest.mark.parametrize("field", [GF, FP])
def test_more_than_one_grid_stride(G, field):
    """300 001 terms in random order (the kernels sweep 262 144 per grid stride): 301 terms plus cancelling pairs"""
    s = stmt(G, field)
    rng = np.random.default_rng(77 + field)
    nl = 15
    base = rand_terms(rng, field, 301, nl, NW)
    s.check(nl, pad_with_cancelling_pairs(rng, field, base, 300001, nl, NW), folded=base)


def test_fp128_limb_carries(G):
    """70 000 terms of value p - 1 on one entry: the 32-bit limb sums run far past 2^32"""
    s = stmt(G, FP)
    n, nl = 70000, 3
    ll = np.zeros(n, dtype=LLTERM)
    ll["c"], ll["w"] = 1, 5
    ll["k"][:, 0], ll["k"][:, 1] = (FP_P - 1) & M64, (FP_P - 1) >> 64
    s.check(nl, ll, folded=[(1, 5, fmul(FP, (n << 128) % FP_P, FP_P - 1))])  # n * (p - 1) as one term


def test_gf2_128_k5_round_trip(G):
    """GF2_128<5> (32-bit subfield, four-byte subfield runs on the wire): what the prover writes the verifier accepts, and one
    flipped bit it does not"""
    pkg, gpu = G.pkg, G.gpu()
    rng = np.random.default_rng(55)
    nw, nq, nl = 300, 0, 5
    p = pkg.ligero_param(GF, nw, nq, 4, NREQ, BE, subfield_log_bits=5)
    W = ol.rand_elts(rng, nw, GF)
    beta5 = ol.gf_ctx(5).beta
    for i in range(p.w):  # the first witness row lies in the subfield
        u, v = int(rng.integers(0, 1 << 32)), 0
        for j in range(32):
            if (u >> j) & 1:
                v ^= int(beta5[j].l[0]) | int(beta5[j].l[1]) << 64
        W[i] = _i2a(v)
    eng = np.random.default_rng(56)
    pr = pkg.LigeroProver(gpu, GF, p, subfield_log_bits=5)
    root = pr.commit(W, p.w, [], lambda n: bytes(eng.integers(0, 256, size=n, dtype=np.uint8)))
    terms = rand_terms(rng, GF, 200, nl, nw)
    Wi = _ints(W)
    b = [0] * nl
    for (c, w, k) in terms:
        b[c] ^= fmul(GF, k, Wi[w])
    ts = pkg.FsTranscript(b"k5")
    ts.write_bytes(root)
    proof = pr.prove(ts, nl, records(terms), bytes(32), [])
    ts.close()

    def verify(d):
        tv = pkg.FsTranscript(b"k5")
        tv.write_bytes(root)
        r = pkg.ligero_verify(gpu, GF, p, root, d, tv, nl, records(terms), bytes(32), _elts(b), [], subfield_log_bits=5)
        tv.close()
        return r

    o_req = 16 * (p.block + p.dblock + p.r + p.dblock - p.block) + 32 * NREQ
    run0, = np.frombuffer(proof, dtype="<u4", count=1, offset=o_req)
    run1, = np.frombuffer(proof, dtype="<u4", count=1, offset=o_req + 4 + 16 * int(run0))
    run2, = np.frombuffer(proof, dtype="<u4", count=1, offset=o_req + 8 + 16 * int(run0) + 4 * int(run1))  # four bytes an element
    assert (run0, run1, run0 + run1 + run2) == (3 * NREQ, NREQ, p.nrow * NREQ)
    assert verify(proof) == (True, "ok")
    ok, why = verify(_flip(proof, 16 * p.block + 40))
    assert not ok and why in REFERENCE_WHY
    pr.close()


# ---------------------------------------------------------------- argument errors leave the transcript alone
class CountingTranscript:
    """a transcript whose every hook counts the call"""

    def __init__(self, pkg):
        self.calls = 0

        def hit(*_a):
            self.calls += 1

        vp, sz = C.c_void_p, C.c_size_t
        self.fns = [C.CFUNCTYPE(None, vp, vp, sz)(hit), C.CFUNCTYPE(None, vp, vp)(hit), C.CFUNCTYPE(None, vp, vp, sz)(hit),
                    C.CFUNCTYPE(None, vp, vp, sz)(hit), C.CFUNCTYPE(vp, vp)(hit), C.CFUNCTYPE(None, vp)(hit)]
        self._ops = pkg.TranscriptOps(None, *[C.cast(f, vp) for f in self.fns], None, None)

    def ops(self):
        return self._ops


@pytest.mark.parametrize("field", [GF, FP])
def test_argument_errors(G, field):
    pkg, gpu = G.pkg, G.gpu()
    s = stmt(G, field)
    L, p = gpu.L, s.p
    ts = CountingTranscript(pkg)
    good = [(0, 1, 1), (2, NW - 1, 1)]
    h32 = bytes(32)
    b3 = np.zeros((3, 2), dtype=np.uint64)
    for bad in ([(3, 1, 1)], good + [(0, NW, 1)], [(1 << 40, 0, 1)]):  # c >= nl, w >= nw
        with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
            s.pr.prove(ts, 3, records(bad), h32, s.lqc)
        with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
            pkg.ligero_verify(gpu, field, p, s.root, b"\x00" * 64, ts, 3, records(bad), h32, b3, s.lqc)
    bad_lqc = list(s.lqc)
    bad_lqc[-1] = (bad_lqc[-1][0], NW, bad_lqc[-1][2])
    with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
        s.pr.prove(ts, 3, records(good), h32, bad_lqc)
    with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
        pkg.ligero_verify(gpu, field, p, s.root, b"\x00" * 64, ts, 3, records(good), h32, b3, bad_lqc)
    with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):  # Fp256Base
        pkg.ligero_verify(gpu, pkg.FIELD_P256, p, s.root, b"\x00" * 64, ts, 3, records(good), h32, b3, s.lqc)
    # NULL arguments and nllterm >= 2^32, straight at the C ABI
    ll = records(good)
    lq = np.ascontiguousarray(np.asarray(s.lqc, dtype=np.uint64).reshape(-1))
    ops, n = ts.ops(), C.c_size_t()

    def vp(a):
        return C.c_void_p(a.ctypes.data)

    ERR_ARG, ERR_UNSUPPORTED = 1, 3
    pa = [s.pr.h, C.byref(ops), 3, 2, vp(ll), h32, vp(lq), None, 0, C.byref(n)]
    for i in (0, 1, 4, 5, 6, 9):
        a = list(pa)
        a[i] = None
        assert L.lfgpu_ligero_prove(*a) == ERR_ARG, i
    a = list(pa)
    a[3] = 1 << 32
    assert L.lfgpu_ligero_prove(*a) == ERR_ARG
    ok, why = C.c_int(), C.c_char_p()
    va = [gpu.h, field, 4, C.byref(p), s.root, b"\x00" * 64, 64, C.byref(ops), 3, 2, vp(ll), h32, vp(b3), vp(lq), C.byref(ok), C.byref(why)]
    for i in (0, 3, 4, 5, 7, 10, 11, 12, 13, 14):
        a = list(va)
        a[i] = None
        assert L.lfgpu_ligero_verify(*a) == ERR_ARG, i
    a = list(va)
    a[9] = 1 << 32
    assert L.lfgpu_ligero_verify(*a) == ERR_ARG
    # a prover over a caller's slab is refused
    h = C.c_void_p()
    gpu._ck(L.lfgpu_ligero_prover_from_slab(gpu.h, field, 4, C.byref(p), 0, p.nrow, C.c_void_p(s.pr.tableau_ptr()), None, None, C.byref(h)))
    a = list(pa)
    a[0] = h
    assert L.lfgpu_ligero_prove(*a) == ERR_UNSUPPORTED
    L.lfgpu_ligero_free(h)
    assert ts.calls == 0, "a refused call touched the transcript"


# ---------------------------------------------------------------- the same bytes again: scratch reuse, accumulator clearing
@pytest.mark.parametrize("field", [GF, FP])
def test_same_bytes_again(G, field):
    a, b = stmt(G, field), stmt(G, field, nq=0)
    rng = np.random.default_rng(9 + field)
    ta = records(rand_terms(rng, field, 2000, 7, NW))
    tb = records(rand_terms(rng, field, 10, 2, NW))
    h = bytes(32)
    a1, a2, b1, b2, a3, b3 = a.prove(7, ta, h), a.prove(7, ta, h), b.prove(2, tb, h), b.prove(2, tb, h), a.prove(7, ta, h), b.prove(2, tb, h)
    assert a1 == a2 == a3 and b1 == b2 == b3
    assert a.prove(7, np.ascontiguousarray(ta[::-1]), h) == a1, "the result depends on the order of the terms"


def test_close_statements(G):
    """(last) the module's committed provers go back to the pool"""
    for s in _stmts.values():
        s.close()
    _stmts.clear()

"""Ligero over Fp256Base behind the C ABI: lfgpu_ligero_commit / low_degree_proof / dot_proof / quadratic_proof / open / tableau
for LFGPU_FIELD_P256, and lfgpu_ligero_prove256 / lfgpu_ligero_verify256 on a caller's own statement.

The reference's known-answer vector (tests/ligero_p256_fixture.py) is reproduced byte for byte and verified.  Synthetic statements
are compared, every element and every proof byte, with the Python model of tests/ligero_p256_model.py (pinned against that same
vector on the CPU by test_ligero_p256_model.py); the term lists are chosen to break the device accumulation of the dot proof's
matrix: unsorted, duplicates, one hot wire, the partial last witness row, 2^17 copies of one term (limb sums past 2^48 when summed
term by term, carries between limbs and the fold above 2^256), more than one sweep of the kernel's grid.  Every expected value is
exact: no tolerance is involved."""
import ctypes as C
import importlib

import numpy as np
import pytest

import ligero_p256_fixture as lf
import ligero_p256_model as lm
from fs_transcript import Transcript

pytestmark = pytest.mark.gpu

REFERENCE_WHY = {"merkle_check failed", "low_degree_check failed", "dot_check failed", "wrong dot product", "quadratic_check failed"}
ERR_ARG, ERR_UNSUPPORTED = 1, 3
SWEEP = 256 * 1024  # terms per sweep of a_terms256_kernel's grid: AT256_THREADS * AT256_BLOCKS_MAX (zk256.hip)


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _flip(d, off, bit=0):
    d = bytearray(d)
    d[off] ^= 1 << bit
    return bytes(d)


# ---------------------------------------------------------------- 1. the reference's known-answer vector
@pytest.fixture(scope="module")
def vector(G):
    v = lf.load()
    pkg = G.pkg
    p = pkg.ligero_param(pkg.FIELD_P256, v["nw"], v["nq"], 4, v["nreq"], 0)
    pr = pkg.LigeroProver(G.gpu(), pkg.FIELD_P256, p)
    root = pr.commit(v["W"], 0, v["lqc"], lf.commit_engine(v).bytes)
    ts = pkg.FsTranscript(b"test")
    ts.write_bytes(root)
    ll = lm.records([(c, w, lm.a2i(k)) for (c, w, k) in v["llterm"]])
    proof = pr.prove(ts, v["nl"], ll, v["hash_of_statement"], v["lqc"])
    ts.close()
    yield dict(v=v, p=p, ll=ll, root=root, proof=proof)
    pr.close()


def _verify_vector(G, vec, proof, b=None):
    v, pkg = vec["v"], G.pkg
    ts = pkg.FsTranscript(b"test")
    ts.write_bytes(v["root"])
    r = pkg.ligero_verify256(G.gpu(), vec["p"], v["root"], proof, ts, v["nl"], vec["ll"], v["hash_of_statement"], v["b"] if b is None else b, v["lqc"])
    ts.close()
    return r


def test_reference_vector_root_and_proof_bytes(G, vector):
    want = vector["v"]["proof"]
    assert vector["root"] == vector["v"]["root"]
    assert len(vector["proof"]) == len(want) == 20332
    assert vector["proof"] == want


def test_reference_vector_verifies(G, vector):
    assert _verify_vector(G, vector, vector["proof"]) == (True, "ok")
    assert _verify_vector(G, vector, vector["v"]["proof"]) == (True, "ok")


def test_reference_vector_rejections(G, vector):
    d, p = vector["v"]["proof"], vector["p"]
    o_ydot = 32 * p.block
    o_q0 = o_ydot + 32 * p.dblock
    o_q2 = o_q0 + 32 * p.r
    o_nonce = o_q2 + 32 * (p.dblock - p.block)
    o_req = o_nonce + 32 * p.nreq
    npath, = np.frombuffer(d, dtype="<u4", count=1, offset=o_req + 8 + 32 * p.nrow * p.nreq)
    o_path = len(d) - 32 * int(npath)
    assert o_path == o_req + 8 + 32 * p.nrow * p.nreq + 4 and npath > 5
    for off in (32 * 10 + 3, o_ydot + 32 * 100 + 2, o_q0 + 32 * 4, o_q2 + 32 * 70 + 9, o_req + 8 + 32 * 17 + 5,  # y_ldt, y_dot, y_q0, y_q2, req
                o_nonce + 32 * 3 + 1, o_path + 32 * 5 + 7):  # a nonce, a path digest
        ok, why = _verify_vector(G, vector, _flip(d, off, 3))
        assert not ok and why in REFERENCE_WHY, (off, why)
    assert _verify_vector(G, vector, _flip(d, o_nonce + 32 * 3 + 1))[1] == "merkle_check failed"
    b = lm.ints(vector["v"]["b"])
    b[0] = (b[0] + lm.of_scalar(1)) % lm.P
    assert _verify_vector(G, vector, d, b=lm.elts(b)) == (False, "wrong dot product")
    assert _verify_vector(G, vector, d[:-1]) == (False, "proof does not parse")
    assert _verify_vector(G, vector, d + b"\x00") == (False, "proof does not parse")


# ---------------------------------------------------------------- statements against the model
NW, NQ, NREQ, BE = 700, 40, 12, 512  # the shape of the 16-byte tests: w = 73, the last witness row and the quadratic rows partial, 343 leaves


class Statement:
    """a committed device prover and the model over the same tableau: a random witness with nq quadratic constraints"""

    def __init__(self, G, nq, seed):
        pkg = G.pkg
        rng = np.random.default_rng(seed)
        self.G = G
        self.p = p = pkg.ligero_param(pkg.FIELD_P256, NW, nq, 4, NREQ, BE)
        W = lm.rand_ints(rng, NW)
        self.lqc = []
        zs = rng.choice(np.arange(NW // 2, NW), size=nq, replace=False) if nq else []
        for i in range(nq):
            x, y, z = int(rng.integers(0, NW // 2)), int(rng.integers(0, NW // 2)), int(zs[i])
            W[z] = lm.mul(W[x], W[y])
            self.lqc.append((x, y, z))
        self.W = W
        Wa = lm.elts(W)

        def engine():
            eng = np.random.default_rng(seed + 1)
            return lambda n: bytes(eng.integers(0, 256, size=n, dtype=np.uint8))

        self.T, self.nonces = lm.tableau(pkg, p, Wa, self.lqc, engine())
        self.model = lm.Model(p, self.T, self.nonces, self.lqc)
        self.pr = pkg.LigeroProver(G.gpu(), pkg.FIELD_P256, p)
        self.root = self.pr.commit(Wa, 0, self.lqc, engine())

    def b_of(self, nl, terms):
        b = [0] * nl
        for (c, w, k) in terms:
            b[c] = (b[c] + lm.mul(k, self.W[w])) % lm.P
        return b

    def expected(self, nl, terms, hash32, seed=b"ligero"):
        ts = Transcript(seed)
        ts.write_bytes(self.root)
        return self.model.prove(ts, nl, terms, hash32), ts.bytes(32)

    def prove(self, nl, ll, hash32, seed=b"ligero"):
        ts = self.G.pkg.FsTranscript(seed)
        ts.write_bytes(self.root)
        proof = self.pr.prove(ts, nl, ll, hash32, self.lqc)
        nxt = ts.bytes(32)
        ts.close()
        return proof, nxt

    def verify(self, proof, nl, ll, hash32, b, seed=b"ligero"):
        ts = self.G.pkg.FsTranscript(seed)
        ts.write_bytes(self.root)
        r = self.G.pkg.ligero_verify256(self.G.gpu(), self.p, self.root, proof, ts, nl, ll, hash32, lm.elts(b), self.lqc)
        ts.close()
        return r

    def check(self, nl, given, folded=None, hash32=bytes(range(32))):
        """prove256 on the list `given` == the model on `folded` (the same sums in fewer terms; default: given itself), the
        transcript ends in the same state, and verify256 accepts"""
        folded = given if folded is None else folded
        want, want_next = self.expected(nl, folded, hash32)
        ll = given if isinstance(given, np.ndarray) else lm.records(given)
        got, got_next = self.prove(nl, ll, hash32)
        o_dot, n_dot = 32 * self.p.block, 32 * self.p.dblock
        assert got[:o_dot] == want[:o_dot], "y_ldt differs"
        assert got[o_dot:o_dot + n_dot] == want[o_dot:o_dot + n_dot], "y_dot differs"
        assert got == want
        assert got_next == want_next, "the transcript was left in another state"
        assert self.verify(got, nl, ll, hash32, self.b_of(nl, folded)) == (True, "ok")
        return got

    def close(self):
        self.pr.close()


_stmts = {}


def stmt(G, nq=NQ):
    if nq not in _stmts:
        _stmts[nq] = Statement(G, nq, seed=500 + nq)
    return _stmts[nq]


def rand_terms(rng, n, nl, nw=NW):
    ks = lm.rand_ints(rng, n)
    return [(int(rng.integers(0, nl)), int(rng.integers(0, nw)), ks[i]) for i in range(n)]


# ---------------------------------------------------------------- 2. the pieces
def test_shape(G):
    p = stmt(G).p
    assert (p.block, p.w, p.dblock, p.nrow, p.block_ext) == (85, 73, 169, 16, 343)
    assert NW % p.w != 0 and NQ % p.w != 0


def test_root_and_tableau(G):
    s = stmt(G)
    p = s.p
    assert s.root == lm.root_of(p, s.T, s.nonces) == s.model.root()
    got = np.zeros((p.nrow, p.block_enc, 4), dtype=np.uint64)
    G.gpu().memcpy_d2h(got, s.pr.tableau_ptr())
    assert (got == s.T).all()


def test_pieces_against_the_model(G):
    s = stmt(G)
    p, m = s.p, s.model
    rng = np.random.default_rng(21)
    u = lm.rand_ints(rng, p.nwqrow)
    assert lm.ints(s.pr.low_degree_proof(lm.elts(u))) == m.low_degree(u)
    A = lm.rand_ints(rng, p.nwqrow * p.w)
    assert lm.ints(s.pr.dot_proof(lm.elts(A))) == m.dot(A)
    uq = lm.rand_ints(rng, p.nqtriples)
    y0, y2 = s.pr.quadratic_proof(lm.elts(uq))
    w0, w2 = m.quadratic(uq)
    assert lm.ints(y0) == w0 and lm.ints(y2) == w2
    idx = [0, 342] + [int(x) for x in rng.choice(np.arange(1, 342), size=NREQ - 2, replace=False)]
    req, nonces, path = s.pr.open(idx)
    wreq, wnonces, wpath = m.open(idx)
    assert [lm.ints(req[i]) for i in range(p.nrow)] == wreq
    assert [bytes(nonces[i]) for i in range(NREQ)] == wnonces
    assert path == wpath


# ---------------------------------------------------------------- 3. term lists chosen to break the accumulation
def test_random_terms_unsorted(G):
    s = stmt(G)
    rng = np.random.default_rng(11)
    nl = 9
    terms = rand_terms(rng, 150, nl)
    proof = s.check(nl, terms)
    b = s.b_of(nl, terms)
    b[3] = (b[3] + lm.of_scalar(1)) % lm.P
    assert s.verify(proof, nl, lm.records(terms), bytes(range(32)), b) == (False, "wrong dot product")


def test_hot_wire(G):
    """5000 terms on ONE wire, spread over all constraints"""
    s = stmt(G)
    rng = np.random.default_rng(12)
    nl = 6
    ks = lm.rand_ints(rng, 5000)
    s.check(nl, [(i % nl, 123, ks[i]) for i in range(5000)])


def test_last_partial_witness_row(G):
    """every wire of the last witness row, which is partial (700 = 9 * 73 + 43)"""
    s = stmt(G)
    rng = np.random.default_rng(13)
    nl = 5
    lo = (NW // s.p.w) * s.p.w
    ks = lm.rand_ints(rng, NW - lo)
    terms = [(int(rng.integers(0, nl)), w, ks[w - lo]) for w in range(lo, NW)]
    s.check(nl, [terms[i] for i in rng.permutation(len(terms))])


def test_many_copies_of_one_term(G):
    """2^17 + 3 copies of one (c, w, k): expected n k alphal[c] mod p, as ONE term of the model"""
    s = stmt(G)
    n, nl = (1 << 17) + 3, 3
    k = lm.P - 1
    ll = np.repeat(lm.records([(1, 5, k)]), n)
    assert len(ll) == n
    s.check(nl, np.ascontiguousarray(ll), folded=[(1, 5, n * k % lm.P)])


def pad_with_cancelling_pairs(rng, base, total, nl):
    """`total` records whose sums are those of `base`: base plus pairs (c, w, k), (c, w, p - k), all in random order"""
    npair = (total - len(base)) // 2
    assert len(base) + 2 * npair == total
    ll = np.zeros(total, dtype=lm.LLTERM256)
    c = rng.integers(0, nl, size=npair).astype(np.uint64)
    w = rng.integers(0, NW, size=npair).astype(np.uint64)
    ks = [int(x) for x in rng.integers(1, 1 << 62, size=npair)]  # (small images are elements like any other)
    ll["c"][:npair], ll["w"][:npair], ll["k"][:npair] = c, w, lm.elts(ks)
    ll["c"][npair:2 * npair], ll["w"][npair:2 * npair], ll["k"][npair:2 * npair] = c, w, lm.elts([lm.P - x for x in ks])
    ll[2 * npair:] = lm.records(base)
    return np.ascontiguousarray(ll[rng.permutation(total)])


def test_more_than_one_grid_sweep(G):
    """one term more than one sweep of the kernel's grid: 301 terms plus cancelling pairs, in random order"""
    s = stmt(G)
    rng = np.random.default_rng(77)
    nl = 15
    base = rand_terms(rng, 301, nl)
    got = s.check(nl, pad_with_cancelling_pairs(rng, base, SWEEP + 1, nl), folded=base)
    assert got == s.prove(nl, lm.records(base), bytes(range(32)))[0]


def test_term_order_does_not_matter(G):
    s = stmt(G)
    rng = np.random.default_rng(9)
    t = rand_terms(rng, 40, 7)
    ta = lm.records(t + [(c, w, 5) for (c, w, _) in t] + t[:7] * 3 + rand_terms(rng, 2000, 7))
    h = bytes(32)
    a1 = s.prove(7, ta, h)
    assert s.prove(7, np.ascontiguousarray(ta[::-1]), h) == a1
    assert s.prove(7, np.ascontiguousarray(ta[rng.permutation(len(ta))]), h) == a1
    assert s.prove(7, ta, h) == a1  # scratch reuse, accumulator clearing


def test_edge_statements(G):
    s = stmt(G)
    s.check(0, [])  # nllterm = 0 with nl = 0: the copy constraints alone
    s0 = stmt(G, nq=0)
    assert s0.p.nqtriples == 0
    s0.check(4, rand_terms(np.random.default_rng(5), 100, 4))
    s0.check(0, [])


# ---------------------------------------------------------------- 4. size query then copy
def _prove_args(s, ops, nl, ll, h32, lq, n):
    return [s.pr.h, C.byref(ops), nl, len(ll), C.c_void_p(ll.ctypes.data), h32, C.c_void_p(lq.ctypes.data) if lq.size else None, None, 0, C.byref(n)]


def test_size_query_then_copy(G):
    pkg, L = G.pkg, G.gpu().L
    s = stmt(G)
    nl = 4
    terms = rand_terms(np.random.default_rng(31), 60, nl)
    ll, lq = lm.records(terms), np.ascontiguousarray(np.asarray(s.lqc, dtype=np.uint64).reshape(-1))
    h32 = bytes(range(32))
    want, want_next = s.expected(nl, terms, h32)
    ts = pkg.FsTranscript(b"ligero")
    ts.write_bytes(s.root)
    ops, n = ts.ops(), C.c_size_t()
    a = _prove_args(s, ops, nl, ll, h32, lq, n)
    assert L.lfgpu_ligero_prove256(*a) == 0 and n.value == len(want)  # the size query runs the proof
    small = C.create_string_buffer(len(want) - 1)
    n.value = 0
    a[7], a[8] = small, len(want) - 1
    assert L.lfgpu_ligero_prove256(*a) == ERR_ARG and n.value == len(want)  # too small: the size again, the bytes stay held
    buf = C.create_string_buffer(len(want))
    a[7], a[8] = buf, len(want)
    assert L.lfgpu_ligero_prove256(*a) == 0 and buf.raw == want
    assert ts.bytes(32) == want_next, "the transcript advanced more than once"
    ts.close()
    # a buffer too small with no size query in front: LFGPU_ERR_ARG with the size, then the copy
    ts = pkg.FsTranscript(b"ligero")
    ts.write_bytes(s.root)
    ops = ts.ops()
    a = _prove_args(s, ops, nl, ll, h32, lq, n)
    n.value = 0
    a[7], a[8] = small, 16
    assert L.lfgpu_ligero_prove256(*a) == ERR_ARG and n.value == len(want)
    a[7], a[8] = buf, len(want)
    C.memset(buf, 0, len(want))
    assert L.lfgpu_ligero_prove256(*a) == 0 and buf.raw == want
    assert ts.bytes(32) == want_next
    ts.close()


# ---------------------------------------------------------------- 5. argument errors, found on the host
class CountingTranscript:
    """a transcript whose every hook counts the call; sized=False: without the writes of 32-byte elements"""

    def __init__(self, pkg, sized=True):
        self.calls = 0

        def hit(*_a):
            self.calls += 1

        vp, sz = C.c_void_p, C.c_size_t
        self.fns = [C.CFUNCTYPE(None, vp, vp, sz)(hit), C.CFUNCTYPE(None, vp, vp)(hit), C.CFUNCTYPE(None, vp, vp, sz)(hit),
                    C.CFUNCTYPE(None, vp, vp, sz)(hit), C.CFUNCTYPE(vp, vp)(hit), C.CFUNCTYPE(None, vp)(hit),
                    C.CFUNCTYPE(None, vp, vp, sz)(hit), C.CFUNCTYPE(None, vp, vp, sz, sz)(hit)]
        ptrs = [C.cast(f, vp) for f in self.fns]
        self._ops = pkg.TranscriptOps(None, *ptrs[:6], *(ptrs[6:] if sized else (None, None)))

    def ops(self):
        return self._ops


def test_argument_errors(G):
    pkg, gpu = G.pkg, G.gpu()
    s = stmt(G)
    L, p = gpu.L, s.p
    ts = CountingTranscript(pkg)
    good = [(0, 1, 1), (2, NW - 1, 1)]
    h32 = bytes(32)
    b3 = np.zeros((3, 4), dtype=np.uint64)
    for bad in ([(3, 1, 1)], good + [(0, NW, 1)], [(1 << 40, 0, 1)]):  # c >= nl, w >= nw
        with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
            s.pr.prove(ts, 3, lm.records(bad), h32, s.lqc)
        with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
            pkg.ligero_verify256(gpu, p, s.root, b"\x00" * 64, ts, 3, lm.records(bad), h32, b3, s.lqc)
    bad_lqc = list(s.lqc)
    bad_lqc[-1] = (bad_lqc[-1][0], NW, bad_lqc[-1][2])
    with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
        s.pr.prove(ts, 3, lm.records(good), h32, bad_lqc)
    with pytest.raises(pkg.LfGpuError, match="lfgpu error 1:"):
        pkg.ligero_verify256(gpu, p, s.root, b"\x00" * 64, ts, 3, lm.records(good), h32, b3, bad_lqc)
    # NULL arguments and the summand bound, straight at the C ABI
    ll = lm.records(good)
    lq = np.ascontiguousarray(np.asarray(s.lqc, dtype=np.uint64).reshape(-1))
    ops, n = ts.ops(), C.c_size_t()

    def vp(a):
        return C.c_void_p(a.ctypes.data)

    pa = [s.pr.h, C.byref(ops), 3, 2, vp(ll), h32, vp(lq), None, 0, C.byref(n)]
    for i in (0, 1, 4, 5, 6, 9):
        a = list(pa)
        a[i] = None
        assert L.lfgpu_ligero_prove256(*a) == ERR_ARG, i
    for nterm in (1 << 32, (1 << 32) - 6 * NQ):  # nllterm + 6 nq >= 2^32 (refused before the list is read)
        a = list(pa)
        a[3] = nterm
        assert L.lfgpu_ligero_prove256(*a) == ERR_ARG
    ok, why = C.c_int(), C.c_char_p()
    va = [gpu.h, C.byref(p), s.root, b"\x00" * 64, 64, C.byref(ops), 3, 2, vp(ll), h32, vp(b3), vp(lq), C.byref(ok), C.byref(why)]
    for i in (0, 1, 2, 3, 5, 8, 9, 10, 11, 12):
        a = list(va)
        a[i] = None
        assert L.lfgpu_ligero_verify256(*a) == ERR_ARG, i
    a = list(va)
    a[7] = 1 << 32
    assert L.lfgpu_ligero_verify256(*a) == ERR_ARG
    # a transcript without the sized element writes
    bare = CountingTranscript(pkg, sized=False)
    bops = bare.ops()
    a = list(pa)
    a[1] = C.byref(bops)
    assert L.lfgpu_ligero_prove256(*a) == ERR_ARG
    a = list(va)
    a[5] = C.byref(bops)
    assert L.lfgpu_ligero_verify256(*a) == ERR_ARG
    assert ts.calls == 0 and bare.calls == 0, "a refused call touched the transcript"


def test_provers_and_entry_points_of_the_other_width(G):
    """prove256 on a GF(2^128) prover, lfgpu_ligero_prove on a P-256 prover, and a P-256 prover or field at every Ligero entry point
    that serves the 16-byte fields only: refused on the host with the documented code"""
    pkg, gpu = G.pkg, G.gpu()
    par = importlib.import_module(pkg.__name__ + ".parallel")
    s = stmt(G)
    L, p = gpu.L, s.p
    ts = CountingTranscript(pkg)
    ops, n = ts.ops(), C.c_size_t()
    h32 = bytes(32)
    lq = np.ascontiguousarray(np.asarray(s.lqc, dtype=np.uint64).reshape(-1))

    def vp(a):
        return C.c_void_p(a.ctypes.data)

    # a GF(2^128) prover at prove256
    pg = pkg.ligero_param(pkg.FIELD_GF2_128, 100, 0, 4, 6, 128)
    eng = np.random.default_rng(1)
    gf = pkg.LigeroProver(gpu, pkg.FIELD_GF2_128, pg)
    gf.commit(np.zeros((100, 2), dtype=np.uint64), 0, [], lambda k: bytes(eng.integers(0, 256, size=k, dtype=np.uint8)))
    ll256 = lm.records([(0, 1, 1)])
    assert L.lfgpu_ligero_prove256(gf.h, C.byref(ops), 1, 1, vp(ll256), h32, None, None, 0, C.byref(n)) == ERR_ARG
    gf.close()
    # the P-256 prover at the 16-byte entry points
    ll16 = np.zeros(1, dtype=pkg.LLTERM_DTYPE)
    assert L.lfgpu_ligero_prove(s.pr.h, C.byref(ops), 1, 1, vp(ll16), h32, vp(lq), None, 0, C.byref(n)) == ERR_ARG
    y = np.zeros((p.dblock, 4), dtype=np.uint64)
    assert L.lfgpu_ligero_dot_proof_sparse(s.pr.h, None, 0, None, None, None, 0, vp(y)) == ERR_ARG
    hs = (C.c_void_p * 1)(s.pr.h.value)
    z = np.zeros(4 * (p.nwqrow + p.block + 2 * p.dblock + p.nrow * p.nreq + 64), dtype=np.uint64)
    nsp = (C.c_size_t * 1)(0)
    nul = (C.c_void_p * 1)(None)
    assert L.lfgpu_ligero_prove_batch(gpu.h, hs, 1, vp(z), nul, 0, None, nul, nul, nsp, vp(z), vp(z), vp(z), vp(z), vp(z)) == ERR_UNSUPPORTED
    idx = (C.c_size_t * p.nreq)(*range(p.nreq))
    npath = (C.c_size_t * 1)()
    path = np.zeros((p.nreq * p.mc_pathlen + 1, 32), dtype=np.uint8)
    assert L.lfgpu_ligero_open_batch(gpu.h, hs, 1, idx, vp(z), vp(z), vp(path), len(path), npath) == ERR_UNSUPPORTED
    # the field at the entry points that take one
    P256 = pkg.FIELD_P256
    W = lm.elts(s.W)
    rng_fn = pkg.RNG_FN(lambda _u, buf, k: C.memset(buf, 0, k))
    out = (C.c_void_p * 1)()
    roots = (C.c_uint8 * 32)()
    Ws = (C.c_void_p * 1)(W.ctypes.data)
    assert L.lfgpu_ligero_commit_batch(gpu.h, P256, 0, C.byref(p), 1, Ws, 0, vp(lq), (pkg.RNG_FN * 1)(rng_fn), None, roots, out) == ERR_ARG
    one = par.CommOps(None, 0, 1, par.AG_FN(lambda *a: 1), par.A2A_FN(lambda *a: 1), par.BC_FN(lambda *a: 1))  # complete, world = 1
    h = C.c_void_p()
    assert L.lfgpu_ligero_commit_sharded(gpu.h, P256, 0, C.byref(p), vp(W), 0, vp(lq), rng_fn, None, C.byref(one), roots, C.byref(h)) == ERR_ARG
    rows = np.zeros((p.nrow, p.dblock, 4), dtype=np.uint64)
    assert L.lfgpu_ligero_layout_rows_sharded(P256, 0, C.byref(p), vp(W), 0, vp(lq), rng_fn, None, C.byref(one), vp(rows), None) == ERR_ARG
    assert L.lfgpu_ligero_encode_rows(gpu.h, P256, 0, C.byref(p), 0, p.nrow, vp(rows), C.c_void_p(s.pr.tableau_ptr())) == ERR_ARG
    assert L.lfgpu_ligero_prover_from_slab(gpu.h, P256, 0, C.byref(p), 0, p.nrow, C.c_void_p(s.pr.tableau_ptr()), None, None, C.byref(h)) == ERR_ARG
    sc = (C.c_uint64 * 2)(1, 0)
    assert L.lfgpu_ligero_inner_product_rows(gpu.h, P256, p.w, p.r, p.dblock, p.nwqrow, None, 0, sc, None, None, 0,
                                             C.c_void_p(s.pr.tableau_ptr())) == ERR_UNSUPPORTED
    ok, why = C.c_int(), C.c_char_p()
    assert L.lfgpu_ligero_verify(gpu.h, P256, 0, C.byref(p), s.root, b"\x00" * 64, 64, C.byref(ops), 1, 1, vp(ll16), h32, vp(z), vp(lq), C.byref(ok),
                                 C.byref(why)) == ERR_ARG
    assert ts.calls == 0
    # and the prover is none the worse for it
    got = np.zeros((p.nrow, p.block_enc, 4), dtype=np.uint64)
    gpu.memcpy_d2h(got, s.pr.tableau_ptr())
    assert (got == s.T).all()


def test_close_statements(G):
    """(last) the module's committed provers go back to the pool"""
    for s in _stmts.values():
        s.close()
    _stmts.clear()

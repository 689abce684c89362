"""What the Ligero prove/verify suites share (test_ligero_prove_verify.py, test_verifier_checks.py): field elements as Python
ints through the oracle, write_com_proof restated, and Statement -- a committed prover over a random witness with its linear
and quadratic constraints, proved and verified through lfgpu_ligero_prove / lfgpu_ligero_verify or through the single calls."""
import numpy as np

import oracle_lib as ol
from fs_transcript import Transcript
from oracle_lib import FP, GF, arr, elt

M64 = (1 << 64) - 1
FP_P = 2**128 - 2**108 + 1
LLTERM = [("c", "<u8"), ("w", "<u8"), ("k", "<u8", (2,))]


# ---------------------------------------------------------------- field elements as Python ints (the 128-bit Elt image)
def _a2i(a):
    return int(a[0]) | int(a[1]) << 64


def _i2a(x):
    return np.array([x & M64, x >> 64], dtype=np.uint64)


def _ints(a):
    return [_a2i(e) for e in np.asarray(a).reshape(-1, 2)]


def _elts(xs):
    return np.ascontiguousarray(np.array([[x & M64, x >> 64] for x in xs], dtype=np.uint64).reshape(-1, 2))


def fmul(field, a, b):
    return _a2i(arr(ol.oracle().lfo_mul(field, elt(_i2a(a)), elt(_i2a(b)))))


def fadd(field, a, b):
    return _a2i(arr(ol.oracle().lfo_add(field, elt(_i2a(a)), elt(_i2a(b)))))


def fneg(field, a):
    return a if field == GF else (FP_P - a) % FP_P


def to_bytes(field, x):
    """to_bytes_field: GF(2^128) the image itself, Fp128 the canonical value of the Montgomery image"""
    if field == FP:
        x = (x * pow(1 << 128, -1, FP_P)) % FP_P
    return x.to_bytes(16, "little")


def draw(ts, field):
    """Field::sample on the transcript's PRF: 16 bytes, Fp128 rejects >= p and stores the Montgomery image"""
    while True:
        x = int.from_bytes(ts.bytes(16), "little")
        if field == GF:
            return x
        if x < FP_P:
            return (x << 128) % FP_P


def _beta():
    beta = ol.gf_ctx(4).beta
    return [int(beta[i].l[0]) | int(beta[i].l[1]) << 64 for i in range(16)]


_ECHELON = None


def gf_in_subfield(x):
    """(does x lie in GF2_128<4>'s 16-bit subfield?, its coordinates over beta)"""
    global _ECHELON
    if _ECHELON is None:
        rows = []
        for i, v in enumerate(_beta()):
            comb = 1 << i
            for (pv, pc, pb) in rows:
                if (v >> pb) & 1:
                    v, comb = v ^ pv, comb ^ pc
            rows.append((v, comb, v.bit_length() - 1))
        _ECHELON = rows
    u = 0
    for (pv, pc, pb) in _ECHELON:
        if (x >> pb) & 1:
            x, u = x ^ pv, u ^ pc
    return x == 0, u


def gf_of_scalar(u):
    v = 0
    for i, bv in enumerate(_beta()):
        if (u >> i) & 1:
            v ^= bv
    return v


def com_proof_bytes(field, y_ldt, y_dot, y_q0, y_q2, req, nonces, path):
    """write_com_proof (lib/zk/zk_proof.h:137-185) restated: y vectors, nonces, run-length coded opened columns, the Merkle path"""
    out = bytearray()
    for y in (y_ldt, y_dot, y_q0, y_q2):
        for x in _ints(y):
            out += to_bytes(field, x)
    out += np.ascontiguousarray(nonces).tobytes()
    xs = _ints(req)
    if field == FP:  # every element lies in the subfield and is sent at full width: an empty full-field run first
        runs = [(False, []), (True, xs)]
    else:
        runs, sub, cur = [], False, []
        for x in xs:
            ins = gf_in_subfield(x)[0]
            while ins != sub:
                runs.append((sub, cur))
                cur, sub = [], not sub
            cur.append(x)
        runs.append((sub, cur))
    for sub, items in runs:
        out += len(items).to_bytes(4, "little")
        for x in items:
            out += gf_in_subfield(x)[1].to_bytes(2, "little") if (sub and field == GF) else to_bytes(field, x)
    out += len(path).to_bytes(4, "little")
    for d in path:
        out += bytes(d)
    return bytes(out)


def records(terms):
    """[(c, w, k as int)] -> lfgpu_ligero_llterm records"""
    ll = np.zeros(len(terms), dtype=LLTERM)
    for i, (c, w, k) in enumerate(terms):
        ll[i] = (c, w, (k & M64, k >> 64))
    return ll


def rand_terms(rng, field, n, nl, nw):
    ks = _ints(ol.rand_elts(rng, n, field))
    return [(int(rng.integers(0, nl)), int(rng.integers(0, nw)), ks[i]) for i in range(n)]


# ---------------------------------------------------------------- statements
class Statement:
    """a committed prover over a random witness that satisfies nq quadratic constraints -- all but those listed in `violate`,
    whose W[z] is off by one (the prover does not check the witness).  subfield_log_bits = 5: GF2_128<5>, and then no
    subfield_boundary (com_proof_bytes knows the 16-bit subfield only).

    prove / verify / expected run under the library's FsTranscript(seed), or under the transcript `ts` where one is given (an
    object with fs_transcript.Transcript's methods and .ops(), such as scripted_transcript.ScriptedTranscript)."""

    def __init__(self, G, field, nw, nq, nreq, be, seed, subfield_boundary=0, subfield_log_bits=4, violate=()):
        pkg, o = G.pkg, ol.oracle()
        rng = np.random.default_rng(seed)
        assert subfield_log_bits == 4 or (field == GF and subfield_boundary == 0)
        self.G, self.field, self.k = G, field, subfield_log_bits
        self.p = pkg.ligero_param(field, nw, nq, 4, nreq, be, subfield_log_bits=subfield_log_bits)
        W = ol.rand_elts(rng, nw, field)
        for i in range(subfield_boundary):
            W[i] = _i2a(gf_of_scalar(int(rng.integers(0, 1 << 16))))
        self.lqc = []
        zs = rng.choice(np.arange(nw // 2, nw), size=nq, replace=False) if nq else []
        for i in range(nq):
            x, y, z = int(rng.integers(0, nw // 2)), int(rng.integers(0, nw // 2)), int(zs[i])
            W[z] = arr(o.lfo_mul(field, elt(W[x]), elt(W[y])))
            self.lqc.append((x, y, z))
        for i in violate:  # z lies in the upper half of the witness and is no one's x or y: only constraint i breaks
            z = self.lqc[i][2]
            W[z] = _i2a(fadd(field, _a2i(W[z]), 1))
        self.W = _ints(W)
        eng = np.random.default_rng(seed + 1)
        self.pr = pkg.LigeroProver(G.gpu(), field, self.p, subfield_log_bits=subfield_log_bits)
        self.root = self.pr.commit(W, subfield_boundary, self.lqc, lambda n: bytes(eng.integers(0, 256, size=n, dtype=np.uint8)))

    def b_of(self, nl, terms):
        """b = A W for the linear terms (c, w, k)"""
        b = [0] * nl
        for (c, w, k) in terms:
            b[c] = fadd(self.field, b[c], fmul(self.field, k, self.W[w]))
        return b

    def expected(self, nl, terms, hash32, seed=b"ligero", ts=None):
        """the proof bytes from the existing single calls and the Python transcript -> (bytes, next 32 transcript bytes)"""
        p, field, pr = self.p, self.field, self.pr
        ts = Transcript(seed) if ts is None else ts
        ts.write_bytes(self.root)
        ts.write_bytes(hash32)
        u_ldt = [draw(ts, field) for _ in range(p.nwqrow)]
        y_ldt = pr.low_degree_proof(_elts(u_ldt))
        alphal = [draw(ts, field) for _ in range(nl)]
        alphaq = [draw(ts, field) for _ in range(3 * p.nq)]
        A = [0] * (p.nwqrow * p.w)  # inner_product_vector (ligero_param.h:382-421)
        for (c, w, k) in terms:
            A[w] = fadd(field, A[w], fmul(field, k, alphal[c]))
        base = p.nwrow * p.w
        for iw in range(p.nq):
            for j in range(3):
                aq = alphaq[3 * iw + j]
                pos = base + j * p.nqtriples * p.w + iw
                A[pos] = fadd(field, A[pos], aq)
                A[self.lqc[iw][j]] = fadd(field, A[self.lqc[iw][j]], fneg(field, aq))
        y_dot = pr.dot_proof(_elts(A))
        u_quad = [draw(ts, field) for _ in range(p.nqtriples)]
        y_q0, y_q2 = pr.quadratic_proof(_elts(u_quad))
        for y in (y_ldt, y_dot, y_q0, y_q2):
            ts.write_array([to_bytes(field, x) for x in _ints(y)])
        idx = ts.choose(p.block_ext, p.nreq)
        self.last_u_ldt, self.last_idx = u_ldt, idx
        req, nonces, path = pr.open(idx)
        return com_proof_bytes(field, y_ldt, y_dot, y_q0, y_q2, req, nonces, path), ts.bytes(32)

    def prove(self, nl, ll, hash32, seed=b"ligero", ts=None):
        own = ts is None
        ts = self.G.pkg.FsTranscript(seed) if own else ts
        ts.write_bytes(self.root)
        proof = self.pr.prove(ts, nl, ll, hash32, self.lqc)
        nxt = ts.bytes(32)
        if own:
            ts.close()
        return proof, nxt

    def verify(self, proof, nl, ll, hash32, b, seed=b"ligero", root=None, ts=None):
        root = self.root if root is None else root
        own = ts is None
        ts = self.G.pkg.FsTranscript(seed) if own else ts
        ts.write_bytes(root)
        r = self.G.pkg.ligero_verify(self.G.gpu(), self.field, self.p, root, proof, ts, nl, ll, hash32, _elts(b), self.lqc,
                                     subfield_log_bits=self.k)
        if own:
            ts.close()
        return r

    def check(self, nl, given, folded=None, hash32=bytes(range(32))):
        """prove on the list `given` == the pieces on `folded` (the same sums in fewer terms; default: given itself), the
        transcript ends in the same state, and the verifier accepts"""
        folded = given if folded is None else folded
        want, want_next = self.expected(nl, folded, hash32)
        ll = given if isinstance(given, np.ndarray) else records(given)
        got, got_next = self.prove(nl, ll, hash32)
        o_dot, n_dot = 16 * self.p.block, 16 * self.p.dblock
        assert got[o_dot:o_dot + n_dot] == want[o_dot:o_dot + n_dot], "y_dot differs"
        assert got == want
        assert got_next == want_next, "the transcript was left in another state"
        assert self.verify(got, nl, ll, hash32, self.b_of(nl, folded)) == (True, "ok")
        return got

    def close(self):
        self.pr.close()

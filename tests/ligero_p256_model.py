"""A model of the Ligero prover over Fp256Base in Python integers mod p, with no device: what tests/test_ligero_p256_model.py pins
against the reference's known-answer vector and tests/test_ligero_p256_gpu.py then compares the device with.

Written from LigeroProver::prove / low_degree_proof / dot_proof / quadratic_proof / compute_req (lib/ligero/ligero_prover.h:84-146,
281-351), inner_product_vector + layout_Aext (lib/ligero/ligero_param.h:382-430), MerkleTree (lib/merkle/merkle_tree.h) and
write_com_proof (lib/zk/zk_proof.h:137-185).  The tableau comes from lfgpu_ligero_layout_rows(P256) (host only) extended with the
oracle's lfo_p256_rs_interpolate; the challenges from tests/fs_transcript.py.

Elements are the integers of their Montgomery images (x R mod p, R = 2^256), as the library stores them: sums are plain sums mod
p, a product takes one factor 1 / R, and to_bytes_field is x / R, 32 bytes little-endian."""
import hashlib

import numpy as np

import oracle_lib as ol

P = ol.P256_P
R = 1 << 256
RINV = pow(R, -1, P)
M64 = (1 << 64) - 1
LLTERM256 = [("c", "<u8"), ("w", "<u8"), ("k", "<u8", (4,))]


def mul(a, b):
    return a * b * RINV % P


def a2i(a):
    return int(a[0]) | int(a[1]) << 64 | int(a[2]) << 128 | int(a[3]) << 192


def ints(a):
    return [a2i(e) for e in np.asarray(a).reshape(-1, 4)]


def elts(xs):
    return np.ascontiguousarray(np.array([[(x >> (64 * j)) & M64 for j in range(4)] for x in xs], dtype=np.uint64).reshape(-1, 4))


def of_scalar(u):
    return u * R % P


def to_bytes(x):
    return (x * RINV % P).to_bytes(32, "little")


def draw(ts):
    """FpGeneric::sample on the transcript's PRF: 32 bytes an attempt, rejected when >= p"""
    while True:
        x = int.from_bytes(ts.bytes(32), "little")
        if x < P:
            return x * R % P


def rand_ints(rng, n):
    """n uniform elements (Montgomery images) from a numpy Generator"""
    out = []
    while len(out) < n:
        x = int.from_bytes(rng.bytes(32), "little")
        if x < P:
            out.append(x)
    return out


def records(terms):
    """[(c, w, k as int)] -> lfgpu_ligero_llterm256 records"""
    ll = np.zeros(len(terms), dtype=LLTERM256)
    if len(terms):
        ll["c"] = [t[0] for t in terms]
        ll["w"] = [t[1] for t in terms]
        ll["k"] = elts([t[2] for t in terms])
    return ll


def tableau(pkg, p, W, lqc, rng_bytes):
    """LigeroProver::commit without the device -> (T [nrow][block_enc][4] uint64, nonces [block_ext][32]): the library's host
    layout, every row extended by the oracle (rows IDOT / IQUAD carry dblock values, the others block)"""
    rows, nonces = pkg.ligero_layout_rows(pkg.FIELD_P256, p, W, 0, lqc, rng_bytes)
    o = ol.oracle()
    T = np.zeros((p.nrow, p.block_enc, 4), dtype=np.uint64)
    T[:, :p.dblock] = rows
    for i in range(p.nrow):
        row = np.ascontiguousarray(T[i])
        o.lfo_p256_rs_interpolate(p.dblock if i in (p.idot, p.iquad) else p.block, p.block_enc, ol.P(row))
        T[i] = row
    return T, nonces


def root_of(p, T, nonces):
    """the column commitment of the oracle over columns [dblock, block_enc)"""
    root = np.zeros(32, dtype=np.uint8)
    T = np.ascontiguousarray(T)
    nz = np.ascontiguousarray(nonces)
    ol.oracle().lfo_column_commit32(p.nrow, p.block_enc, p.dblock, p.block_ext, ol.P(T), ol.P(nz), ol.P(root), None)
    return bytes(root)


class Model:
    def __init__(self, p, T, nonces, lqc):
        self.p, self.lqc = p, [tuple(int(x) for x in q) for q in lqc]
        self.T = [ints(T[i]) for i in range(p.nrow)]
        self.nonces = [bytes(nonces[i]) for i in range(p.block_ext)]
        self._layers = None

    # ---- the three row combinations
    def low_degree(self, u):
        p, T = self.p, self.T
        return [(T[p.ildt][j] + sum(mul(u[i], T[p.iw + i][j]) for i in range(p.nwqrow))) % P for j in range(p.block)]

    def inner_product_vector(self, nl, terms, alphal, alphaq):
        """A[w] += k alphal[c]; the copy constraints A[base + j nqtriples w + iw] += aq, A[lqc[iw][j]] -= aq (:382-421)"""
        p = self.p
        A = [0] * (p.nwqrow * p.w)
        for (c, w, k) in terms:
            assert c < nl
            A[w] = (A[w] + mul(k, alphal[c])) % P
        base = p.nwrow * p.w
        for iw in range(p.nq):
            for j in range(3):
                aq = alphaq[3 * iw + j]
                pos = base + j * p.nqtriples * p.w + iw
                A[pos] = (A[pos] + aq) % P
                A[self.lqc[iw][j]] = (A[self.lqc[iw][j]] - aq) % P
        return A

    def dot(self, A):
        p, T = self.p, self.T
        o = ol.oracle()
        y = list(T[p.idot][:p.dblock])
        for i in range(p.nwqrow):
            row = elts([0] * p.r + A[i * p.w:(i + 1) * p.w] + [0] * (p.dblock - p.block))  # layout_Aext, then block -> dblock
            o.lfo_p256_rs_interpolate(p.block, p.dblock, ol.P(row))
            a = ints(row)
            for j in range(p.dblock):
                y[j] = (y[j] + mul(a[j], T[p.iw + i][j])) % P
        return y

    def quadratic(self, u):
        p, T = self.p, self.T
        y = list(T[p.iquad][:p.dblock])
        nt = p.nqtriples
        for i in range(nt):
            X, Y, Z = T[p.iq + i], T[p.iq + nt + i], T[p.iq + 2 * nt + i]
            for j in range(p.dblock):
                y[j] = (y[j] + mul(u[i], (Z[j] - mul(X[j], Y[j])) % P)) % P
        assert not any(y[p.r:p.block]), "the W part of y_quad is non-zero"
        return y[:p.r], y[p.block:]

    # ---- the opening
    def layers(self):
        if self._layers is None:
            p, T = self.p, self.T
            n = p.block_ext
            L = [b""] * (2 * n)
            for j in range(n):
                h = hashlib.sha256(self.nonces[j])
                for i in range(p.nrow):
                    h.update(to_bytes(T[i][p.dblock + j]))
                L[n + j] = h.digest()
            for i in range(n - 1, 0, -1):
                L[i] = hashlib.sha256(L[2 * i] + L[2 * i + 1]).digest()
            self._layers = L
        return self._layers

    def root(self):
        return self.layers()[1]

    def open(self, idx):
        """-> (req [nrow][nreq], the nonces of the opened leaves, MerkleTree::generate_compressed_proof)"""
        p = self.p
        n, L = p.block_ext, self.layers()
        req = [[self.T[i][p.dblock + j] for j in idx] for i in range(p.nrow)]
        mark = [False] * (2 * n)
        for j in idx:
            mark[n + j] = True
        for i in range(n - 1, 0, -1):
            mark[i] = mark[2 * i] or mark[2 * i + 1]
        path = []
        for i in range(n - 1, 0, -1):
            if mark[i]:
                child = 2 * i
                if mark[child]:
                    child = 2 * i + 1
                if not mark[child]:
                    path.append(L[child])
        return req, [self.nonces[j] for j in idx], path

    # ---- LigeroProver::prove and write_com_proof
    def prove(self, ts, nl, terms, hash32):
        """ts: a fs_transcript.Transcript that holds the root -> the write_com_proof bytes; the pieces stay in self.last"""
        p = self.p
        ts.write_bytes(hash32)
        u_ldt = [draw(ts) for _ in range(p.nwqrow)]
        y_ldt = self.low_degree(u_ldt)
        alphal = [draw(ts) for _ in range(nl)]
        alphaq = [draw(ts) for _ in range(3 * p.nq)]
        A = self.inner_product_vector(nl, terms, alphal, alphaq)
        y_dot = self.dot(A)
        u_quad = [draw(ts) for _ in range(p.nqtriples)]
        y_q0, y_q2 = self.quadratic(u_quad)
        for y in (y_ldt, y_dot, y_q0, y_q2):
            ts.write_array([to_bytes(x) for x in y])
        idx = ts.choose(p.block_ext, p.nreq)
        req, nonces, path = self.open(idx)
        self.last = dict(u_ldt=u_ldt, alphal=alphal, alphaq=alphaq, A=A, u_quad=u_quad, idx=idx, y_ldt=y_ldt, y_dot=y_dot, y_q0=y_q0, y_q2=y_q2, req=req,
                         nonces=nonces, path=path)
        return com_proof_bytes(y_ldt, y_dot, y_q0, y_q2, req, nonces, path)


def com_proof_bytes(y_ldt, y_dot, y_q0, y_q2, req, nonces, path):
    """write_com_proof for a prime field: every element lies in the subfield and goes at full width, so the opened columns are
    an empty full-field run and one subfield run"""
    out = bytearray()
    for y in (y_ldt, y_dot, y_q0, y_q2):
        for x in y:
            out += to_bytes(x)
    for nz in nonces:
        out += bytes(nz)
    flat = [x for row in req for x in row]
    out += (0).to_bytes(4, "little")
    out += len(flat).to_bytes(4, "little")
    for x in flat:
        out += to_bytes(x)
    out += len(path).to_bytes(4, "little")
    for d in path:
        out += bytes(d)
    return bytes(out)

"""Every check of the Ligero verifier (zkp::ligero_verify, csrc/zk_proto.h) as the check that refuses.

Under the real SHA/AES transcript a tampered proof byte moves every later challenge, the opened columns included, so whatever
is flipped the Merkle check refuses first and the low-degree, dot and quadratic checks are never the ones that find the
fault.  Here the transcript is tests/scripted_transcript.py, whose challenges depend on the SHAPE of what is written and not on
its content: a tampered copy of an honest proof is checked under the honest proof's challenges and opened columns, the Merkle
check passes, and the check that owns the tampered section has to refuse -- with exactly its reason.

A change of ONE element of a y vector is always caught, whatever columns are opened: it adds a non-zero multiple of one Lagrange
basis polynomial over the vector's own evaluation points, whose roots are all the other points of the vector, so it is non-zero at
every extension column.  No escape probability is budgeted anywhere below.

Ligero level (lfgpu_ligero_prove / lfgpu_ligero_verify: GF2_128<4>, GF2_128<5>, Fp128): 700 wires, 150 quadratic constraints in
three triple rows, the last one partial (what no synthetic fixture has: nqtriples is 1 everywhere else).
ZK level (lfgpu_zk_prove / lfgpu_zk_verify and lfgpu_zk_verify_committed: GF(2^128), Fp128, Fp256Base -- the last with device
code of its own, csrc/zk256.hip): the `funnel` circuits of the three synthetic suites.

The attack the quadratic check exists for -- a commitment to a witness with one W[z] != W[x] W[y] -- runs under the REAL transcript.
The library's own prover refuses such a witness (pinned below), so the commitment and the proof are forged with the CPU oracle, and
the verifier has to answer exactly "quadratic_check failed".

The scripted transcript also reaches what the real one does not within a test's life: the rejection branch of elt_sample / h256_sample
(a draw >= p: 2^-20 per Fp128 draw, 2^-32 per P-256 draw) by splicing such a draw into the stream, and column 0 opened together
with column block_ext - 1 by replacing the first two draws of choose."""
import json
import lzma
import os

import numpy as np
import pytest

import ligero_statement as ls
from ligero_statement import FP_P, Statement, _elts, _ints, draw, rand_terms, records, to_bytes
from oracle_lib import FP, GF
from scripted_transcript import ScriptedTranscript

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P256 = 2**256 - 2**224 + 2**192 + 2**96 - 1
MERKLE, LOW_DEGREE, DOT, DOT_VALUE, QUADRATIC = ("merkle_check failed", "low_degree_check failed", "dot_check failed", "wrong dot product",
                                                 "quadratic_check failed")


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def nat_len(n):
    """the bytes RandomEngine::nat draws for a bound n"""
    return (n.bit_length() + 7) // 8


def flip_low_bit(d, off, nbytes, modulus):
    """the element at `off` with the low bit of its low wire byte flipped; the copy must still parse (a prime field refuses an
    image >= p with "proof does not parse", which would say nothing about the checks)"""
    d = bytearray(d)
    d[off] ^= 1
    assert modulus is None or int.from_bytes(d[off:off + nbytes], "little") < modulus, "pick another position: the image is no element"
    return bytes(d)


def flip_byte(d, off):
    d = bytearray(d)
    d[off] ^= 1
    return bytes(d)


def challenge_epoch(eps):
    """the epoch opened by the 32-byte hash_of_A write, the last 32-byte write_bytes of a proof: it holds the u_ldt, alphal, alphaq
    and u_quad draws"""
    e = [x for x in eps if x["write"] == (0, 32)][-1]
    assert e["draws"]
    return e


def choose_epoch(eps):
    """the last epoch with draws: the one after the y_quad_2 write"""
    e = [x for x in eps if x["draws"]][-1]
    assert e["write"][0] == 2
    return e


def y_offsets(p, B, base=0):
    """byte offsets of the sections of write_com_proof from the parameters: y_ldt, y_dot, y_quad_0, y_quad_2, the nonces, the
    opened columns"""
    o = dict(y_ldt=base, y_dot=base + B * p.block, y_q0=base + B * (p.block + p.dblock))
    o["y_q2"] = o["y_q0"] + B * p.r
    o["nonces"] = o["y_q2"] + B * (p.dblock - p.block)
    o["req"] = o["nonces"] + 32 * p.nreq
    return o


def y_cases(p, B, o):
    """(what, offset, expected reason): one element of every y vector at its edges and at the seams of its parts"""
    assert p.block == p.r + p.w and p.dblock == 2 * p.block - 1 and p.r >= 2
    cases = [("y_ldt[%d]" % i, o["y_ldt"] + B * i, LOW_DEGREE) for i in (0, p.r - 1, p.r, p.block - 1)]
    cases += [("y_dot[%d]" % i, o["y_dot"] + B * i, DOT) for i in (0, p.r, p.r + p.w - 1, p.r + p.w, p.dblock - 1)]
    cases += [("y_q0[%d]" % i, o["y_q0"] + B * i, QUADRATIC) for i in (0, p.r - 1)]
    cases += [("y_q2[%d]" % i, o["y_q2"] + B * i, QUADRATIC) for i in (0, p.dblock - p.block - 1)]
    return cases


# ================================================================ Ligero level
NW, NQ, NREQ, BE, NL = 700, 150, 12, 512, 9
HASH32 = bytes(range(32))
LIGERO = {"gf_k4": (GF, 4), "gf_k5": (GF, 5), "fp128": (FP, 4)}
SEED = 20


class LigeroCase:
    """a statement, its honest proof under ScriptedTranscript(SEED) and the prover's log"""

    def __init__(self, G, variant, violate=()):
        self.field, self.k = LIGERO[variant]
        rng = np.random.default_rng(1 + self.k + self.field)
        # GF2_128<4>: the first witness row holds subfield elements, so the opening has two-byte runs
        self.s = Statement(G, self.field, NW, NQ, NREQ, BE, seed=500 + self.field + self.k, subfield_boundary=73 if (self.field, self.k) == (GF, 4) else 0,
                           subfield_log_bits=self.k, violate=violate)
        p = self.p = self.s.p
        assert p.nqtriples == 3 and 150 % p.w != 0 and p.nq == NQ
        self.terms = rand_terms(rng, self.field, 150, NL, NW)
        self.ll = records(self.terms)
        self.b = self.s.b_of(NL, self.terms)
        self.modulus = FP_P if self.field == FP else None
        self.o = y_offsets(p, 16)
        # row 0 (the low-degree blinding row, never in the subfield) of opened column j: behind the length of the first run, and
        # for Fp128 behind the empty full-field run in front of it
        self.o_col = self.o["req"] + (8 if self.field == FP else 4)
        if violate:
            return
        ts = ScriptedTranscript(SEED)
        self.proof, _ = self.s.prove(NL, self.ll, HASH32, ts=ts)
        ts.check()
        self.eps = ts.epochs()
        self.n_draws = p.nwqrow + NL + 3 * p.nq + p.nqtriples
        assert challenge_epoch(self.eps)["draws"].count(16) >= self.n_draws
        if self.field == GF:  # no rejection in this field: the draws are exactly the challenges
            assert challenge_epoch(self.eps)["draws"] == [16] * self.n_draws

    def scripted(self, script=()):
        ts = ScriptedTranscript(SEED)
        for kind, epoch, at, data in script:
            getattr(ts, kind)(epoch, at, data)
        return ts

    def verify(self, proof, b=None, root=None, script=(), ts=None):
        ts = self.scripted(script) if ts is None else ts
        r = self.s.verify(proof, NL, self.ll, HASH32, self.b if b is None else b, root=root, ts=ts)
        ts.check()
        return r

    def prove(self, script=()):
        ts = self.scripted(script)
        proof, nxt = self.s.prove(NL, self.ll, HASH32, ts=ts)
        ts.check()
        return proof, nxt, ts


_ligero = {}


@pytest.fixture(params=sorted(LIGERO))
def lig(G, request):
    if request.param not in _ligero:
        _ligero[request.param] = LigeroCase(G, request.param)
    return _ligero[request.param]


def test_ligero_each_check_refuses(lig):
    p, d, o = lig.p, lig.proof, lig.o
    assert lig.verify(d) == (True, "ok")
    assert len(d) > o["req"] + 16 * p.nreq * 3
    for what, off, why in y_cases(p, 16, o):
        assert lig.verify(flip_low_bit(d, off, 16, lig.modulus)) == (False, why), what
    # the sum of the w middle entries of y_dot is the dot VALUE; the dot CHECK must catch a change that leaves the sum alone
    e = 1
    at = [o["y_dot"] + 16 * (p.r + i) for i in (0, 1)]
    v = [int.from_bytes(d[a:a + 16], "little") for a in at]
    v = [v[0] ^ e, v[1] ^ e] if lig.field == GF else [(v[0] + e) % FP_P, (v[1] - e) % FP_P]
    bad = bytearray(d)
    for a, x in zip(at, v):
        bad[a:a + 16] = x.to_bytes(16, "little")
    assert bytes(bad) != d
    assert lig.verify(bytes(bad)) == (False, DOT), "+e, -e in y_dot"
    # the right-hand side: A and the proof untouched, only the value of the inner product is wrong
    for k in (0, NL - 1):
        b = list(lig.b)
        b[k] = ls.fadd(lig.field, b[k], 1)
        assert lig.verify(d, b=b) == (False, DOT_VALUE), k
    # the commitment: the root, a nonce, an element of an opened column, a digest of the path
    assert lig.verify(d, root=flip_byte(lig.s.root, 9)) == (False, MERKLE)
    for what, off in (("nonce", o["nonces"] + 32 * 3 + 1), ("last nonce", o["nonces"] + 32 * p.nreq - 1), ("last path digest", len(d) - 32 + 7),
                      ("a path digest before it", len(d) - 32 * 5)):
        assert lig.verify(flip_byte(d, off)) == (False, MERKLE), what
    for j in (0, p.nreq - 1):
        assert lig.verify(flip_low_bit(d, lig.o_col + 16 * j, 16, lig.modulus)) == (False, MERKLE), j


WHERE = {"first_row": 0, "last_partial_row": NQ - 1}


@pytest.mark.parametrize("variant", sorted(LIGERO))
@pytest.mark.parametrize("where", sorted(WHERE))
def test_ligero_honest_prover_refuses_a_dishonest_witness(G, variant, where):
    """One W[z] != W[x] W[y] does not get through the library's prover: the layout of lfgpu_ligero_commit makes the reference's
    check (ligero_prover.h:259-260) on every quadratic constraint, in the last, partial triple row too."""
    with pytest.raises(G.pkg.LfGpuError, match=r"lfgpu error 5: ligero_commit: invalid quadratic constraints"):
        LigeroCase(G, variant, violate=[WHERE[where]])


def forge(c, violate):
    """The adversary the quadratic check exists for, with a prover of its own (the library's refuses, above, and its
    quadratic_proof refuses a non-zero W part as well): the honest tableau is read back, W[z] of every constraint in `violate` is
    raised by one in its witness row AND in its copy in the Qz row (so that every linear constraint, the copy constraints included,
    still holds for b = A W'), both rows are Reed-Solomon encoded again and the columns committed again, all by the CPU oracle;
    the proof then comes from the oracle's row combinations (sharded_util.OracleSlabProver, which keeps no check of y_quad's W part
    and so drops its non-zero entries, as the attack has it) under the real transcript, restated in Python.
    -> a Statement whose prover, root and W are the forged ones"""
    import copy
    import ctypes as C

    import torch

    import oracle_lib as ol
    from oracle_lib import P
    from sharded_util import OracleSlabProver, _rs
    s, p, field = c.s, c.p, c.field
    gpu = s.G.gpu()
    T = np.zeros((p.nrow, p.block_enc, 2), dtype=np.uint64)
    gpu._ck(gpu.L.lfgpu_memcpy_d2h(gpu.h, C.c_void_p(T.ctypes.data), C.c_void_p(s.pr.tableau_ptr()), T.nbytes))

    def encode(row, col=None):
        m = np.zeros((p.block_enc, 2), dtype=np.uint64)
        m[:p.block] = T[row, :p.block]
        if col is not None:
            m[col] = ls._i2a(ls.fadd(field, ls._a2i(m[col]), 1))
        _rs(field, p.block, p.block_enc, m, c.k)
        return m

    for row in (p.ildt, p.iw, p.iw + p.nwrow - 1, p.nrow - 1):  # the adversary's encoder is the tableau's
        assert (encode(row) == T[row]).all(), row
    W = list(s.W)
    iqz = p.iq + 2 * p.nqtriples
    for i in violate:
        x, y, z = s.lqc[i]
        wrow, wcol, qrow, qcol = p.iw + z // p.w, p.r + z % p.w, iqz + i // p.w, p.r + i % p.w
        assert ls._a2i(T[wrow, wcol]) == ls._a2i(T[qrow, qcol]) == W[z] == ls.fmul(field, W[x], W[y])
        T[wrow], T[qrow] = encode(wrow, wcol), encode(qrow, qcol)
        W[z] = ls.fadd(field, W[z], 1)
        assert ls._a2i(T[wrow, wcol]) == ls._a2i(T[qrow, qcol]) == W[z]
    nonces = np.random.default_rng(4).integers(0, 256, size=(p.block_ext, 32), dtype=np.uint8)
    layers = np.zeros((2 * p.block_ext, 32), dtype=np.uint8)
    root = np.zeros(32, dtype=np.uint8)
    ol.oracle().lfo_column_commit(field, p.nrow, p.block_enc, p.dblock, p.block_ext, P(T), P(nonces), P(root), P(layers))
    f = copy.copy(s)
    f.pr = OracleSlabProver(field, p, 0, p.nrow, torch.from_numpy(T.view(np.uint8).reshape(p.nrow, p.block_enc * 16)), torch.from_numpy(layers),
                            nonces.tobytes(), c.k)
    f.root, f.W = bytes(root), W
    return f


@pytest.mark.parametrize("where", ["nowhere"] + sorted(WHERE))
def test_ligero_dishonest_witness_real_transcript(lig, where):
    """A commitment to a W in which one W[z] != W[x] W[y] (forge, above), b = A W for that W, a proof made without the prover's
    own guards, the library's SHA/AES transcript: everything is consistent but one quadratic constraint, so the Merkle,
    low-degree and dot checks and the dot value pass and the quadratic check refuses.  (The w middle entries of y_quad are non-zero
    now; they are not sent and the verifier pads with zeros.)  `nowhere` is the control: the forger's tools with nothing
    violated give a proof that is accepted."""
    violate = [] if where == "nowhere" else [WHERE[where]]
    assert (NQ - 1) // lig.p.w == lig.p.nqtriples - 1 and NQ % lig.p.w != 0
    f = forge(lig, violate)
    for i in violate:
        x, y, z = f.lqc[i]
        assert f.W[z] != ls.fmul(lig.field, f.W[x], f.W[y])
    if not violate:  # on the honest tableau the forger's row combinations (the CPU oracle) are the device's, three triple rows included
        import oracle_lib as ol
        rng, p = np.random.default_rng(8), lig.p
        u, A, uq = (ol.rand_elts(rng, n, lig.field) for n in (p.nwqrow, p.nwqrow * p.w, p.nqtriples))
        assert (f.pr.low_degree_proof(u) == lig.s.pr.low_degree_proof(u)).all()
        assert (f.pr.dot_proof(A) == lig.s.pr.dot_proof(A)).all()
        for got, want in zip(lig.s.pr.quadratic_proof(uq), f.pr.quadratic_proof(uq)):
            assert (got == want).all()
    proof, _ = f.expected(NL, lig.terms, HASH32)
    want = (False, QUADRATIC) if violate else (True, "ok")
    assert f.verify(proof, NL, lig.ll, HASH32, f.b_of(NL, lig.terms)) == want
    assert lig.s.verify(proof, NL, lig.ll, HASH32, lig.b) == (False, MERKLE)  # it is no proof for the honest commitment


def test_ligero_honest_witness_real_transcript(lig):
    """the library's own prover on the same statement under the real transcript: accepted"""
    proof, _ = lig.s.prove(NL, lig.ll, HASH32)
    assert lig.s.verify(proof, NL, lig.ll, HASH32, lig.b) == (True, "ok")


def test_ligero_fp128_rejected_draws(G):
    """draws >= p in front of the first u_ldt, the first alphal, the first alphaq and the last u_quad draw: each costs one more
    16-byte draw on both sides and changes nothing else"""
    c = _ligero.get("fp128") or _ligero.setdefault("fp128", LigeroCase(G, "fp128"))
    p = c.p
    ce = challenge_epoch(c.eps)
    plain = ce["draws"]
    assert plain == [16] * c.n_draws, "the unscripted stream of this seed has a rejected draw of its own: choose another seed"
    ff = b"\xff" * 16
    at = [(0, ff), (p.nwqrow, ff), (p.nwqrow + NL, FP_P.to_bytes(16, "little")), (c.n_draws - 1, ff)]  # p itself is the smallest refused image
    script = [("splice", ce["epoch"], 16 * k, data) for k, data in reversed(at)]  # back to front: the offsets are the plain stream's
    proof, nxt, ts = c.prove(script)
    assert proof == c.proof
    assert challenge_epoch(ts.epochs())["draws"] == [16] * (c.n_draws + len(at))
    assert [e["draws"] for e in ts.epochs() if e["epoch"] != ce["epoch"]] == [e["draws"] for e in c.eps if e["epoch"] != ce["epoch"]]
    tv = c.scripted(script)
    assert c.verify(proof, ts=tv) == (True, "ok")
    assert challenge_epoch(tv.epochs())["draws"] == [16] * (c.n_draws + len(at))
    # one splice alone moves no challenge either
    for k, data in at:
        one = [("splice", ce["epoch"], 16 * k, data)]
        assert c.prove(one)[0] == c.proof, k
        assert c.verify(c.proof, script=one) == (True, "ok"), k


def test_ligero_fp128_largest_accepted_draw(G):
    """p - 1 as the first draw is accepted (the boundary of the rejection test): y_ldt is the low-degree proof for u[0] = the
    Montgomery image of p - 1 and the other u from the stream, and the proof is the one the pieces give"""
    c = _ligero.get("fp128") or _ligero.setdefault("fp128", LigeroCase(G, "fp128"))
    ce = challenge_epoch(c.eps)
    script = [("replace", ce["epoch"], 0, (FP_P - 1).to_bytes(16, "little"))]
    proof, nxt, ts = c.prove(script)
    assert challenge_epoch(ts.epochs())["draws"] == [16] * c.n_draws  # accepted: no further draw
    assert proof != c.proof
    assert c.verify(proof, script=script) == (True, "ok")
    tu = c.scripted(script)
    tu.write_bytes(c.s.root)
    tu.write_bytes(HASH32)
    u = [draw(tu, FP) for _ in range(c.p.nwqrow)]
    assert u[0] == ((FP_P - 1) << 128) % FP_P
    y_ldt = c.s.pr.low_degree_proof(_elts(u))
    assert proof[:16 * c.p.block] == b"".join(to_bytes(FP, x) for x in _ints(y_ldt))
    want, want_next = c.s.expected(NL, c.terms, HASH32, ts=c.scripted(script))
    assert c.s.last_u_ldt == u
    assert (proof, nxt) == (want, want_next)


def test_ligero_edge_columns(lig):
    """choose's first two draws replaced: column 0 and column block_ext - 1 opened together, through prove, the wire and verify"""
    p = lig.p
    n = p.block_ext
    assert nat_len(n) == nat_len(n - 1)
    ln = nat_len(n)
    ch = choose_epoch(lig.eps)
    script = [("replace", ch["epoch"], 0, (0).to_bytes(ln, "little")), ("replace", ch["epoch"], ln, (n - 2).to_bytes(ln, "little"))]
    proof, nxt, ts = lig.prove(script)
    want, want_next = lig.s.expected(NL, lig.terms, HASH32, ts=lig.scripted(script))
    idx = lig.s.last_idx
    assert idx[:2] == [0, n - 1] and len(set(idx)) == p.nreq
    assert (proof, nxt) == (want, want_next)
    o = lig.o
    assert proof[:o["nonces"]] == lig.proof[:o["nonces"]] and proof[o["nonces"]:] != lig.proof[o["nonces"]:]
    assert lig.verify(proof, script=script) == (True, "ok")
    for j in (0, 1):
        assert lig.verify(flip_low_bit(proof, lig.o_col + 16 * j, 16, lig.modulus), script=script) == (False, MERKLE), j
    assert lig.verify(proof) == (False, MERKLE)  # under the plain script other columns are asked for


def test_ligero_close(G):
    """(last of the Ligero level) the committed provers go back to the pool"""
    for c in _ligero.values():
        c.s.close()
    _ligero.clear()


# ================================================================ ZK level
ZK = {"gf": ("synth_gf", 2, None), "fp128": ("synth_fp128", 2, FP_P), "p256": ("synth_p256", 4, P256)}


class ZkCase:
    """the funnel circuit of a field (9 layers, 302 inputs, 6 opened columns), its honest proof under ScriptedTranscript(SEED)
    and the logs of the prover's two lineages"""

    def __init__(self, G, field):
        import ligero_fixture as lf
        stem, words, self.modulus = ZK[field]
        self.G, self.lf = G, lf
        self.B = B = 8 * words
        self.rec = [r for r in json.load(open(os.path.join(GOLD, stem + ".json")))["cases"] if r["case"] == "funnel"][0]
        raw = lzma.decompress(open(os.path.join(GOLD, stem + "_funnel.lfc1.xz"), "rb").read())
        wb = lzma.decompress(open(os.path.join(GOLD, stem + "_funnel.w.xz"), "rb").read())
        self.W = np.frombuffer(wb, dtype=np.uint64).reshape(-1, words).copy()
        self.gpu = G.gpu()
        self.circ = G.pkg.Circuit(self.gpu, raw)
        ci = self.circ.info
        assert (ci.nl, ci.ninputs, ci.npub_in) == (9, 302, 1)
        self.zk = G.pkg.ZkProver(self.gpu, self.circ, self.rec["rate"], self.rec["nreq"], self.rec["block_enc_arg"])
        p = self.p = self.zk.param
        assert (p.nreq, p.block_enc, p.nqtriples) == (6, 128 if field == "gf" else 256, 1)
        self.pub = self.W[:ci.npub_in]
        self.logw = [self.circ.layer(i)["logw"] for i in range(ci.nl)]
        self.o_layer = [32 + B * sum(4 * l + 2 for l in self.logw[:i]) for i in range(ci.nl + 1)]  # a layer: 4 logw round values, then wc[2]
        self.o = y_offsets(p, B, base=self.o_layer[-1])
        self.o_col = self.o["req"] + (4 if field == "gf" else 8)  # as at the Ligero level
        self.wire, ts = self.prove()
        self.eps = ts.epochs()
        (cl,) = ts.clones()
        self.clone_eps = ts.epochs(cl)
        assert len(self.wire) > self.o["req"] + 8 + B * p.nreq * p.nrow

    def scripted(self, script=()):
        ts = ScriptedTranscript(SEED)
        for kind, epoch, at, data in script:
            getattr(ts, kind)(epoch, at, data)
        return ts

    def prove(self, script=()):
        ts = self.scripted(script)
        self.root = self.zk.commit(self.W, self.lf.LcgRng(self.rec["rng_seed"]).bytes, ts)
        assert self.zk.prove(self.W, ts) is True
        ts.check()
        return self.zk.wire(), ts

    def verify(self, wire, pub=None, script=(), committed=False, ts=None):
        ts = self.scripted(script) if ts is None else ts
        if committed:
            ts.write_bytes(wire[:32])
        r = self.G.pkg.zk_verify(self.gpu, self.circ, wire, self.pub if pub is None else pub, ts, self.rec["rate"], self.rec["nreq"],
                                 self.rec["block_enc_arg"], committed=committed)
        ts.check()
        return r

    def close(self):
        self.zk.close()
        self.circ.close()


_zk = {}


def zk_case(G, field):
    if field not in _zk:
        _zk[field] = ZkCase(G, field)
    return _zk[field]


@pytest.fixture(params=sorted(ZK))
def zkc(G, request):
    return zk_case(G, request.param)


@pytest.mark.parametrize("committed", [False, True], ids=["zk_verify", "zk_verify_committed"])
def test_zk_each_check_refuses(zkc, committed):
    p, d, o, B, mod = zkc.p, zkc.wire, zkc.o, zkc.B, zkc.modulus

    def verify(wire, pub=None):
        return zkc.verify(wire, pub=pub, committed=committed)

    assert verify(d) == (True, "ok")
    for what, off, why in y_cases(p, B, o):
        assert verify(flip_low_bit(d, off, B, mod)) == (False, why), what
    # The statement side.  build_constraints (csrc/zk_proto.h) turns the sumcheck section and the public inputs into the rows of A
    # and the right-hand sides b.  A round value p(0), p(2) enters through Expression::axpy / axmy as the KNOWN factor: it moves
    # `known`, hence b[layer], while the symbolic coefficients (the entries of A) are products of challenges only -- and the
    # challenges do not move here.  So A is the honest one, the dot check passes, and the dot VALUE is wrong.  The public inputs
    # enter only input_constraint_b's pub_binding, the last entry of b: the same.  A claim wc enters ConstraintBuilder::finalize as a
    # COEFFICIENT of the claim pads (sym[cp] -= eqq wc[1], sym[cp + 1] -= eqq wc[0]): one entry of A changes, the extended row of A
    # differs at every opened column, and the dot check refuses before the value is looked at.
    first, last = 0, len(zkc.logw) - 1
    for ly in (first, last):
        assert zkc.logw[ly] >= 1
        t0, wc1 = zkc.o_layer[ly], zkc.o_layer[ly + 1] - B
        assert verify(flip_low_bit(d, t0, B, mod)) == (False, DOT_VALUE), ("round value, layer", ly)
        assert verify(flip_low_bit(d, t0 + B * (4 * zkc.logw[ly] - 1), B, mod)) == (False, DOT_VALUE), ("last round value, layer", ly)
        assert verify(flip_low_bit(d, wc1, B, mod)) == (False, DOT), ("wc[1], layer", ly)
        assert verify(flip_low_bit(d, wc1 - B, B, mod)) == (False, DOT), ("wc[0], layer", ly)
    pub = zkc.pub.copy()
    pub[-1, 0] ^= np.uint64(2)  # the Elt image of the public input (wire 0, the constant one): still an element
    assert mod is None or sum(int(x) << (64 * i) for i, x in enumerate(pub[-1])) < mod
    assert verify(d, pub=pub) == (False, DOT_VALUE)
    # the commitment
    for what, off in (("root", 5), ("nonce", o["nonces"] + 32 * 2 + 1), ("last nonce", o["nonces"] + 32 * p.nreq - 1), ("path", len(d) - 9)):
        assert verify(flip_byte(d, off)) == (False, MERKLE), what
    for j in (0, p.nreq - 1):
        assert verify(flip_low_bit(d, zkc.o_col + B * j, B, mod)) == (False, MERKLE), j


@pytest.mark.parametrize("field", ["fp128", "p256"])
def test_zk_rejected_draws(G, field):
    """Fp128 and Fp256Base: an all-ones draw spliced in front of the first sumcheck challenge (drawn on the clone, replayed on the
    original by the prover's build_constraints and by the verifier), in front of the first round challenge and in front of the first
    u_ldt draw: the wire is the unspliced run's, each lineage draws once more per splice, the verifier accepts under the script."""
    zkc = zk_case(G, field)
    B = zkc.B
    first_sc = zkc.clone_eps[0]  # the epoch the clone was made in: begin_circuit's 80 draws and the first layer's alpha, beta
    assert first_sc["draws"] == [B] * 82
    first_round = [e for e in zkc.clone_eps if e["write"] == (1, B) and e["draws"]][0]  # behind write(p(0)), write(p(2))
    assert first_round["draws"] == [B] and first_round["epoch"] == first_sc["epoch"] + 2
    ce = challenge_epoch(zkc.eps)
    n_ch = zkc.p.nwqrow + 10 + 3 * zkc.p.nq + zkc.p.nqtriples  # nl + 1 = 10 linear constraints
    assert ce["draws"] == [B] * n_ch
    ff = b"\xff" * B
    script = [("splice", e["epoch"], 0, ff) for e in (first_sc, first_round, ce)]
    wire, ts = zkc.prove(script)
    assert wire == zkc.wire
    (cl,) = ts.clones()
    by_epoch = {e["epoch"]: e["draws"] for e in ts.epochs()}
    by_epoch_clone = {e["epoch"]: e["draws"] for e in ts.epochs(cl)}
    assert by_epoch_clone[first_sc["epoch"]] == [B] * 83 and by_epoch_clone[first_round["epoch"]] == [B] * 2
    assert by_epoch[first_sc["epoch"]] == [B] * 83 and by_epoch[first_round["epoch"]] == [B] * 2  # the replay on the original
    assert by_epoch[ce["epoch"]] == [B] * (n_ch + 1)
    assert sum(map(len, by_epoch.values())) == sum(len(e["draws"]) for e in zkc.eps) + 3
    tv = zkc.scripted(script)
    assert zkc.verify(wire, ts=tv) == (True, "ok")
    assert {e["epoch"]: e["draws"] for e in tv.epochs()} == by_epoch  # the verifier draws what the prover's original lineage drew


def test_zk_edge_columns(zkc):
    p, B = zkc.p, zkc.B
    n = p.block_ext
    assert nat_len(n) == nat_len(n - 1)
    ln = nat_len(n)
    ch = choose_epoch(zkc.eps)
    script = [("replace", ch["epoch"], 0, (0).to_bytes(ln, "little")), ("replace", ch["epoch"], ln, (n - 2).to_bytes(ln, "little"))]
    wire, ts = zkc.prove(script)  # Ts::choose makes columns 0 and block_ext - 1 of that stream (test_ligero_edge_columns sees the indices)
    o = zkc.o
    assert wire[:o["nonces"]] == zkc.wire[:o["nonces"]] and wire[o["nonces"]:] != zkc.wire[o["nonces"]:]
    assert choose_epoch(ts.epochs())["draws"][:2] == [ln, ln]
    assert zkc.verify(wire, script=script) == (True, "ok")
    assert zkc.verify(wire, script=script, committed=True) == (True, "ok")
    assert zkc.verify(flip_low_bit(wire, zkc.o_col + B * 1, B, zkc.modulus), script=script) == (False, MERKLE)
    assert zkc.verify(flip_low_bit(wire, zkc.o_col + B * 0, B, zkc.modulus), script=script) == (False, MERKLE)
    assert zkc.verify(wire) == (False, MERKLE)  # under the plain script other columns are asked for


def test_zk_close(G):
    """(last) provers and circuits are released"""
    for c in _zk.values():
        c.close()
    _zk.clear()

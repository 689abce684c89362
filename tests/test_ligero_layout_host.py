"""csrc/ligero_layout.h on the host: lig::layout, the host half of LigeroProver::commit for all three fields, compiled without
device code (tests/host_ligero_layout.hip) and checked against an independent Python model written from ligero_prover.h:171-270
and merkle_commitment.h:52-54.  The engine is a Python callback over a scripted byte string that records the size of every call.
No GPU."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import __graft_entry__ as ge
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostligerolayout.so")
SRC = os.path.join(HERE, "host_ligero_layout.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
GF, FP128, P256 = 4, 6, 1
FIELDS = [GF, FP128, P256]
PRIME = {FP128: 2**128 - 2**108 + 1, P256: 2**256 - 2**224 + 2**192 + 2**96 - 1}
NBYTES = {GF: 16, FP128: 16, P256: 32}
SUB_BYTES = 2  # kSubFieldBytes of GF2_128<4>
ERR_ARG, ERR_ASSERT = 1, 5
NW, NQ, SFB = 40, 10, 17  # witnesses, quadratic constraints, and (GF) a subfield boundary strictly inside witness row 2
RNG_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)

_libs = None


def _lib():
    """(harness, package): the harness links against the built library for the host helpers ligero_layout.h calls"""
    global _libs
    if _libs is None:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        if not os.path.exists(ge.LIB):
            ge.build()
        pkg = ge.load_package()
        pkg.load_library()
        csrc = os.path.join(ol.ROOT, "longfellow-zk_amd", "csrc")
        deps = [SRC, ge.LIB] + [os.path.join(csrc, h) for h in ("ligero_layout.h", "fp256.h", "fields.h", "ctx.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC, "-L" + os.path.dirname(ge.LIB),
                                   "-l:" + os.path.basename(ge.LIB), "-Wl,-rpath," + os.path.dirname(ge.LIB)])
        _libs = (C.CDLL(SO), pkg)
    return _libs


def _param(pkg, field, nw, nq):
    """rate 4, 3 opened columns, block_enc 63: block 10, w 7, dblock 19, 44 leaves"""
    p = pkg.LigeroParam()
    rc = pkg.load_library().lfgpu_ligero_param_init(C.byref(p), C.c_int(field), C.c_int(4 if field != P256 else 0), C.c_size_t(nw), C.c_size_t(nq),
                                                    C.c_size_t(4), C.c_size_t(3), C.c_size_t(63))
    assert rc == 0
    # what the cases below rely on: two witness rows or more with the last one partly filled; with nq, the same for the triples
    assert p.nwrow >= 2 and nw % p.w != 0 and p.w >= 2 and p.r >= 1 and p.block_ext >= 2
    assert (p.nqtriples >= 2 and nq % p.w != 0) if nq else p.nqtriples == 0
    assert p.nrow == 3 + p.nwrow + 3 * p.nqtriples and (p.ildt, p.idot, p.iquad, p.iw) == (0, 1, 2, 3) and p.iq == 3 + p.nwrow
    return p


def _gf_sub(u):
    """of_scalar(u) = sum_i bit_i(u) beta_i over the 16-bit subfield basis"""
    beta = ol.gf_ctx(4).beta
    v = 0
    for i in range(16):
        if (u >> i) & 1:
            v ^= int(beta[i].l[0]) | int(beta[i].l[1]) << 64
    return v


def _mul(field, a, b):
    if field != GF:
        return a * b % PRIME[field]
    e = lambda v: ol.Elt((C.c_uint64 * 2)(v & (2**64 - 1), v >> 64))
    r = ol.oracle().lfo_gf_mul(e(a), e(b))
    return int(r.l[0]) | int(r.l[1]) << 64


def _witness(field, p, seed):
    """(W, lqc): NW canonical values -- for GF subfield elements (0 and 1 among them) below SFB -- and nq triples with
    W[l2] = W[l0] W[l1], the products in the last nq places"""
    rng = random.Random(seed)
    W = [rng.randrange(PRIME[field]) if field != GF else rng.getrandbits(128) for _ in range(p.nw)]
    if field == GF:
        W[:SFB] = [0, 1] + [_gf_sub(rng.randrange(1 << 16)) for _ in range(SFB - 2)]
    lqc = []
    for i in range(p.nq):
        l0, l1, l2 = rng.randrange(p.nw - p.nq), rng.randrange(p.nw - p.nq), p.nw - p.nq + i
        W[l2] = _mul(field, W[l0], W[l1])
        lqc += [l0, l1, l2]
    return W, lqc


class Model:
    """LigeroProver::commit's layout over a byte stream, in Python integers; `sizes` is the reference's call pattern: one call
    per attempt, per subfield element and per nonce"""

    def __init__(self, field, stream):
        self.field, self.stream, self.pos, self.sizes = field, stream, 0, []

    def take(self, n):
        self.sizes.append(n)
        self.pos += n
        assert self.pos <= len(self.stream)
        return self.stream[self.pos - n:self.pos]

    def elt(self):  # Field::sample: rejection sampling for the prime fields
        while True:
            v = int.from_bytes(self.take(NBYTES[self.field]), "little")
            if self.field == GF or v < PRIME[self.field]:
                return v

    def sub_elt(self):  # Field::sample_subfield
        return _gf_sub(int.from_bytes(self.take(SUB_BYTES), "little")) if self.field == GF else self.elt()

    def layout(self, p, W, sfb, lqc):
        f, pm = self.field, PRIME.get(self.field)
        T = [[0] * p.dblock for _ in range(p.nrow)]
        T[p.ildt][:p.block] = [self.elt() for _ in range(p.block)]  # layout_blinding_rows
        T[p.idot] = [self.elt() for _ in range(p.dblock)]
        rest = T[p.idot][p.r + 1:p.r + p.w]
        if f == GF:  # the W part sums to zero
            T[p.idot][p.r] = 0
            for v in rest:
                T[p.idot][p.r] ^= v
        else:
            T[p.idot][p.r] = -sum(rest) % pm
        T[p.iquad] = [self.elt() for _ in range(p.dblock)]
        T[p.iquad][p.r:p.r + p.w] = [0] * p.w
        for i in range(p.nwrow):  # layout_witness_rows
            sub = (i + 1) * p.w <= sfb
            T[p.iw + i][:p.r] = [self.sub_elt() if sub else self.elt() for _ in range(p.r)]
            chunk = W[i * p.w:(i + 1) * p.w]
            T[p.iw + i][p.r:p.r + len(chunk)] = chunk
        for i in range(p.nqtriples):  # layout_quadratic_rows: x, y, z rows of triple i are drawn one after the other
            for h in range(3):
                T[p.iq + h * p.nqtriples + i][:p.r] = [self.elt() for _ in range(p.r)]
            for j in range(min(p.w, p.nq - i * p.w)):
                for h in range(3):
                    T[p.iq + h * p.nqtriples + i][p.r + j] = W[lqc[3 * (i * p.w + j) + h]]
        nonces = b"".join(self.take(32) for _ in range(p.block_ext))  # MerkleCommitment::commit
        return T, nonces


class Engine:
    """the RandomEngine hook: serves `stream`, records the size of every call"""

    def __init__(self, stream):
        self.stream, self.pos, self.calls = stream, 0, []

        def fill(_, buf, n):
            self.calls.append(n)
            chunk = self.stream[self.pos:self.pos + n]
            self.pos += n
            C.memmove(buf, chunk + bytes(n - len(chunk)), n)

        self.fn = RNG_FN(fill)


def _run(L, field, p, W, sfb, lqc, stream, exact=False, lo=0, hi=None, want_nonces=True):
    """(rc, rows as integers, nonces, engine, message)"""
    hi = p.nrow if hi is None else hi
    nb = NBYTES[field]
    eng = Engine(stream)
    rows = C.create_string_buffer(max((hi - lo) * p.dblock * nb, 1))
    nonces = C.create_string_buffer(32 * p.block_ext) if want_nonces else None
    err = C.create_string_buffer(256)
    rc = L.hll_layout(C.c_int(field), C.byref(p), b"".join(v.to_bytes(nb, "little") for v in W), C.c_size_t(sfb), (C.c_size_t * max(len(lqc), 1))(*lqc),
                      eng.fn, None, C.c_int(int(exact)), C.c_size_t(lo), C.c_size_t(hi), rows, nonces, err)
    got = [[int.from_bytes(rows.raw[(i * p.dblock + j) * nb:(i * p.dblock + j + 1) * nb], "little") for j in range(p.dblock)] for i in range(hi - lo)]
    return rc, got, nonces.raw if want_nonces else None, eng, err.value.decode()


def _stream(field, p, seed, reject_at=None):
    """more random bytes than a layout draws; reject_at: an attempt (counted in elements from the start) replaced by 0xff.."""
    nb = NBYTES[field]
    s = bytearray(random.Random(seed).randbytes(nb * (p.nrow * p.dblock + 8) + 32 * p.block_ext))
    if reject_at is not None:
        s[nb * reject_at:nb * (reject_at + 1)] = b"\xff" * nb
    return bytes(s)


_whole = {}


def _case(field, nq):
    """the whole layout of one shape, computed once: (L, p, W, sfb, lqc, stream, model rows, model nonces, model)"""
    if (field, nq) not in _whole:
        L, pkg = _lib()
        p = _param(pkg, field, NW, nq)
        sfb = SFB if field == GF else 0
        if field == GF:  # the boundary falls strictly inside a witness row
            assert sfb % p.w != 0 and 2 * p.w <= sfb < p.nw
        W, lqc = _witness(field, p, 11 * field + nq)
        stream = _stream(field, p, 1000 + field)
        m = Model(field, stream)
        T, nonces = m.layout(p, W, sfb, lqc)
        _whole[(field, nq)] = (L, p, W, sfb, lqc, stream, T, nonces, m)
    return _whole[(field, nq)]


@pytest.mark.parametrize("nq", [NQ, 0])
@pytest.mark.parametrize("field", FIELDS)
def test_whole_layout_matches_model(field, nq):
    L, p, W, sfb, lqc, stream, T, nonces, m = _case(field, nq)
    for exact in (False, True):
        rc, got, gn, eng, msg = _run(L, field, p, W, sfb, lqc, stream, exact)
        assert rc == 0, msg
        assert got == T and gn == nonces and eng.pos == m.pos == sum(eng.calls)
        if exact:  # one call per attempt, per subfield element and per nonce
            assert eng.calls == m.sizes
    if field == GF:  # rows 0 and 1 lie below the boundary (subfield draws), row 2 holds it (full-field draws)
        first = p.block + 2 * p.dblock  # draws in front of the witness rows
        assert m.sizes[first:first + 3 * p.r] == [SUB_BYTES] * (2 * p.r) + [16] * p.r


@pytest.mark.parametrize("field", FIELDS)
def test_every_slab_equals_its_rows_of_the_whole(field):
    L, p, W, sfb, lqc, stream, T, nonces, m = _case(field, NQ)
    single = [p.ildt, p.idot, p.iquad, p.iw, p.iq - 1, p.nrow - 1]  # blinding rows, first / last witness row, last quadratic row
    cuts = [(0, 0), (0, p.nrow)] + [(i, i + 1) for i in single] + [(0, 2), (2, p.iw + 1), (p.iw + 1, p.iq + 1), (p.iq + 1, p.nrow)]
    for exact in (False, True):
        for lo, hi in cuts:
            rc, got, gn, eng, msg = _run(L, field, p, W, sfb, lqc, stream, exact, lo, hi)
            assert rc == 0, msg
            assert got == T[lo:hi] and gn == nonces and eng.pos == m.pos, (lo, hi, exact)
            if exact:
                assert eng.calls == m.sizes
    # the empty slab without a nonce buffer only advances the engine
    rc, got, gn, eng, msg = _run(L, field, p, W, sfb, lqc, stream, False, 0, 0, want_nonces=False)
    assert rc == 0 and got == [] and eng.pos == m.pos


@pytest.mark.parametrize("field", [FP128, P256])
def test_rejected_attempt_same_elements_exact_or_merged(field):
    L, p, W, sfb, lqc, _, _, _, _ = _case(field, NQ)
    nb = NBYTES[field]
    reject_at = p.block + p.r + 2  # inside the IDOT row's draws
    stream = _stream(field, p, 2000 + field, reject_at)
    m = Model(field, stream)
    T, nonces = m.layout(p, W, sfb, lqc)
    nelts = p.block + 2 * p.dblock + p.r * (p.nwrow + 3 * p.nqtriples)
    assert m.sizes.count(nb) - (p.block_ext if nb == 32 else 0) > nelts  # at least one attempt was rejected
    runs = [_run(L, field, p, W, sfb, lqc, stream, exact) for exact in (False, True)]
    for rc, got, gn, eng, msg in runs:
        assert rc == 0, msg
        assert got == T and gn == nonces and eng.pos == m.pos
    assert runs[1][3].calls == m.sizes and set(m.sizes) == {nb, 32}
    assert len(runs[0][3].calls) < len(m.sizes)  # merged draws: fewer calls for the same bytes


@pytest.mark.parametrize("field", FIELDS)
def test_error_paths(field):
    L, p, W, sfb, lqc, stream, _, _, _ = _case(field, NQ)
    bad = list(lqc)
    bad[3 * (p.nq - 1) + 1] = p.nw  # an index >= nw in the last, partly filled triple
    rc, _, _, _, msg = _run(L, field, p, W, sfb, bad, stream)
    assert rc == ERR_ARG and msg == "ligero_commit: lqc index >= nw"
    W2 = list(W)
    W2[lqc[2]] ^= 1  # W[l2] != W[l0] * W[l1] (the flipped value stays canonical: the products are never p - 1 here)
    assert field == GF or W2[lqc[2]] < PRIME[field]
    rc, _, _, _, msg = _run(L, field, p, W2, sfb, lqc, stream)
    assert rc == ERR_ASSERT and msg == "ligero_commit: invalid quadratic constraints (ligero_prover.h:259-260)"
    if field == GF:  # a full-field value below the boundary: refused before any draw
        W3 = list(W)
        W3[5] = 1 << 127
        rc, _, _, eng, msg = _run(L, field, p, W3, sfb, lqc, stream)
        assert rc == ERR_ARG and eng.calls == []
        assert msg == "ligero_commit: element not in subfield: W[5], below subfield_boundary %d (ligero_prover.h:63-66)" % sfb

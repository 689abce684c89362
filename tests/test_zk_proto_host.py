"""csrc/zk_proto.h on the host: the field-generic protocol layer's wire format (ZkProof::write / read), the sparse share of
inner_product_vector, the transcript view and the staging of ZkProver::commit's witness, compiled without device code (tests/host_zk_proto.hip) and checked against
independent Python models.  No GPU: the device steps of the policies are not instantiated here."""
import ctypes as C
import os
import random
import shutil
import struct
import subprocess

import pytest

import __graft_entry__ as ge
import oracle_lib as ol
from fs_transcript import Transcript

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libhostzkproto.so")
SRC = os.path.join(HERE, "host_zk_proto.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
GF, FP128, P256 = 4, 6, 1
PRIME = {FP128: 2**128 - 2**108 + 1, P256: 2**256 - 2**224 + 2**192 + 2**96 - 1}
NBYTES = {GF: 16, FP128: 16, P256: 32}
LOGW = [0, 1, 3, 2]  # a zero-round layer and a first layer (zk_proof.h sends 4 logw + 2 elements per layer)
MAX_RUN = 1 << 25


class HzpProof(C.Structure):
    _fields_ = [("root", C.c_uint8 * 32)] + [(n, C.c_char_p) for n in ("sc", "y_ldt", "y_dot", "y_q0", "y_q2", "req", "nonces", "path")] + \
               [("npath", C.c_size_t)]


_libs = None


def _lib():
    """(harness, package): the harness links against the built library for the host helpers zk_proto.h calls"""
    global _libs
    if _libs is None:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        if not os.path.exists(ge.LIB):
            ge.build()
        pkg = ge.load_package()
        pkg.load_library()
        csrc = os.path.join(ol.ROOT, "longfellow-zk_amd", "csrc")
        deps = [SRC, ge.LIB] + [os.path.join(csrc, h) for h in ("zk_proto.h", "hostfield.h", "fp256.h", "fields.h", "ctx.h", "zkint.h")]
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC, "-L" + os.path.dirname(ge.LIB),
                                   "-l:" + os.path.basename(ge.LIB), "-Wl,-rpath," + os.path.dirname(ge.LIB)])
        L = C.CDLL(SO)
        L.hzp_nat.restype = C.c_size_t
        _libs = (L, pkg)
    return _libs


def _param(pkg, field, nw, nq, nreq=3):
    p = pkg.LigeroParam()
    fn = pkg.load_library().lfgpu_ligero_param_init
    rc = fn(C.byref(p), C.c_int(field), C.c_int(4 if field != P256 else 0), C.c_size_t(nw), C.c_size_t(nq), C.c_size_t(4), C.c_size_t(nreq), C.c_size_t(0))
    assert rc == 0
    return p


def _enc(field, v):
    return v.to_bytes(NBYTES[field], "little")


def _rand_elt(rng, field):
    return rng.randrange(PRIME[field]) if field != GF else rng.getrandbits(128)


def _gf_sub(u):
    """of_scalar(u) = sum_i bit_i(u) beta_i over the 16-bit subfield basis"""
    beta = ol.gf_ctx(4).beta
    v = 0
    for i in range(16):
        if (u >> i) & 1:
            v ^= int(beta[i].l[0]) | int(beta[i].l[1]) << 64
    return v


class Proof:
    """a ZkProof of deterministic pseudo-random canonical elements; req[i] = (value, subfield coordinates or None)"""

    def __init__(self, field, p, seed):
        rng = random.Random(seed)
        self.field, self.p = field, p
        self.root = bytes(rng.randrange(256) for _ in range(32))
        self.hp = [[[_rand_elt(rng, field) for _ in range(2 * lw)] for _ in range(2)] for lw in LOGW]
        self.wc = [[_rand_elt(rng, field) for _ in range(2)] for _ in LOGW]
        self.y = [[_rand_elt(rng, field) for _ in range(n)] for n in (p.block, p.dblock, p.r, p.dblock - p.block)]
        self.req = []
        for i in range(p.nreq * p.nrow):
            if field == GF and (i // 5) % 2 == 0:  # runs of 5: full-field first, as the format starts
                self.req.append((_rand_elt(rng, field), None))
            elif field == GF:
                u = rng.randrange(1 << 16)
                self.req.append((_gf_sub(u), u))
            else:
                self.req.append((_rand_elt(rng, field), None))
        self.nonces = bytes(rng.randrange(256) for _ in range(32 * p.nreq))
        self.npath = p.nreq + 1
        self.path = bytes(rng.randrange(256) for _ in range(32 * self.npath))

    def wire(self):
        """(bytes, section boundaries) by the zk_proof.h layout, written from the layout and nothing else"""
        f = self.field
        out, cuts = bytearray(self.root), [0, 32]
        for lw, hp, wc in zip(LOGW, self.hp, self.wc):  # per round: p(0) of both hands, then p(2) of both hands; then wc
            for rnd in range(lw):
                for k in range(2):
                    out += _enc(f, hp[0][2 * rnd + k]) + _enc(f, hp[1][2 * rnd + k])
            out += _enc(f, wc[0]) + _enc(f, wc[1])
            cuts.append(len(out))
        for y in self.y:
            out += b"".join(_enc(f, v) for v in y)
            cuts.append(len(out))
        out += self.nonces
        cuts.append(len(out))
        i, sub_run = 0, False  # alternating full-field / subfield runs, full-field first, u32 length each
        is_sub = (lambda e: e[1] is not None) if f == GF else (lambda e: True)
        while i < len(self.req):
            n = 0
            while i + n < len(self.req) and n < MAX_RUN and is_sub(self.req[i + n]) == sub_run:
                n += 1
            out += struct.pack("<I", n)
            for v, u in self.req[i:i + n]:
                out += struct.pack("<H", u) if (sub_run and f == GF) else _enc(f, v)
            cuts.append(len(out))
            i, sub_run = i + n, not sub_run
        out += struct.pack("<I", self.npath)
        cuts.append(len(out))
        out += self.path
        return bytes(out), cuts

    def sc_bytes(self):
        f = self.field
        return b"".join(b"".join(_enc(f, v) for v in hp[0] + hp[1] + wc) for hp, wc in zip(self.hp, self.wc))

    def members(self):
        f = self.field
        return [self.sc_bytes()] + [b"".join(_enc(f, v) for v in y) for y in self.y] + [b"".join(_enc(f, v) for v, _ in self.req), self.nonces, self.path]


def _write(L, field, p, pr):
    hp = HzpProof()
    hp.root[:] = pr.root
    for name, b in zip(("sc", "y_ldt", "y_dot", "y_q0", "y_q2", "req", "nonces", "path"), pr.members()):
        setattr(hp, name, b)
    hp.npath = pr.npath
    out, n = C.create_string_buffer(1 << 20), C.c_size_t(0)
    logw = (C.c_size_t * len(LOGW))(*LOGW)
    assert L.hzp_write(C.c_int(field), logw, C.c_size_t(len(LOGW)), C.byref(p), C.byref(hp), out, C.c_size_t(len(out)), C.byref(n)) == 0
    return out.raw[:n.value]


def _read(L, field, p, wire):
    """the parsed members, or None when ZkProof::read refuses"""
    nb = NBYTES[field]
    sizes = [sum(4 * lw + 2 for lw in LOGW) * nb, p.block * nb, p.dblock * nb, p.r * nb, (p.dblock - p.block) * nb, p.nreq * p.nrow * nb, 32 * p.nreq,
             32 * p.nreq * p.mc_pathlen]
    bufs = [C.create_string_buffer(max(s, 1)) for s in sizes]
    hp = HzpProof()
    for name, b in zip(("sc", "y_ldt", "y_dot", "y_q0", "y_q2", "req", "nonces", "path"), bufs):
        setattr(hp, name, C.cast(b, C.c_char_p))
    logw = (C.c_size_t * len(LOGW))(*LOGW)
    if not L.hzp_read(C.c_int(field), logw, C.c_size_t(len(LOGW)), C.byref(p), wire, C.c_size_t(len(wire)), C.byref(hp)):
        return None
    sizes[-1] = 32 * hp.npath
    return bytes(hp.root), [b.raw[:s] for b, s in zip(bufs, sizes)], hp.npath


@pytest.mark.parametrize("field", [FP128, P256, GF])
def test_wire_round_trip_and_refusals(field):
    L, pkg = _lib()
    nb = NBYTES[field]
    p = _param(pkg, field, 40 + sum(4 * lw + 3 for lw in LOGW), len(LOGW))
    pr = Proof(field, p, 7 + field)
    want, cuts = pr.wire()
    got = _write(L, field, p, pr)
    assert got == want
    back = _read(L, field, p, want)
    assert back is not None and back[0] == pr.root and back[1] == pr.members() and back[2] == pr.npath
    # every proper prefix that ends at a section boundary, and the proof less its last byte
    assert cuts == sorted(set(cuts)) and cuts[-1] < len(want)
    for cut in cuts + [len(want) - 1]:
        assert _read(L, field, p, want[:cut]) is None, cut
    if field != GF:  # an element encoding >= p, in a sumcheck element, a y vector and an opened column
        top = b"\xff" * nb
        req0 = cuts[-2] - p.nreq * p.nrow * nb  # the one subfield run holds every opened element
        for off in (32, cuts[len(LOGW) + 1], req0):
            assert _read(L, field, p, want[:off] + top + want[off + nb:]) is None, off
        assert _read(L, field, p, want[:32] + _enc(field, PRIME[field] - 1) + want[32 + nb:]) is not None
    # the digest count: below nreq, above nreq * mc_pathlen (the bytes are there in both cases)
    head = want[:cuts[-1] - 4]
    for bad in (p.nreq - 1, p.nreq * p.mc_pathlen + 1):
        assert _read(L, field, p, head + struct.pack("<I", bad) + bytes(32 * bad)) is None, bad
    assert _read(L, field, p, head + struct.pack("<I", p.nreq) + bytes(32 * p.nreq)) is not None
    # a run length that overruns nreq * nrow (again with the bytes present)
    runs0 = cuts[len(LOGW) + 6]  # after the nonces: the first run's length
    first = struct.unpack("<I", want[runs0:runs0 + 4])[0]
    total = p.nreq * p.nrow
    over = want[:runs0] + struct.pack("<I", total + 1) + bytes((total + 1) * nb) + want[runs0 + 4 + first * nb:]
    assert _read(L, field, p, over) is None


@pytest.mark.parametrize("field", [FP128, P256])
def test_inner_product_sparse_matches_integer_model(field):
    L, pkg = _lib()
    pm, nb = PRIME[field], NBYTES[field]
    rng = random.Random(100 + field)
    p = _param(pkg, field, 50, 4)
    base = p.nwrow * p.w
    ncon = 5
    lqc = [rng.randrange(50) for _ in range(3 * p.nq)]
    lqc[4] = lqc[0]  # two copy constraints on one witness element
    # linear terms: duplicates among themselves, on a copy term's original (lqc) and on a copy's own slot (Ax + 1)
    lin = [(rng.randrange(ncon), rng.randrange(50), rng.randrange(pm)) for _ in range(30)]
    lin += [(0, lqc[0], rng.randrange(pm)), (3, lqc[0], rng.randrange(pm)), (1, base + 1, rng.randrange(pm)), lin[2]]
    alphal = [rng.randrange(pm) for _ in range(ncon)]
    alphaq = [rng.randrange(pm) for _ in range(3 * p.nq)]
    model = {}
    for c, w, k in lin:
        model[w] = (model.get(w, 0) + k * alphal[c]) % pm
    for iw in range(p.nq):
        for j in range(3):
            aq, copy = alphaq[3 * iw + j], base + j * p.nqtriples * p.w + iw
            model[copy] = (model.get(copy, 0) + aq) % pm
            model[lqc[3 * iw + j]] = (model.get(lqc[3 * iw + j], 0) - aq) % pm
    sz = lambda v: (C.c_size_t * len(v))(*v)
    cat = lambda v: b"".join(_enc(field, x) for x in v)
    cap = len(lin) + 6 * p.nq
    idx, val, n = (C.c_uint64 * cap)(), C.create_string_buffer(cap * nb), C.c_size_t(0)
    rc = L.hzp_inner_product_sparse(C.c_int(field), C.byref(p), C.c_size_t(len(lin)), sz([t[0] for t in lin]), sz([t[1] for t in lin]), cat([t[2] for t in lin]),
                                    C.c_size_t(ncon), cat(alphal), sz(lqc), cat(alphaq), idx, val, C.byref(n))
    assert rc == 0
    got_idx = list(idx[:n.value])
    assert got_idx == sorted(model) and len(got_idx) < cap  # sorted, folded
    assert [int.from_bytes(val.raw[nb * i:nb * (i + 1)], "little") for i in range(n.value)] == [model[i] for i in got_idx]


class Hooks:
    """lfgpu_transcript_ops over fs_transcript.Transcript; every element write is recorded as the hook saw it"""

    def __init__(self, pkg, init=b"zk_proto"):
        self.t, self.calls = Transcript(init), []
        vp, sz, pb = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8)

        def gen(_, out, n):
            C.memmove(out, self.t.bytes(n), n)

        self._keep = [
            C.CFUNCTYPE(None, vp, pb, sz)(lambda _, d, n: self.calls.append(("bytes", C.string_at(d, n)))),
            C.CFUNCTYPE(None, vp, pb)(lambda _, e: self.calls.append(("elt", C.string_at(e, 16)))),
            C.CFUNCTYPE(None, vp, pb, sz)(lambda _, e, n: self.calls.append(("array", C.string_at(e, 16 * n), n))),
            C.CFUNCTYPE(None, vp, pb, sz)(gen),
            C.CFUNCTYPE(None, vp, pb, sz)(lambda _, e, nb: self.calls.append(("elt_sized", C.string_at(e, nb), nb))),
            C.CFUNCTYPE(None, vp, pb, sz, sz)(lambda _, e, n, nb: self.calls.append(("array_sized", C.string_at(e, n * nb), n, nb))),
        ]
        k = [C.cast(f, vp) for f in self._keep]
        self.ops = pkg.TranscriptOps(None, k[0], k[1], k[2], k[3], None, None, k[4], k[5])


@pytest.mark.parametrize("field", [FP128, P256, GF])
def test_transcript_view(field):
    L, pkg = _lib()
    nb = NBYTES[field]
    for n in (1, 64, 65, 4096, 4097):  # RandomEngine::nat: n = 1, powers of two, powers of two plus one
        h, ref = Hooks(pkg), Transcript(b"zk_proto")
        assert [L.hzp_nat(C.c_int(field), C.byref(h.ops), C.c_size_t(n)) for _ in range(20)] == [ref.nat(n) for _ in range(20)]
    for n, k in ((1, 1), (64, 9), (65, 65), (257, 6)):  # RandomEngine::choose
        h, ref = Hooks(pkg), Transcript(b"zk_proto")
        res = (C.c_size_t * k)()
        L.hzp_choose(C.c_int(field), C.byref(h.ops), C.c_size_t(n), C.c_size_t(k), res)
        assert list(res) == ref.choose(n, k)
    rng = random.Random(field)
    elts = [_rand_elt(rng, field) for _ in range(3)]
    for n in (0, 3):  # write_array: one hook call with the count and the to_bytes_field images
        h = Hooks(pkg)
        img = b"".join(_enc(field, v) for v in elts[:n])
        assert L.hzp_write_array(C.c_int(field), C.byref(h.ops), img, C.c_size_t(n)) == 0
        assert h.calls == ([("array_sized", img, n, 32)] if field == P256 else [("array", img, n)])
    h = Hooks(pkg)
    assert L.hzp_write_elt(C.c_int(field), C.byref(h.ops), _enc(field, elts[0])) == 0
    assert h.calls == ([("elt_sized", _enc(field, elts[0]), 32)] if field == P256 else [("elt", _enc(field, elts[0]))])


# ---- zkp::stage_witness: the witness of ZkProver::commit (private inputs || fill_pad) against a model of the reference
def _gf_mul(a, b):
    """GF(2^128) = GF(2)[x] / (x^128 + x^7 + x^2 + x + 1), bit i of the integer = the coefficient of x^i"""
    r = 0
    for i in range(128):
        if (b >> i) & 1:
            r ^= a << i
    for i in range(254, 127, -1):
        if (r >> i) & 1:
            r ^= (1 << i) | (0x87 << (i - 128))
    return r


class ScriptedEngine:
    """RandomEngine over a fixed byte stream; Field::sample as the reference draws it: kBytes per attempt, one bytes() call each,
    rejected when the little-endian value is >= p (lib/algebra/fp_generic.h:360-371; every 16-byte string is in GF(2^128))"""

    def __init__(self, stream):
        self.stream, self.pos, self.calls = stream, 0, []

    def bytes(self, n):
        assert self.pos + n <= len(self.stream)
        self.calls.append(n)
        self.pos += n
        return self.stream[self.pos - n:self.pos]

    def elt(self, field):
        while True:
            v = int.from_bytes(self.bytes(NBYTES[field]), "little")
            if field == GF or v < PRIME[field]:
                return v


def _fill_pad_model(field, rng, inputs, npub):
    """(witness, lqc): the private inputs, then ZkProver::fill_pad (zk_prover.h:152-188, logc = 0) -- per layer and round p(0) and
    p(2) of hand 0 then hand 1, then wc0, wc1 and the computed product -- with setup_lqc's indices of the last three (zk_common.h)"""
    mul = _gf_mul if field == GF else (lambda a, b: a * b % PRIME[field])
    w, lqc = list(inputs[npub:]), []
    for lw in LOGW:
        for _ in range(lw):
            for _h in range(2):
                for k in range(3):
                    if k != 1:
                        w.append(rng.elt(field))
        wc = [rng.elt(field), rng.elt(field)]
        lqc += [len(w), len(w) + 1, len(w) + 2]
        w += wc + [mul(wc[0], wc[1])]
    return w, lqc


STAGE_NPUB, STAGE_NIN = 2, 7


def _stage_stream():
    """16-byte blocks: the first 32 bytes 0xff (>= p for Fp128 and P-256: the first attempt is rejected in both prime fields), a
    second such pair further in, pseudo-random bytes elsewhere"""
    rng = random.Random(20)
    blocks = [bytes(rng.randrange(256) for _ in range(16)) for _ in range(160)]
    for i in (0, 1, 10, 11):
        blocks[i] = b"\xff" * 16
    return b"".join(blocks)


def _stage(L, field, inputs, exact, bulk_model=False):
    nb = NBYTES[field]
    stream = _stage_stream()
    nw = STAGE_NIN - STAGE_NPUB + sum(4 * lw + 3 for lw in LOGW)
    calls, ncalls = (C.c_size_t * 256)(), C.c_size_t(0)
    out, lqc, n = C.create_string_buffer(nw * nb), (C.c_size_t * (3 * len(LOGW)))(), C.c_size_t(0)
    rc = L.hzp_stage_witness(C.c_int(field), (C.c_size_t * len(LOGW))(*LOGW), C.c_size_t(len(LOGW)), C.c_size_t(STAGE_NPUB), C.c_size_t(STAGE_NIN),
                             b"".join(_enc(field, v) for v in inputs), C.c_int(exact), C.c_int(bulk_model), stream, C.c_size_t(len(stream)), calls, C.c_size_t(256),
                             C.byref(ncalls), out, lqc, C.byref(n))
    assert rc == 0 and ncalls.value <= 256
    return [int.from_bytes(out.raw[nb * i:nb * (i + 1)], "little") for i in range(nw)], list(lqc), n.value, list(calls[:ncalls.value])


@pytest.mark.parametrize("field", [GF, FP128, P256])
def test_stage_witness_exact_calls_matches_fill_pad_model(field):
    L, _ = _lib()
    rng = random.Random(300 + field)
    inputs = [_rand_elt(rng, field) for _ in range(STAGE_NIN)]
    ref = ScriptedEngine(_stage_stream())
    want, want_lqc = _fill_pad_model(field, ref, inputs, STAGE_NPUB)
    got, lqc, n, calls = _stage(L, field, inputs, exact=1)
    ndraw = sum(4 * lw + 2 for lw in LOGW)
    assert len(ref.calls) == ndraw + (0 if field == GF else 4 if field == FP128 else 2)  # the rejected attempts: 16-byte blocks 0, 1, 10, 11
    assert calls == ref.calls  # one hook call per attempt, of the reference's size
    assert got == want  # the private inputs, the draws in fill_pad's order, wc0 * wc1 computed at every lqc[3 ly + 2]
    assert lqc == want_lqc and n == len(want)


def test_stage_witness_bulk_p256_is_one_sample_many():
    L, _ = _lib()
    rng = random.Random(301)
    inputs = [_rand_elt(rng, P256) for _ in range(STAGE_NIN)]
    got = _stage(L, P256, inputs, exact=0)
    model = _stage(L, P256, inputs, exact=0, bulk_model=True)
    assert got == model
    ndraw = sum(4 * lw + 2 for lw in LOGW)
    assert got[3] == [32 * ndraw, 32 * 2]  # one bulk call, then one for the two rejected attempts
    # the accepted 32-byte chunks of one long draw are the exact-calls elements, so the staged vector is the same
    assert got[:3] == _stage(L, P256, inputs, exact=1)[:3]

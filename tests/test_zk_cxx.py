"""The C++ host driver of the ZK prover (include/lfgpu_zk.h, csrc/zk.hip).

GPU: lfgpu_zk_commit + lfgpu_zk_prove on the reference's flatsha256 circuits produce the reference's own wire bytes
(ZkProof::write, lib/zk/zk_proof.h:90-185; length + SHA-256 recorded by oracle/gen_flatsha_fixtures.py from the
real reference run with the same LCG RandomEngine and transcript seed).
CPU: the built-in transcript primitives against FIPS vectors / hashlib / the harness transcript."""
import hashlib
import json
import lzma
import os

import numpy as np
import pytest

from __graft_entry__ import load_package

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    return load_package()


@pytest.mark.parametrize("portable", [0, 1])
def test_sha256_and_aes256_known_answers(pkg, portable):
    """both the SHA-NI / AES-NI paths and the portable C++ (csrc/fs_crypto.cc)"""
    L = pkg.load_library()
    L.lfgpu_crypto_hw(portable)
    try:
        _known_answers(pkg)
        t = pkg.FsTranscript(b"prf")
        stream = t.bytes(16 * 37 + 5) + t.bytes(3) + t.bytes(64)  # bulk path, tail, refill
        t.close()
        L.lfgpu_crypto_hw(1)
        t = pkg.FsTranscript(b"prf")
        assert stream == t.bytes(len(stream))  # one call, portable cipher: same stream
        t.close()
    finally:
        L.lfgpu_crypto_hw(0)


def _known_answers(pkg):
    assert pkg.sha256(b"abc").hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"  # FIPS 180-4 B.1
    rs = np.random.RandomState(5)
    for n in (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 121, 4096, 100003):
        d = rs.bytes(n)
        assert pkg.sha256(d) == hashlib.sha256(d).digest(), n
    key = bytes(range(32))  # FIPS-197 C.3
    assert pkg.aes256_ecb_block(key, bytes.fromhex("00112233445566778899aabbccddeeff")).hex() == "8ea2b7ca516745bfeafc49904b496089"


@pytest.mark.parametrize("portable", [0, 1])
def test_host_gf2128_product_matches_oracle(pkg, portable):
    """the PCLMULQDQ product of the host bookkeeping (csrc/fs_crypto.cc) and its portable fallback vs the oracle"""
    import ctypes as C
    import oracle_lib as ol
    L = pkg.load_library()
    L.lfgpu_crypto_hw(portable)
    try:
        rng = np.random.default_rng(77)
        vals = ol.rand_elts(rng, 400)
        vals[0] = 0
        vals[1] = (1, 0)
        vals[2] = (0, 1 << 63)
        vals[3] = (2**64 - 1, 2**64 - 1)
        o = ol.oracle()
        for i in range(0, 400, 2):
            a, b = vals[i], vals[(i * 7 + 3) % 400]
            out = (C.c_uint64 * 2)()
            L.lfgpu_host_gf2128_mul((C.c_uint64 * 2)(int(a[0]), int(a[1])), (C.c_uint64 * 2)(int(b[0]), int(b[1])), out)
            want = o.lfo_gf_mul(ol.elt(a), ol.elt(b))
            assert (out[0], out[1]) == (want.l[0], want.l[1])
    finally:
        L.lfgpu_crypto_hw(0)


def test_builtin_transcript_matches_harness_transcript(pkg):
    """same byte stream as tests/fs_transcript.py (which is pinned by the reference fixtures) under interleaved
    writes and reads, including the PRF reset on every write and reads that straddle AES blocks"""
    from fs_transcript import Transcript
    a, b = Transcript(b"test"), pkg.FsTranscript(b"test")
    rs = np.random.RandomState(11)
    for step in range(60):
        op = rs.randint(4)
        if op == 0:
            d = rs.bytes(rs.randint(0, 200))
            a.write_bytes(d)
            b.write_bytes(d)
        elif op == 1:
            e = rs.bytes(16)
            a.write_elt(e)
            b.write_elt(e)
        elif op == 2:
            es = [rs.bytes(16) for _ in range(rs.randint(0, 5))]
            a.write_array(es)
            b.write_array(es)
        for _ in range(rs.randint(1, 4)):
            n = int(rs.randint(1, 50))
            assert a.bytes(n) == b.bytes(n), step
    b.close()


def _load(nb):
    raw = lzma.decompress(open(os.path.join(GOLD, "flatsha_nb%d.lfc1.xz" % nb), "rb").read())
    W = np.frombuffer(lzma.decompress(open(os.path.join(GOLD, "flatsha_nb%d.w.xz" % nb), "rb").read()), dtype=np.uint64).reshape(-1, 2).copy()
    info = json.load(open(os.path.join(GOLD, "flatsha_nb%d.json" % nb)))
    return raw, W, info


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 32])
def test_zk_cxx_driver_emits_reference_wire_bytes(nb):
    import gpu_util as G
    import ligero_fixture as lf
    raw, W, info = _load(nb)
    want = lzma.decompress(open(os.path.join(GOLD, "flatsha_nb%d.zkproof.xz" % nb), "rb").read())
    circ = G.pkg.Circuit(G.gpu(), raw)
    ci = circ.info
    assert (ci.nl, ci.ninputs, ci.npub_in, ci.nterms) == (info["nl"], info["ninputs"], info["npub_in"], info["nterms"])
    zk = G.pkg.ZkProver(G.gpu(), circ, 7, 132)
    assert (zk.param.block_enc, zk.param.nrow, zk.param.nw) == (info["zk_block_enc"], info["zk_nrow"], info["zk_nw"])
    for rep in range(2):  # the prover object is reusable: a second commit + prove gives the same proof
        ts = G.pkg.FsTranscript(b"test")
        rng = lf.LcgRng(100)
        root = zk.commit(W, rng.bytes, ts)
        assert root == want[:32]
        assert zk.prove(W, ts)
        wire = zk.wire()
        assert len(wire) == info["zk_wire_bytes"]
        assert hashlib.sha256(wire).hexdigest() == info["zk_wire_sha256"]
        ts.close()
    zk.close()
    circ.close()


@pytest.mark.gpu
def test_zk_cxx_driver_rejects_bad_witness_and_bad_circuits():
    import gpu_util as G
    import ligero_fixture as lf
    raw, W, _ = _load(1)
    gpu = G.gpu()
    # the reference reader's sanity checks (lib/proto/circuit_reader.h:104-110,161-168): subfield_boundary <= ninputs,
    # 0 < logw, logw <= nw, nq > 0
    nin = int.from_bytes(raw[16:19], "little")
    nk = int.from_bytes(raw[22:25], "little")
    lay0 = 25 + 16 * nk  # first layer header: logw, nw, nq
    sfb_big = raw[:13] + (nin + 1).to_bytes(3, "little") + raw[16:]
    logw_zero = raw[:lay0] + (0).to_bytes(3, "little") + raw[lay0 + 3:]
    nw_small = raw[:lay0] + (9).to_bytes(3, "little") + (8).to_bytes(3, "little") + raw[lay0 + 6:]
    nq_zero = raw[:lay0 + 6] + (0).to_bytes(3, "little") + raw[lay0 + 9:]
    for bad in (raw[:-1], raw[:100], b"\x02" + raw[1:], raw + b"\x00", sfb_big, logw_zero, nw_small, nq_zero):
        with pytest.raises(G.pkg.LfGpuError):
            G.pkg.Circuit(gpu, bad)
    circ = G.pkg.Circuit(gpu, raw)
    zk = G.pkg.ZkProver(gpu, circ, 7, 132)
    W2 = W.copy()
    W2[1:, 0] ^= np.uint64(1)  # break (almost) every wire: the circuit's assert-zero terms / outputs must catch it
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(W2, lf.LcgRng(100).bytes, ts)
    assert zk.prove(W2, ts) is False
    with pytest.raises(G.pkg.LfGpuError):
        zk.wire()
    ts.close()
    zk.close()
    circ.close()


def _subfield_solver():
    """GF2_128<4>::solve (lib/gf2k/gf2_128.h:496-508) in Python: coordinates of e in the basis beta, or None"""
    import ctypes as C
    import oracle_lib as ol
    ctx = ol.gf_ctx(4)
    rows = []  # (vector as int, combination mask, pivot bit)
    for i in range(16):
        v = ctx.beta[i].l[0] | (ctx.beta[i].l[1] << 64)
        comb = 1 << i
        for (rv, rc, pb) in rows:
            if (v >> pb) & 1:
                v ^= rv
                comb ^= rc
        rows.append((v, comb, v.bit_length() - 1))

    def solve(e):
        u = 0
        for (rv, rc, pb) in rows:
            if (e >> pb) & 1:
                e ^= rv
                u ^= rc
        return u if e == 0 else None

    return solve


def wire_from_components(comp, layers_logw, p, fp128=False):
    """ZkProof::write (lib/zk/zk_proof.h:90-185) from the component dump of oracle/ref_flatsha.cc (.zkproof)"""
    if fp128:  # Fp128: every element is "in the subfield" and to_bytes_subfield is the full 16-byte image
        def solve(e):
            return e
        sub_bytes = 16
    else:
        solve = _subfield_solver()
        sub_bytes = 2
    pos = 0

    def take(n):
        nonlocal pos
        b = comp[pos:pos + n]
        pos += n
        return b

    out = bytearray(take(32))
    for logw in layers_logw:
        for _ in range(logw):
            h0t0, h0t2, h1t0, h1t2 = take(16), take(16), take(16), take(16)
            out += h0t0 + h1t0 + h0t2 + h1t2
        out += take(32)
    out += take(16 * (p.block + p.dblock + p.r + (p.dblock - p.block)))
    req = take(16 * p.nrow * p.nreq)
    out += take(32 * p.nreq)  # nonces precede the opened columns on the wire
    elts = [int.from_bytes(req[16 * i:16 * i + 16], "little") for i in range(p.nrow * p.nreq)]
    ci, sub = 0, False
    while ci < len(elts):
        run = 0
        while ci + run < len(elts) and (solve(elts[ci + run]) is not None) == sub:
            run += 1
        out += run.to_bytes(4, "little")
        for e in elts[ci:ci + run]:
            out += solve(e).to_bytes(sub_bytes, "little") if sub else e.to_bytes(16, "little")
        ci += run
        sub = not sub
    npath = int.from_bytes(take(8), "little")
    out += npath.to_bytes(4, "little") + take(32 * npath)
    assert pos == len(comp)
    return bytes(out)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 32])
def test_zk_verifier_accepts_reference_and_own_proofs_rejects_tampering(nb):
    """lfgpu_zk_verify = ZkVerifier::recv_commitment + verify (lib/zk/zk_verifier.h:68-94).  The REFERENCE prover's
    proof (component fixture re-serialised to the wire format; the re-serialisation is pinned by the recorded SHA-256
    of the reference's own ZkProof::write output) and this library's proof are accepted; single-byte corruptions
    in every section of the proof are rejected."""
    import gpu_util as G
    import ligero_fixture as lf
    raw, W, info = _load(nb)
    comp = lzma.decompress(open(os.path.join(GOLD, "flatsha_nb%d.zkproof.xz" % nb), "rb").read())
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    p = G.pkg.ligero_param(G.pkg.FIELD_GF2_128, info["zk_nw"], circ.info.nl, 7, 132, 0)
    logws = [circ.layer(i)["logw"] for i in range(circ.info.nl)]
    ref_wire = wire_from_components(comp, logws, p)
    assert len(ref_wire) == info["zk_wire_bytes"] and hashlib.sha256(ref_wire).hexdigest() == info["zk_wire_sha256"]
    pub = W[:circ.info.npub_in]

    def verify(wire):
        ts = G.pkg.FsTranscript(b"test")
        r = G.pkg.zk_verify(gpu, circ, wire, pub, ts)
        ts.close()
        return r

    assert verify(ref_wire) == (True, "ok")
    # our own proof under a different RandomEngine (different pads, blinding rows and nonces)
    zk = G.pkg.ZkProver(gpu, circ, 7, 132)
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(W, lf.LcgRng(4242).bytes, ts)
    assert zk.prove(W, ts)
    own = zk.wire()
    ts.close()
    zk.close()
    assert own != ref_wire
    assert verify(own) == (True, "ok")
    # tampering: one flipped bit per section
    sc_bytes = sum((4 * l + 2) * 16 for l in logws)
    off_y = 32 + sc_bytes
    sections = {
        "root": 5,
        "sumcheck": 32 + 16 * 3 + 1,
        "y_ldt": off_y + 7,
        "y_dot": off_y + 16 * p.block + 16 * (p.r + 3) + 2,
        "y_quad": off_y + 16 * (p.block + p.dblock) + 9,
        "nonce": off_y + 16 * (p.block + p.dblock + p.r + p.dblock - p.block) + 40,
        "req": off_y + 16 * (p.block + p.dblock + p.r + p.dblock - p.block) + 32 * p.nreq + 4 + 16 * 1000 + 3,
        "path": len(own) - 11,
    }
    for name, off in sections.items():
        bad = bytearray(own)
        bad[off] ^= 0x10
        okb, why = verify(bytes(bad))
        assert not okb, name
        assert why != "ok", name
    assert verify(own[:-1]) == (False, "proof does not parse")
    assert verify(own + b"\x00")[0] in (True, False)  # trailing bytes are the caller's business (ReadBuffer is not checked for exhaustion)
    # wrong transcript seed: every challenge differs
    ts = G.pkg.FsTranscript(b"tesu")
    assert G.pkg.zk_verify(gpu, circ, own, pub, ts)[0] is False
    ts.close()
    circ.close()


@pytest.mark.gpu
def test_zk_public_inputs_and_subfield_boundary_match_reference():
    """The mdoc hash circuit's two features the flatsha benchmark circuit lacks: public inputs (bound through
    input_constraint, written to the transcript) and a subfield boundary (witness rows below it are padded with
    subfield randomness, and opened subfield elements travel as 2 bytes in runs).  Fixture: the reference run on the
    1-block circuit with npub_in = 9, subfield_boundary = 777 (oracle/gen_flatsha_fixtures.py variant)."""
    import gpu_util as G
    import ligero_fixture as lf
    raw, W, _ = _load(1)
    info = json.load(open(os.path.join(GOLD, "flatsha_nb1_pub9_sfb777.json")))
    b = bytearray(raw)
    b[1 + 9:1 + 12] = info["npub_in"].to_bytes(3, "little")          # header: version, fid, nv, nc, NPUB, SFB, ...
    b[1 + 12:1 + 15] = info["subfield_boundary"].to_bytes(3, "little")
    raw2 = bytes(b)
    assert hashlib.sha256(raw2).hexdigest() == info["lfc1_sha256"]  # exactly the bytes the reference serialised
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw2)
    assert (circ.info.npub_in, circ.info.subfield_boundary) == (9, 777)
    zk = G.pkg.ZkProver(gpu, circ, 7, 132)
    assert zk.param.nw == info["zk_nw"]
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(W, lf.LcgRng(100).bytes, ts)
    assert zk.prove(W, ts)
    wire = zk.wire()
    ts.close()
    assert len(wire) == info["zk_wire_bytes"]
    assert hashlib.sha256(wire).hexdigest() == info["zk_wire_sha256"]
    tv = G.pkg.FsTranscript(b"test")
    assert G.pkg.zk_verify(gpu, circ, wire, W[:9], tv) == (True, "ok")
    tv.close()
    pub_bad = W[:9].copy()
    pub_bad[3, 0] ^= np.uint64(1)  # a different public input: rejected
    tv = G.pkg.FsTranscript(b"test")
    assert G.pkg.zk_verify(gpu, circ, wire, pub_bad, tv)[0] is False
    tv.close()
    zk.close()
    circ.close()


@pytest.mark.gpu
def test_zk_over_fp128_matches_reference():
    """The same driver over the prime field Fp128 (field id 6): the flatsha256 circuit compiled by the reference over
    Fp128<> with ReedSolomonFactory<Fp128, FFTConvolutionFactory> (as lib/zk/zk_test.cc:252-330 sets ZK up for that
    field), LCG RandomEngine, transcript "test".  Exercises rejection sampling, Montgomery <-> wire conversions, the
    signed constraint algebra, the Fp128 sumcheck / Ligero kernels end to end, and the verifier."""
    import gpu_util as G
    import ligero_fixture as lf
    raw = lzma.decompress(open(os.path.join(GOLD, "flatsha_fp_nb1.lfc1.xz"), "rb").read())
    W = np.frombuffer(lzma.decompress(open(os.path.join(GOLD, "flatsha_fp_nb1.w.xz"), "rb").read()), dtype=np.uint64).reshape(-1, 2).copy()
    comp = lzma.decompress(open(os.path.join(GOLD, "flatsha_fp_nb1.zkproof.xz"), "rb").read())
    info = json.load(open(os.path.join(GOLD, "flatsha_fp_nb1.json")))
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    assert (circ.info.field, circ.info.nl, circ.info.nterms) == (G.pkg.FIELD_FP128, info["nl"], info["nterms"])
    zk = G.pkg.ZkProver(gpu, circ, 7, 132)
    assert (zk.param.nw, zk.param.block_enc, zk.param.nrow) == (info["zk_nw"], info["zk_block_enc"], info["zk_nrow"])
    logws = [circ.layer(i)["logw"] for i in range(circ.info.nl)]
    ref_wire = wire_from_components(comp, logws, zk.param, fp128=True)
    assert len(ref_wire) == info["zk_wire_bytes"] and hashlib.sha256(ref_wire).hexdigest() == info["zk_wire_sha256"]
    ts = G.pkg.FsTranscript(b"test")
    root = zk.commit(W, lf.LcgRng(100).bytes, ts)
    assert root == comp[:32]
    assert zk.prove(W, ts)
    wire = zk.wire()
    ts.close()
    assert wire == ref_wire
    for w in (ref_wire, wire):
        tv = G.pkg.FsTranscript(b"test")
        assert G.pkg.zk_verify(gpu, circ, w, W[:0], tv) == (True, "ok")
        tv.close()
    bad = bytearray(wire)
    bad[32 + 16 * 5 + 3] ^= 1
    tv = G.pkg.FsTranscript(b"test")
    assert G.pkg.zk_verify(gpu, circ, bytes(bad), W[:0], tv)[0] is False
    tv.close()
    zk.close()
    circ.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fp,block_enc", [(True, 8192), (True, 16384), (False, 16384), (False, 32768)])
def test_zk_prove_verify_with_explicit_large_block_enc(fp, block_enc):
    """ZkProver / ZkVerifier with a caller-chosen block_enc above the sizes the reference fixtures use (Fp128: the
    two-pass FFT inside the RS extension; GF2_128: rows larger than the LDS-resident RS kernel, further cosets through the
    batched LCH14 FFT).  The verifier's device tableau (A rows, y vectors) must survive the RS helpers' own scratch use
    (round-1 advisor finding: it used to alias the FFT pass buffer).  No reference fixture has these sizes: parity of
    the proof bytes is unpinned here; the property checked is prove -> verify accepts, tampered -> rejects."""
    import gpu_util as G
    import ligero_fixture as lf
    if fp:
        raw = lzma.decompress(open(os.path.join(GOLD, "flatsha_fp_nb1.lfc1.xz"), "rb").read())
        W = np.frombuffer(lzma.decompress(open(os.path.join(GOLD, "flatsha_fp_nb1.w.xz"), "rb").read()), dtype=np.uint64).reshape(-1, 2).copy()
    else:
        raw, W, _ = _load(1)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    zk = G.pkg.ZkProver(gpu, circ, 7, 132, block_enc)
    assert zk.param.block_enc == block_enc
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(W, lf.LcgRng(7).bytes, ts)
    assert zk.prove(W, ts)
    wire = zk.wire()
    ts.close()
    zk.close()
    pub = W[:circ.info.npub_in]
    tv = G.pkg.FsTranscript(b"test")
    assert G.pkg.zk_verify(gpu, circ, wire, pub, tv, 7, 132, block_enc) == (True, "ok")
    tv.close()
    bad = bytearray(wire)
    bad[len(bad) // 2] ^= 4
    tv = G.pkg.FsTranscript(b"test")
    assert G.pkg.zk_verify(gpu, circ, bytes(bad), pub, tv, 7, 132, block_enc)[0] is False
    tv.close()
    circ.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [2, 4, 8, 16, 33])
def test_zk_cxx_driver_wire_bytes_other_block_counts(nb):
    """the remaining sizes of BM_ShaZK_fp2_128 (reference docs/content/en/docs/benchmarks.md:55-61); 33 blocks is the
    reference's ragged case (witness and layer widths are not powers of two).  Fixtures: circuit + witness + the
    reference's commitment root and the length / SHA-256 of its ZkProof::write bytes (oracle/gen_flatsha_fixtures.py light)"""
    import gpu_util as G
    import ligero_fixture as lf
    raw, W, info = _load(nb)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    assert (circ.info.nl, circ.info.ninputs, circ.info.nterms) == (info["nl"], info["ninputs"], info["nterms"])
    zk = G.pkg.ZkProver(gpu, circ, 7, 132)
    assert (zk.param.block_enc, zk.param.nrow, zk.param.nw) == (info["zk_block_enc"], info["zk_nrow"], info["zk_nw"])
    ts = G.pkg.FsTranscript(b"test")
    root = zk.commit(W, lf.LcgRng(100).bytes, ts)
    assert root.hex() == info["zk_root"]
    assert zk.prove(W, ts)
    wire = zk.wire()
    ts.close()
    assert len(wire) == info["zk_wire_bytes"] and hashlib.sha256(wire).hexdigest() == info["zk_wire_sha256"]
    tv = G.pkg.FsTranscript(b"test")
    assert G.pkg.zk_verify(gpu, circ, wire, W[:circ.info.npub_in], tv) == (True, "ok")
    tv.close()
    zk.close()
    circ.close()


@pytest.mark.gpu
def test_zk_mdoc_hash_circuit_matches_reference():
    """BASELINE config 5, the GF2_128 half: the REAL mdoc hash circuit (kZkSpecs[0]; 17 layers, 7.76 M terms, 952 public
    inputs, subfield boundary 85112, Ligero block_enc 4151 -- not a power of two) with the witness of the reference's own
    example (mdoc_tests[0], age_over_18), proved by the library's ZK driver: wire bytes identical to the reference's
    ZkProver<GF2_128<>, LCH14ReedSolomonFactory> under the same transcript and RandomEngine (oracle/ref_mdoc.cc ->
    oracle/gen_mdoc_fixture.py), and accepted by the library's verifier.  (The signature half: the next test.)"""
    import gpu_util as G
    import ligero_fixture as lf
    info = json.load(open(os.path.join(GOLD, "mdoc.json")))["hash"]
    raw = lzma.decompress(open(os.path.join(GOLD, "mdoc_hash.lfc1.xz"), "rb").read())
    W = np.frombuffer(lzma.decompress(open(os.path.join(GOLD, "mdoc_hash.w.xz"), "rb").read()), dtype=np.uint64).reshape(-1, 2).copy()
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    ci = circ.info
    assert (ci.nl, ci.ninputs, ci.npub_in, ci.subfield_boundary, ci.nterms) == (info["nl"], info["ninputs"], info["npub_in"],
                                                                               info["subfield_boundary"], info["nterms"])
    zk = G.pkg.ZkProver(gpu, circ, info["rate"], info["nreq"], info["block_enc"])
    assert (zk.param.block_enc, zk.param.nrow, zk.param.block, zk.param.nw) == (info["block_enc"], info["nrow"], info["block"], info["nw"])
    ts = G.pkg.FsTranscript(b"test")
    root = zk.commit(W, lf.LcgRng(100).bytes, ts)
    assert root.hex() == info["zk_root"]
    assert zk.prove(W, ts)
    wire = zk.wire()
    ts.close()
    assert len(wire) == info["zk_wire_bytes"] and hashlib.sha256(wire).hexdigest() == info["zk_wire_sha256"]
    tv = G.pkg.FsTranscript(b"test")
    assert G.pkg.zk_verify(gpu, circ, wire, W[:ci.npub_in], tv, info["rate"], info["nreq"], info["block_enc"]) == (True, "ok")
    tv.close()
    pub_bad = W[:ci.npub_in].copy()
    pub_bad[5, 0] ^= np.uint64(1)
    tv = G.pkg.FsTranscript(b"test")
    assert G.pkg.zk_verify(gpu, circ, wire, pub_bad, tv, info["rate"], info["nreq"], info["block_enc"])[0] is False
    tv.close()
    zk.close()
    circ.close()


@pytest.mark.gpu
def test_zk_mdoc_signature_circuit_matches_reference():
    """BASELINE config 5, the Fp256Base half: the REAL mdoc signature circuit (kZkSpecs[0]: 21 layers of 2^9 .. 2^16 wires,
    481 833 terms, 900 public inputs, 32-byte elements; Ligero block_enc 4096, 19 rows) with the witness of the reference's
    own example, proved by the library's P-256 ZK driver (csrc/zk256.hip over csrc/p256.hip): commitment root and wire
    bytes identical to the reference's ZkProver<Fp256Base, ReedSolomonFactory<Fp256Base, FFTExtConvolutionFactory>> under
    the same transcript and RandomEngine (oracle/ref_mdoc.cc -> oracle/gen_mdoc_fixture.py); then the library's verifier for
    this field on those bytes and on tampered copies."""
    import gpu_util as G
    import ligero_fixture as lf
    info = json.load(open(os.path.join(GOLD, "mdoc.json")))
    rate, nreq = info["hash"]["rate"], info["hash"]["nreq"]
    info = info["sig"]
    raw = lzma.decompress(open(os.path.join(GOLD, "mdoc_sig.lfc1.xz"), "rb").read())
    W = np.frombuffer(lzma.decompress(open(os.path.join(GOLD, "mdoc_sig.w.xz"), "rb").read()), dtype=np.uint64).reshape(-1, 4).copy()
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    ci = circ.info
    assert ci.field == G.pkg.FIELD_P256
    assert (ci.nl, ci.ninputs, ci.npub_in, ci.subfield_boundary, ci.nterms) == (info["nl"], info["ninputs"], info["npub_in"],
                                                                               info["subfield_boundary"], info["nterms"])
    assert W.shape[0] == ci.ninputs
    zk = G.pkg.ZkProver(gpu, circ, rate, nreq, info["block_enc"])
    assert (zk.param.block_enc, zk.param.nrow, zk.param.block, zk.param.dblock, zk.param.nw) == (
        info["block_enc"], info["nrow"], info["block"], info["dblock"], info["nw"])
    for rep in range(2):  # the second run reuses the cached bind structure and tables
        ts = G.pkg.FsTranscript(b"test")
        root = zk.commit(W, lf.LcgRng(100).bytes, ts)
        assert root.hex() == info["zk_root"]
        assert zk.prove(W, ts)
        wire = zk.wire()
        ts.close()
        assert len(wire) == info["zk_wire_bytes"] and hashlib.sha256(wire).hexdigest() == info["zk_wire_sha256"]
    print("mdoc signature circuit on the device (ms):", zk.timings(), "reference, 1 CPU thread:", info["ref_commit_ms"], info["ref_prove_ms"])
    # a witness that violates the circuit: prove() returns False as the reference's does (eval_circuit fails)
    Wbad = W.copy()
    Wbad[ci.npub_in + 7, 0] ^= np.uint64(1)
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(Wbad, lf.LcgRng(100).bytes, ts)
    assert zk.prove(Wbad, ts) is False
    ts.close()
    # the library's verifier for this field (csrc/zk256.hip): accepts the proof -- which is the reference's, byte for byte --
    # and rejects a flipped bit in every section and a wrong public input, with the reference's reasons
    def verify(w, pub):
        tv = G.pkg.FsTranscript(b"test")
        try:
            return G.pkg.zk_verify(gpu, circ, w, pub, tv, rate, nreq, info["block_enc"])
        finally:
            tv.close()
    pub = W[:ci.npub_in]
    assert verify(wire, pub) == (True, "ok")
    p = zk.param
    sc_bytes = sum(4 * circ.layer(i)["logw"] + 2 for i in range(ci.nl)) * 32
    offs = {"root": 5, "sumcheck": 32 + sc_bytes // 2, "y_ldt": 32 + sc_bytes + 40, "y_dot": 32 + sc_bytes + 32 * p.block + 40,
            "y_quad": 32 + sc_bytes + 32 * (p.block + p.dblock) + 8, "nonce": 32 + sc_bytes + 32 * (p.block + 2 * p.dblock - p.w) + 3,
            "opened column": 32 + sc_bytes + 32 * (p.block + 2 * p.dblock - p.w) + 32 * p.nreq + 8 + 32 * 77, "merkle path": len(wire) - 9}
    for name, off in offs.items():
        bad = bytearray(wire)
        bad[off] ^= 0x04
        okv, why = verify(bytes(bad), pub)
        assert okv is False, name
    pub_bad = pub.copy()
    pub_bad[3, 0] ^= np.uint64(1)
    assert verify(wire, pub_bad)[0] is False
    assert verify(wire[:-5], pub) == (False, "proof does not parse")
    zk.close()
    circ.close()


@pytest.mark.gpu
def test_zk_small_p256_circuit_matches_reference():
    """The Fp256Base prover and verifier on TINY layers: the reference's own zk_test example circuit (lib/zk/zk_test.cc:250-271,
    2 n = (s - 2) m^2 - (s - 4) m; 2 layers, 4 inputs of which 2 public) compiled over the P-256 base field and proved by the
    reference's ZkProver<Fp256Base, .> with rate 4, 6 queries, block_enc chosen by LigeroParam's search (oracle/ref_small_p256.cc
    -> tests/golden/small_p256.json, `./oracle/_ref/gen_small_p256 > tests/golden/small_p256.json`): the library's wire bytes
    must be identical, its verifier must accept them and reject tampered copies; a witness with m changed does not prove.
    (Layers of 1 .. 9 variables and everything else between and beyond this toy and the signature circuit: test_zk_p256_synth.py.)"""
    import gpu_util as G
    import ligero_fixture as lf
    fx = json.load(open(os.path.join(GOLD, "small_p256.json")))
    assert fx["reference_verifier_accepts"] is True
    raw, want = bytes.fromhex(fx["lfc1"]), bytes.fromhex(fx["zk_wire"])
    W = np.frombuffer(bytes.fromhex(fx["witness"]), dtype=np.uint64).reshape(-1, 4).copy()
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    ci = circ.info
    assert (ci.field, ci.nl, ci.ninputs, ci.npub_in, ci.nv) == (G.pkg.FIELD_P256, fx["nl"], fx["ninputs"], fx["npub_in"], fx["nv"])
    zk = G.pkg.ZkProver(gpu, circ, fx["rate"], fx["nreq"], 0)
    assert (zk.param.block_enc, zk.param.nrow, zk.param.block) == (fx["block_enc"], fx["nrow"], fx["block"])
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(W, lf.LcgRng(100).bytes, ts)
    assert zk.prove(W, ts)
    wire = zk.wire()
    ts.close()
    assert wire == want and hashlib.sha256(wire).hexdigest() == fx["zk_wire_sha256"]

    def verify(w, pub):
        tv = G.pkg.FsTranscript(b"test")
        try:
            return G.pkg.zk_verify(gpu, circ, w, pub, tv, fx["rate"], fx["nreq"], 0)
        finally:
            tv.close()
    pub = W[:ci.npub_in]
    assert verify(wire, pub) == (True, "ok")
    for off in (3, 40, 200, len(wire) // 2, len(wire) - 40):
        bad = bytearray(wire)
        bad[off] ^= 1
        assert verify(bytes(bad), pub)[0] is False, off
    Wbad = W.copy()
    Wbad[2, 0] ^= np.uint64(8)  # m: the constraint no longer holds
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(Wbad, lf.LcgRng(100).bytes, ts)
    assert zk.prove(Wbad, ts) is False
    ts.close()
    zk.close()
    circ.close()


@pytest.mark.gpu
def test_zk_verify_with_commitment_received_separately():
    """ZkVerifier::recv_commitment and ::verify are two calls in the reference (lib/zk/zk_verifier.h:68-94) and the mdoc verifier
    does other transcript work between them (mdoc_zk.cc:676-681): lfgpu_zk_verify_committed is verify for a transcript that has
    already received the commitment.  Same verdict as the combined call when the caller wrote the root (write_bytes of the first
    32 proof bytes, as LigeroTranscript::write_commitment does); rejection when it did not, or wrote a different one."""
    import gpu_util as G
    import ligero_fixture as lf
    raw, W, info = _load(1)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    zk = G.pkg.ZkProver(gpu, circ, 7, 132)
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(W, lf.LcgRng(100).bytes, ts)
    assert zk.prove(W, ts)
    wire = zk.wire()
    ts.close()
    zk.close()
    assert hashlib.sha256(wire).hexdigest() == info["zk_wire_sha256"]
    pub = W[:circ.info.npub_in]

    def run(prefix, committed):
        tv = G.pkg.FsTranscript(b"test")
        try:
            if prefix is not None:
                tv.write_bytes(prefix)
            return G.pkg.zk_verify(gpu, circ, wire, pub, tv, committed=committed)
        finally:
            tv.close()
    assert run(None, False) == (True, "ok")
    assert run(wire[:32], True) == (True, "ok")
    assert run(None, True)[0] is False
    assert run(bytes(32), True)[0] is False
    assert run(wire[:32], False)[0] is False  # the root twice
    circ.close()

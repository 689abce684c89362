"""The Fp256Base prover and verifier (csrc/zk256.hip) at the shapes its two fixed circuits never reach.

The mdoc signature circuit (2^9 .. 2^16 wires per layer, one tableau shape) and the 2-layer toy of
test_zk_small_p256_circuit_matches_reference pin the paths they take and nothing between or beyond.  The fixtures here
are synthetic layered circuits compiled, proved and verified by the REAL reference (oracle/ref_synth_p256.cc ->
oracle/gen_synth_p256_fixtures.py -> tests/golden/synth_p256*): the library must produce the reference's proof bytes,
section by section, and its verifier must accept them and reject tampered copies.

  wide    70006-wire layers, 140006 hand pairs (above the resident grid's 131072), a wire read by 70000 terms, gates of
          1167 terms; rate 5, 40 queries, block_enc by LigeroParam's search
  odd     2^12 + 1 inputs, then 3 * 2^10, 5000 and 2^10 + 1 wires (odd from the start, odd midway, odd all the way); one
          hand pair shared by 4996 terms
  funnel  1 .. 9 output variables (the direct EQ kernel and the first sizes of the table split), a layer of 6 wires and
          4 hand pairs
  tall    40010 inputs in a tableau of 16384 columns, 10 public inputs, subfield boundary three witness rows in

test_fixtures_cover_the_shapes holds what the cases are FOR: a fixture regenerated with less coverage fails it."""
import hashlib
import json
import lzma
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GEN = os.path.join(ROOT, "oracle", "_ref", "gen_synth_p256")
CASES = ("wide", "odd", "funnel", "tall")
P256 = 2**256 - 2**224 + 2**192 + 2**96 - 1
G256_MAX = 131072  # csrc/zk256.hip: largest HQUAD / hand array the resident grid takes
# (rate, nreq) of the two fixed P-256 fixtures: mdoc.json "sig", small_p256.json
FIXED_RATE_NREQ = ((7, 132), (4, 6))
PARAM_FIELDS = ("nw", "nq", "rateinv", "nreq", "block_enc", "block", "dblock", "block_ext", "r", "w", "nwrow", "nqtriples",
                "nwqrow", "nrow", "mc_pathlen", "ildt", "idot", "iquad", "iw", "iq")


def records():
    recs = json.load(open(os.path.join(GOLD, "synth_p256.json")))["cases"]
    return {r["case"]: r for r in recs}


def load_case(name):
    """-> (record, LFC1 bytes, witness [ninputs, 4] uint64)"""
    rec = records()[name]
    raw = lzma.decompress(open(os.path.join(GOLD, "synth_p256_%s.lfc1.xz" % name), "rb").read())
    wb = lzma.decompress(open(os.path.join(GOLD, "synth_p256_%s.w.xz" % name), "rb").read())
    return rec, raw, np.frombuffer(wb, dtype=np.uint64).reshape(-1, 4).copy()


def read_lfc1_p256(raw):
    """the reference's LFC1 wire format (lib/proto/circuit_writer.h:39-85) with 32-byte constants ->
    dict(nv, nc, npub_in, subfield_boundary, ninputs, nl, nconst, layers=[{logw, nw, g, h0, h1, vi}])"""
    b = np.frombuffer(raw, dtype=np.uint8)
    assert b[0] == 1
    pos = 1

    def num():
        nonlocal pos
        v = int(b[pos]) | int(b[pos + 1]) << 8 | int(b[pos + 2]) << 16
        pos += 3
        return v

    _fid, nv, nc, npub, sfb, nin, nl, nk = (num() for _ in range(8))
    pos += 32 * nk
    layers = []
    for _ in range(nl):
        logw, nw, nq = num(), num(), num()
        t = b[pos:pos + 12 * nq].reshape(nq, 4, 3).astype(np.int64)
        pos += 12 * nq
        v = t[:, :, 0] | (t[:, :, 1] << 8) | (t[:, :, 2] << 16)
        idx = np.cumsum((v[:, :3] >> 1) * (1 - 2 * (v[:, :3] & 1)), axis=0)  # deltas, LSB = sign
        layers.append(dict(logw=logw, nw=nw, g=idx[:, 0], h0=idx[:, 1], h1=idx[:, 2], vi=v[:, 3]))
    assert pos + 32 == len(b)
    return dict(nv=nv, nc=nc, npub_in=npub, subfield_boundary=sfb, ninputs=nin, nl=nl, nconst=nk, layers=layers)


def elt_int(row):
    return sum(int(row[k]) << (64 * k) for k in range(4))


def test_fixtures_cover_the_shapes():
    """Every shape the cases exist for, asserted from the recorded header -- and the record itself checked against the
    circuit and witness bytes it describes (layer sizes, term counts, distinct hand pairs, fan-in and fan-out), so that
    neither a thinner regenerated fixture nor a record that drifted from its files passes."""
    recs = records()
    assert tuple(sorted(recs)) == tuple(sorted(CASES)) and 3 <= len(recs) <= 5
    gold_limit = os.path.getsize(os.path.join(GOLD, "flatsha_nb32.zkproof.xz"))
    reads_hub = 0
    for name in CASES:
        rec, raw, W = load_case(name)
        assert rec["reference_verifier_accepts"] is True, name
        for ext in (".lfc1.xz", ".w.xz"):
            assert os.path.getsize(os.path.join(GOLD, "synth_p256_" + name + ext)) <= gold_limit
        assert hashlib.sha256(raw).hexdigest() == rec["lfc1_sha256"] and hashlib.sha256(W.tobytes()).hexdigest() == rec["witness_sha256"]
        c = read_lfc1_p256(raw)
        assert (c["nl"], c["ninputs"], c["npub_in"], c["nv"], c["subfield_boundary"], c["nc"]) == \
            (rec["nl"], rec["ninputs"], rec["npub_in"], rec["nv"], rec["subfield_boundary"], 1), name
        assert W.shape == (rec["ninputs"], 4) and len(rec["layers"]) == rec["nl"]
        assert sum(l["nterms"] for l in rec["layers"]) == rec["nterms"]
        nv = c["nv"]
        for i, (l, r) in enumerate(zip(c["layers"], rec["layers"])):
            pair = l["h0"] * (1 << 24) + l["h1"]
            _, pair_counts = np.unique(pair, return_counts=True)
            reads = np.bincount(np.concatenate([l["h0"], l["h1"][l["h1"] != l["h0"]]]), minlength=l["nw"])
            got = dict(logv=max(0, (nv - 1).bit_length()), nv=nv, logw=l["logw"], nw=l["nw"], nterms=len(l["g"]), nh0=len(pair_counts),
                       max_gate_terms=int(np.bincount(l["g"]).max()), max_pair_terms=int(pair_counts.max()), max_wire_reads=int(reads.max()))
            assert got == r, (name, i)
            assert l["g"].max() < nv and l["h1"].max() < l["nw"] and l["nw"] <= 1 << l["logw"]
            nv = l["nw"]
        # the witness: wire 0 is one; the three special inputs hold 0, 1 and p - 1 (Montgomery images) and products read them
        one = elt_int(W[0])
        assert one == 2**256 % P256
        last = c["layers"][-1]
        for key, want in (("input_zero", 0), ("input_one", one), ("input_mone", P256 - one)):
            w = rec[key]
            assert 0 < w < rec["ninputs"] and elt_int(W[w]) == want, (name, key)
            in_product = ((last["h0"] == w) | (last["h1"] == w)) & (last["h0"] != 0)  # h0 <= h1; wire 0 is the constant
            assert in_product.any(), (name, key)
        reads_hub = max(reads_hub, max(r["max_wire_reads"] for r in rec["layers"]))
    L = [(n, l) for n in CASES for l in recs[n]["layers"]]
    have = lambda pred: [n for n, l in L if pred(l)]  # noqa: E731
    for logv in (3, 4, 5, 6, 7, 8):  # the direct EQ kernel below 6, the first sizes of the table split (lb != hb at 7) from 6 on
        assert have(lambda l: l["logv"] == logv), logv
    assert have(lambda l: l["nv"] > 1 << 16)
    assert have(lambda l: l["nw"] > 1 << 16)
    assert have(lambda l: l["nh0"] > G256_MAX)
    assert have(lambda l: l["nh0"] > l["nw"]) and have(lambda l: l["nh0"] < l["nw"])
    pow2 = lambda n: n > 0 and n & (n - 1) == 0  # noqa: E731
    assert have(lambda l: l["nw"] - 1 >= 1 << 10 and pow2(l["nw"] - 1))  # 2^k + 1, k >= 10: odd through every halving
    assert have(lambda l: l["nw"] % 3 == 0 and pow2(l["nw"] // 3))  # 3 * 2^j: odd after j halvings
    assert have(lambda l: l["nw"] % 2 == 0 and not pow2(l["nw"]))  # even, not a power of two
    assert have(lambda l: l["nh0"] <= 4 and l["logw"] >= 3)
    assert have(lambda l: l["max_gate_terms"] > 1024) and have(lambda l: l["max_pair_terms"] > 1024)
    assert reads_hub >= 1 << 16
    assert [r for r in recs.values() if r["npub_in"] > 0 and r["subfield_boundary"] > 0]
    assert [r for r in recs.values() if r["ligero_param"]["block_enc"] >= 16384]
    fixed_rates, fixed_nreqs = zip(*FIXED_RATE_NREQ)
    assert [r for r in recs.values() if r["rate"] not in fixed_rates and r["nreq"] not in fixed_nreqs and r["block_enc_arg"] == 0]
    for r in recs.values():  # the recorded sections tile the proof
        off = 0
        for s in r["sections"]:
            assert s["offset"] == off and s["bytes"] > 0
            off += s["bytes"]
        assert off == r["zk_wire_bytes"]
        assert [s["name"] for s in r["sections"]] == ["root"] + ["sumcheck_layer_%d" % i for i in range(r["nl"])] + \
            ["y_ldt", "y_dot", "y_quad_0", "y_quad_2", "nonces", "opened_columns", "merkle_path"]
        assert r["sections"][0]["sha256"] == hashlib.sha256(bytes.fromhex(r["zk_root"])).hexdigest()


def test_fixtures_regenerate_byte_identical():
    """Where the reference generator has been built (oracle/Makefile `ref`), it reproduces the committed fixtures: the
    circuit and witness bytes inside the .xz files and every recorded value."""
    if not os.path.exists(GEN):
        pytest.skip("oracle/_ref/gen_synth_p256 is not built (the reference is not on this machine)")
    assert tuple(subprocess.check_output([GEN, "--list"], text=True).split()) == CASES
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            subprocess.run([GEN, name, tmp], check=True, stdout=subprocess.DEVNULL, timeout=600)
            stem = os.path.join(tmp, "synth_p256_" + name)
            rec, raw, W = load_case(name)
            assert open(stem + ".lfc1", "rb").read() == raw, name
            assert open(stem + ".w", "rb").read() == W.tobytes(), name
            assert json.load(open(stem + ".json")) == rec, name


def _verify(G, gpu, circ, rec, wire, pub):
    tv = G.pkg.FsTranscript(b"test")
    try:
        return G.pkg.zk_verify(gpu, circ, wire, pub, tv, rec["rate"], rec["nreq"], rec["block_enc_arg"])
    finally:
        tv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_zk_synth_p256_matches_reference(name):
    """Through the prover-level ABI, as test_zk_small_p256_circuit_matches_reference: header and LigeroParam as the reference
    computed them, its commitment root, its proof bytes -- every section of ZkProof::write on its own first, so that a
    mismatch names the sumcheck layer or the Ligero part -- twice on one ZkProver (the bind offsets cached at the first proof,
    the self-cleaning accumulators); the verifier accepts them and rejects a flipped bit in every section, a changed public
    input; a witness with one private input changed does not prove."""
    import gpu_util as G
    import ligero_fixture as lf
    rec, raw, W = load_case(name)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    ci = circ.info
    assert (ci.field, ci.nl, ci.ninputs, ci.npub_in, ci.nv, ci.logv, ci.subfield_boundary, ci.nterms, ci.nc) == \
        (G.pkg.FIELD_P256, rec["nl"], rec["ninputs"], rec["npub_in"], rec["nv"], rec["logv"], rec["subfield_boundary"], rec["nterms"], 1)
    for i, l in enumerate(rec["layers"]):
        assert circ.layer(i) == dict(logw=l["logw"], nw=l["nw"], nterms=l["nterms"]), i
    zk = G.pkg.ZkProver(gpu, circ, rec["rate"], rec["nreq"], rec["block_enc_arg"])
    assert {f: getattr(zk.param, f) for f in PARAM_FIELDS} == rec["ligero_param"]
    wires = []
    for rep in range(2):
        ts = G.pkg.FsTranscript(b"test")
        root = zk.commit(W, lf.LcgRng(rec["rng_seed"]).bytes, ts)
        assert root.hex() == rec["zk_root"], rep
        assert zk.prove(W, ts) is True, rep
        wire = zk.wire()
        ts.close()
        for s in rec["sections"]:  # before the length (the Merkle path's varies with the challenges): the first section that differs is named
            assert hashlib.sha256(wire[s["offset"]:s["offset"] + s["bytes"]]).hexdigest() == s["sha256"], (rep, s["name"])
        assert len(wire) == rec["zk_wire_bytes"], rep
        assert hashlib.sha256(wire).hexdigest() == rec["zk_wire_sha256"], rep
        wires.append(wire)
    assert wires[0] == wires[1]
    pub = W[:ci.npub_in]
    assert _verify(G, gpu, circ, rec, wire, pub) == (True, "ok")
    for s in rec["sections"]:  # one offset inside every recorded section
        bad = bytearray(wire)
        bad[s["offset"] + s["bytes"] // 2] ^= 0x04
        assert _verify(G, gpu, circ, rec, bytes(bad), pub)[0] is False, s["name"]
    pub_bad = pub.copy()
    pub_bad[ci.npub_in - 1, 1] ^= np.uint64(1)
    assert _verify(G, gpu, circ, rec, wire, pub_bad)[0] is False
    Wbad = W.copy()
    Wbad[ci.npub_in + 7, 0] ^= np.uint64(1)  # a private data input that products read
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(Wbad, lf.LcgRng(rec["rng_seed"]).bytes, ts)
    assert zk.prove(Wbad, ts) is False
    ts.close()
    # and the prover is not left in a state: the good witness proves to the same bytes again
    ts = G.pkg.FsTranscript(b"test")
    zk.commit(W, lf.LcgRng(rec["rng_seed"]).bytes, ts)
    assert zk.prove(W, ts) is True
    assert zk.wire() == wire
    ts.close()
    zk.close()
    circ.close()

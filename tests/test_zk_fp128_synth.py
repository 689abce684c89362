"""The Fp128 prover and verifier (csrc/zk.hip and the kernels under it, compiled for LFC1 field id 6) at the shapes the one
reference circuit of that field, flatsha_fp_nb1, never reaches.  (test_zk_p256_synth.py does the same for Fp256Base,
test_zk_gf_synth.py for GF(2^128).)

That circuit has 684 .. 24546 wires per layer, at least 684 hand pairs everywhere, no public input and one tableau shape
(block_enc 4096, rate 7, 132 queries).  The fixtures here are synthetic layered circuits compiled, proved and verified by
the REAL reference (oracle/ref_synth_fp128.cc -> oracle/gen_synth_p256_fixtures.py fp128 -> tests/golden/synth_fp128*):
the library must produce the reference's proof bytes, section by section, and its verifier must accept them and reject
tampered copies.

  wide    two layers of 263006 wires (not a power of two) with 526006 hand pairs each: two round-hands on the whole-GPU
          per-launch kernels before the resident grid's hand-off point of 131072; a wire read by 263000 terms, gates of
          4384 terms; rate 5, 40 queries, block_enc by LigeroParam's search
  odd     2^12 + 1 inputs, then 3 * 2^10, 5000 and 2^10 + 1 wires (odd from the start, odd midway, odd all the way); one
          hand pair shared by 4996 terms
  funnel  9 .. 2 and 0 output variables (the direct EQ kernel below 6), layers that start within one wave (50, 24, 12, 6
          and 4 wires; 4 and 2 hand pairs); rate 4, 6 queries
  tall    40010 inputs in a tableau of 16384 columns (two-pass FFT plan), 10 public inputs, begin_full_field() three
          witness rows in
  long    3003 inputs in a tableau of 2^18 columns: the RS encode of the commitment runs the Fp128 FFT at 2^18 points
          (2^20, the size of fp_fft_tile_1024x4_tws, took this test 9.5 s and is left to test_fp128_twside.py);
          two outputs (the one output variable the funnel cannot hold: under a single output lie three wires)

test_fixtures_cover_the_shapes holds what the cases are FOR: a fixture regenerated with less coverage fails it.

The rejection branch of elt_sample (a draw >= p, about 2^-20 per draw) is reached by test_verifier_checks.py, which splices such
draws into a scripted transcript; the same file makes each check of the verifier the one that refuses, with its exact reason."""
import hashlib
import json
import lzma
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle_lib import SC_GRID_MAX as GRID_MAX
from synth_fixture import elt_int, read_lfc1_16 as read_lfc1_fp128

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GEN = os.path.join(ROOT, "oracle", "_ref", "gen_synth_fp128")
CASES = ("wide", "odd", "funnel", "tall", "long")
P128 = 2**128 - 2**108 + 1
FIXED_RATE_NREQ = (7, 132)  # of flatsha_fp_nb1, the one other Fp128 reference circuit
PARAM_FIELDS = ("nw", "nq", "rateinv", "nreq", "block_enc", "block", "dblock", "block_ext", "r", "w", "nwrow", "nqtriples",
                "nwqrow", "nrow", "mc_pathlen", "ildt", "idot", "iquad", "iw", "iq")


def records():
    recs = json.load(open(os.path.join(GOLD, "synth_fp128.json")))["cases"]
    return {r["case"]: r for r in recs}


def load_case(name):
    """-> (record, LFC1 bytes, witness [ninputs, 2] uint64)"""
    rec = records()[name]
    raw = lzma.decompress(open(os.path.join(GOLD, "synth_fp128_%s.lfc1.xz" % name), "rb").read())
    wb = lzma.decompress(open(os.path.join(GOLD, "synth_fp128_%s.w.xz" % name), "rb").read())
    return rec, raw, np.frombuffer(wb, dtype=np.uint64).reshape(-1, 2).copy()


def test_fixtures_cover_the_shapes():
    """Every shape the cases exist for, asserted from the recorded header -- and the record itself checked against the
    circuit and witness bytes it describes (layer sizes, term counts, distinct hand pairs, fan-in and fan-out), so that
    neither a thinner regenerated fixture nor a record that drifted from its files passes."""
    recs = records()
    assert tuple(sorted(recs)) == tuple(sorted(CASES))
    gold_limit = os.path.getsize(os.path.join(GOLD, "flatsha_nb32.zkproof.xz"))
    for name in CASES:
        rec, raw, W = load_case(name)
        assert rec["reference_verifier_accepts"] is True, name
        for ext in (".lfc1.xz", ".w.xz"):
            assert os.path.getsize(os.path.join(GOLD, "synth_fp128_" + name + ext)) <= gold_limit
        assert hashlib.sha256(raw).hexdigest() == rec["lfc1_sha256"] and hashlib.sha256(W.tobytes()).hexdigest() == rec["witness_sha256"]
        assert len(raw) == rec["lfc1_bytes"]
        c = read_lfc1_fp128(raw)
        assert (c["fid"], c["nl"], c["ninputs"], c["npub_in"], c["nv"], c["subfield_boundary"], c["nc"], c["nconst"]) == \
            (6, rec["nl"], rec["ninputs"], rec["npub_in"], rec["nv"], rec["subfield_boundary"], 1, rec["nconst"]), name
        assert W.shape == (rec["ninputs"], 2) and len(rec["layers"]) == rec["nl"]
        top = np.uint64(P128 >> 64)  # p = top * 2^64 + 1: every image is a value below p
        assert ((W[:, 1] < top) | ((W[:, 1] == top) & (W[:, 0] == 0))).all()
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
            assert l["g"].min() >= 0 and l["h0"].min() >= 0 and (l["h0"] <= l["h1"]).all() and l["vi"].max() < c["nconst"]
            nv = l["nw"]
        assert nv == rec["ninputs"]
        # the witness: wire 0 is one; the three special inputs hold 0, 1 and p - 1 (Montgomery images) and products read them
        one = elt_int(W[0])
        assert one == 2**128 % P128
        last = c["layers"][-1]
        for key, want in (("input_zero", 0), ("input_one", one), ("input_mone", P128 - one)):
            w = rec[key]
            assert 0 < w < rec["ninputs"] and elt_int(W[w]) == want, (name, key)
            in_product = ((last["h0"] == w) | (last["h1"] == w)) & (last["h0"] != 0)  # h0 <= h1; wire 0 is the constant
            assert in_product.any(), (name, key)
        # the private input whose change must break the proof (test_zk_synth_fp128_matches_reference) is read by a product
        w = rec["npub_in"] + 7
        assert (((last["h0"] == w) | (last["h1"] == w)) & (last["h0"] != 0)).any() and elt_int(W[w]) not in (0, P128 - 1), name
    L = [(n, l) for n in CASES for l in recs[n]["layers"]]
    have = lambda pred: [n for n, l in L if pred(l)]  # noqa: E731
    pow2 = lambda n: n > 0 and n & (n - 1) == 0  # noqa: E731
    # above the grid's hand-off point, in wires and in hand pairs, in one layer; the fixture goes beyond twice that, so that
    # TWO round-hands (hand 0 and hand 1 of the first round) run on the per-launch kernels before the hand-off
    assert have(lambda l: l["nw"] > GRID_MAX and l["nh0"] > GRID_MAX and not pow2(l["nw"]))
    assert have(lambda l: l["nw"] > 2 * GRID_MAX and l["nh0"] > 2 * GRID_MAX and not pow2(l["nw"]))
    assert have(lambda l: l["nw"] > GRID_MAX and l["max_wire_reads"] >= 1 << 16)
    assert have(lambda l: l["nw"] - 1 >= 1 << 10 and pow2(l["nw"] - 1))  # 2^k + 1, k >= 10: odd through every halving
    assert have(lambda l: l["nw"] % 3 == 0 and pow2(l["nw"] // 3))  # 3 * 2^j: odd after j halvings
    assert have(lambda l: l["nw"] % 2 == 0 and not pow2(l["nw"]))  # even, not a power of two
    for logv in range(10):  # the direct EQ kernel below 6, the first sizes of the table split from 6 on
        assert have(lambda l: l["logv"] == logv), logv
    assert have(lambda l: l["nv"] == 1)
    assert have(lambda l: l["nw"] <= 64)  # starts on the single-wave tail
    assert have(lambda l: l["nw"] <= 8 and l["nh0"] <= 4)
    assert have(lambda l: l["max_wire_reads"] >= 1 << 16)
    assert have(lambda l: l["max_gate_terms"] > 1024) and have(lambda l: l["max_pair_terms"] > 1024)
    # public inputs beyond wire 0 (five data inputs and the outputs), in the tallest tableau, full-field mark set
    assert [r for r in recs.values() if r["npub_in"] >= 1 + 5 + r["noutput_inputs"] and r["first_output_input"] < r["npub_in"] and
            r["ninputs"] >= 40000 and r["npub_in"] < r["subfield_boundary"] < r["ninputs"] and r["ligero_param"]["nwrow"] > 3 and
            r["block_enc_arg"] == 16384]
    assert [r for r in recs.values() if r["ligero_param"]["block_enc"] >= 16384]
    assert [r for r in recs.values() if r["ligero_param"]["block_enc"] >= 1 << 18 and r["rate"] == 4 and r["nreq"] <= 20]
    assert [r for r in recs.values() if r["rate"] != FIXED_RATE_NREQ[0] and r["nreq"] != FIXED_RATE_NREQ[1] and r["block_enc_arg"] == 0]
    for r in recs.values():  # the recorded sections tile the proof
        assert r["ligero_param"]["rateinv"] == r["rate"] and r["ligero_param"]["nreq"] == r["nreq"]
        assert r["block_enc_arg"] in (0, r["ligero_param"]["block_enc"])
        off = 0
        for s in r["sections"]:
            assert s["offset"] == off and s["bytes"] > 0
            off += s["bytes"]
        assert off == r["zk_wire_bytes"]
        assert [s["name"] for s in r["sections"]] == ["root"] + ["sumcheck_layer_%d" % i for i in range(r["nl"])] + \
            ["y_ldt", "y_dot", "y_quad_0", "y_quad_2", "nonces", "opened_columns", "merkle_path"]
        sec = {s["name"]: s["bytes"] for s in r["sections"]}
        assert [sec["sumcheck_layer_%d" % i] for i in range(r["nl"])] == [(4 * l["logw"] + 2) * 16 for l in r["layers"]]
        assert (sec["y_ldt"], sec["y_dot"]) == (16 * r["ligero_param"]["block"], 16 * r["ligero_param"]["dblock"])
        assert r["sections"][0]["sha256"] == hashlib.sha256(bytes.fromhex(r["zk_root"])).hexdigest()


def test_fixtures_regenerate_byte_identical():
    """Where the reference generator has been built (oracle/Makefile `ref`), it reproduces the committed fixtures: the
    circuit and witness bytes inside the .xz files and every recorded value."""
    if not os.path.exists(GEN):
        pytest.skip("oracle/_ref/gen_synth_fp128 is not built (the reference is not on this machine)")
    assert tuple(subprocess.check_output([GEN, "--list"], text=True).split()) == CASES
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            subprocess.run([GEN, name, tmp], check=True, stdout=subprocess.DEVNULL, timeout=600)
            stem = os.path.join(tmp, "synth_fp128_" + name)
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
def test_zk_synth_fp128_matches_reference(name):
    """Through the prover-level ABI, as test_zk_over_fp128_matches_reference: header and LigeroParam as the reference
    computed them, its commitment root, its proof bytes -- every section of ZkProof::write on its own first, so that a
    mismatch names the sumcheck layer or the Ligero part -- twice on one ZkProver (the bind offsets cached at the first proof,
    the self-cleaning accumulators); the verifier accepts them and rejects a flipped bit in every section, a changed public
    input and (tall) an element of y_ldt that is not below p; a witness with one private input changed does not prove."""
    import gpu_util as G
    import ligero_fixture as lf
    rec, raw, W = load_case(name)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    ci = circ.info
    assert (ci.field, ci.nl, ci.ninputs, ci.npub_in, ci.nv, ci.logv, ci.subfield_boundary, ci.nterms, ci.nc) == \
        (G.pkg.FIELD_FP128, rec["nl"], rec["ninputs"], rec["npub_in"], rec["nv"], rec["logv"], rec["subfield_boundary"], rec["nterms"], 1)
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
    pub_bad[ci.npub_in - 1, 1] ^= np.uint64(1)  # wire 0, or (tall) the last public output
    assert _verify(G, gpu, circ, rec, wire, pub_bad)[0] is False
    if name == "tall":  # 2^128 - 1 >= p is no element: of_bytes_field refuses it, the proof does not parse (never reduced mod p)
        s = {s["name"]: s for s in rec["sections"]}["y_ldt"]
        bad = bytearray(wire)
        at = s["offset"] + 16 * (s["bytes"] // 32)
        bad[at:at + 16] = b"\xff" * 16
        assert _verify(G, gpu, circ, rec, bytes(bad), pub) == (False, "proof does not parse")
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

"""The GF(2^128) prover and verifier (csrc/zk.hip and the kernels under it, compiled for LFC1 field id 4) at the shapes
the SHA circuits of that field -- flatsha_nb{1..33}, the mdoc hash circuit -- never reach.

Those circuits have bit-valued witnesses, three tableau shapes (block 455, 461 or 910, block_enc 4096, 4151 or 8192: every
commit takes the LDS-resident mixed-row encoder) and subfield boundaries 0, 777 and 85112.  The fixtures here are
synthetic layered circuits compiled, proved and verified by the REAL reference (oracle/ref_synth_gf.cc ->
oracle/gen_synth_p256_fixtures.py gf -> tests/golden/synth_gf*): the library must produce the reference's proof bytes,
section by section, and its verifier must accept them and reject tampered copies.

  wide    two layers of 263006 wires (not a power of two), the upper with 526006 hand pairs: two round-hands on the
          whole-GPU per-launch kernels before the resident grid's hand-off point of 131072; a wire read by 263001 terms and
          a hand pair shared by 263000, gates of 4384 terms; rate 5, 40 queries, block_enc 1024 by LigeroParam's search
  odd     2^12 + 1 inputs, then 3 * 2^10, 5000 and 2^10 + 1 wires; begin_full_field() exactly three witness rows in
          (subfield_boundary - npub_in == 3 w, the edge of `(i + 1) * w <= subfield_boundary`), a full-field value right
          after it
  funnel  9 .. 2 and 0 output variables (the direct EQ kernel below 6), layers of 50, 24, 12, 6 and 4 wires (4 and 2 hand
          pairs); rate 4, 6 queries: block 21 in 128 columns (LCH14 plans of fewer than 7 levels)
  tall    120010 inputs in 36 rows of 24581 columns: block 4097 and dblock 8193 are beyond the LDS-resident encoder, and the
          33 rows after IQUAD go through gf_rs_rows_big in one call of >= 32 rows, its bit-sliced tower variant; 10 public
          inputs; begin_full_field() 9000 inputs in: two subfield-only rows, a mixed row, 27 full rows, so the opened
          columns hold a full-field run, a two-byte run and a full-field run
  long    3003 inputs in 7 rows of 65535 columns, the most GF2_128<4> admits (evaluation points must exist in the 16-bit
          subfield): the plain variant of gf_rs_rows_big, the last LCH14 coset partial for block and for dblock; two
          outputs (one output variable)

test_fixtures_cover_the_shapes holds what the cases are FOR: a fixture regenerated with less coverage fails it.

The opened columns of a proof have at most ONE two-byte run: the subfield-only rows are a prefix of the witness rows, every
other row is blinded with full-field randomness, and req is stored row by row (ligero_param.h:349), so the runs are
[3 nreq, s nreq, (nrow - 3 - s) nreq] for s subfield-only rows.  The test asserts exactly that for every case; "more
than one subfield run" cannot be produced by a legal witness.

GPU time per case on an MI355X (test_zk_synth_gf_matches_reference, five proofs and the tampered verifications each):
  wide 0.3 s (1.9 s as the first test of a process, with the context's start-up), odd 0.10 s, long 0.10 s, tall 0.06 s,
  funnel 0.02 s (the reference generator: 13 s for wide on the CPU, under 0.3 s for each of the others)

Not reached: a rejection branch of GF sampling does not exist (every 16-byte or 2-byte draw is an element)."""
import hashlib
import json
import lzma
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle_lib import SC_GRID_MAX as GRID_MAX
from synth_fixture import GfSubfield, elt_int, read_lfc1_16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GEN = os.path.join(ROOT, "oracle", "_ref", "gen_synth_gf")
CASES = ("wide", "odd", "funnel", "tall", "long")
GF = 4  # FieldID GF2_128_ID
FIXED_RATE_NREQ = (7, 132)  # of every SHA fixture of this field
ERR_ARG = 1  # LFGPU_ERR_ARG
PARAM_FIELDS = ("nw", "nq", "rateinv", "nreq", "block_enc", "block", "dblock", "block_ext", "r", "w", "nwrow", "nqtriples",
                "nwqrow", "nrow", "mc_pathlen", "ildt", "idot", "iquad", "iw", "iq")


def records():
    recs = json.load(open(os.path.join(GOLD, "synth_gf.json")))["cases"]
    return {r["case"]: r for r in recs}


_loaded = {}


def load_case(name):
    """-> (record, LFC1 bytes, witness [ninputs, 2] uint64, a copy); decompressed once per process"""
    if name not in _loaded:
        raw = lzma.decompress(open(os.path.join(GOLD, "synth_gf_%s.lfc1.xz" % name), "rb").read())
        wb = lzma.decompress(open(os.path.join(GOLD, "synth_gf_%s.w.xz" % name), "rb").read())
        _loaded[name] = (records()[name], raw, np.frombuffer(wb, dtype=np.uint64).reshape(-1, 2))
    rec, raw, W = _loaded[name]
    return rec, raw, W.copy()


def opened(rec):
    return {s["name"]: s for s in rec["sections"]}["opened_columns"]


def pow2(n):
    return n > 0 and n & (n - 1) == 0


def test_fixtures_cover_the_shapes():
    """Every shape the cases exist for, asserted from the recorded header -- and the record itself checked against the
    circuit and witness bytes it describes (layer sizes, term counts, distinct hand pairs, fan-in and fan-out: in
    characteristic 2 a product that occurs twice in a gate is gone from the compiled circuit), so that neither a thinner
    regenerated fixture nor a record that drifted from its files passes."""
    recs = records()
    sub = GfSubfield()
    assert tuple(sorted(recs)) == tuple(sorted(CASES))
    gold_limit = os.path.getsize(os.path.join(GOLD, "flatsha_nb32.zkproof.xz"))
    for name in CASES:
        rec, raw, W = load_case(name)
        assert rec["reference_verifier_accepts"] is True, name
        for ext in (".lfc1.xz", ".w.xz"):
            assert os.path.getsize(os.path.join(GOLD, "synth_gf_" + name + ext)) <= gold_limit
        assert hashlib.sha256(raw).hexdigest() == rec["lfc1_sha256"] and hashlib.sha256(W.tobytes()).hexdigest() == rec["witness_sha256"]
        assert len(raw) == rec["lfc1_bytes"]
        c = read_lfc1_16(raw)
        assert (c["fid"], c["nl"], c["ninputs"], c["npub_in"], c["nv"], c["subfield_boundary"], c["nc"], c["nconst"]) == \
            (GF, rec["nl"], rec["ninputs"], rec["npub_in"], rec["nv"], rec["subfield_boundary"], 1, rec["nconst"]), name
        assert W.shape == (rec["ninputs"], 2) and len(rec["layers"]) == rec["nl"]
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
        # the witness: wire 0 is one; the three special inputs hold 0, 1 and of_scalar(0xffff) and products read them
        assert elt_int(W[0]) == 1
        last = c["layers"][-1]
        for key, want in (("input_zero", 0), ("input_one", 1), ("input_ones", sub.of_scalar(0xffff))):
            w = rec[key]
            assert 0 < w < rec["ninputs"] and elt_int(W[w]) == want, (name, key)
            in_product = ((last["h0"] == w) | (last["h1"] == w)) & (last["h0"] != 0)  # h0 <= h1; wire 0 is the constant
            assert in_product.any(), (name, key)
        # the private input whose change must break the proof (test_zk_synth_gf_matches_reference) is read by a product
        w = rec["npub_in"] + 7
        assert (((last["h0"] == w) | (last["h1"] == w)) & (last["h0"] != 0)).any() and elt_int(W[w]) not in (0, 1), name
        # the boundary as LigeroProver::commit gets it; every private input below it lies in the subfield, as that
        # function demands (ligero_prover.h:63-66), and -- where there is a boundary -- the input AT it does not
        npub, sfb, p = rec["npub_in"], rec["subfield_boundary"], rec["ligero_param"]
        assert rec["ligero_subfield_boundary"] == max(0, sfb - npub)
        if sfb:
            for v in np.unique(W[npub:sfb], axis=0):
                assert sub.contains(elt_int(v)), name
            assert npub < sfb < rec["ninputs"] and not sub.contains(elt_int(W[sfb])), name
        # the run structure of the opened columns, from the reference's wire bytes: alternating 16-byte and 2-byte runs
        oc = opened(rec)
        assert oc["bytes"] == 4 * len(oc["runs"]) + 16 * oc["full"] + 2 * oc["sub"], name
        assert (sum(oc["runs"][0::2]), sum(oc["runs"][1::2])) == (oc["full"], oc["sub"]) and oc["full"] + oc["sub"] == p["nrow"] * p["nreq"]
        s = rec["ligero_subfield_boundary"] // p["w"]  # subfield-only rows: (i + 1) * w <= boundary
        assert oc["runs"] == ([3 * p["nreq"], s * p["nreq"], (p["nrow"] - 3 - s) * p["nreq"]] if s else [p["nrow"] * p["nreq"]]), name
    L = {n: recs[n]["layers"] for n in CASES}
    P = {n: recs[n]["ligero_param"] for n in CASES}
    have = lambda n, pred: [l for l in L[n] if pred(l)]  # noqa: E731
    # wide
    r = recs["wide"]
    assert have("wide", lambda l: l["nw"] > 2 * GRID_MAX and l["nh0"] > 2 * GRID_MAX and not pow2(l["nw"]))
    assert have("wide", lambda l: l["nw"] > GRID_MAX and l["max_wire_reads"] >= 1 << 16)
    assert have("wide", lambda l: l["max_gate_terms"] > 1024) and have("wide", lambda l: l["max_pair_terms"] > 1024)
    assert r["rate"] != FIXED_RATE_NREQ[0] and r["nreq"] != FIXED_RATE_NREQ[1] and r["block_enc_arg"] == 0
    # odd
    r = recs["odd"]
    assert r["ninputs"] == (1 << 12) + 1 and [l["nw"] for l in L["odd"]][-4:] == [(1 << 10) + 1, 5000, 3 << 10, (1 << 12) + 1]
    j, rem = divmod(r["ligero_subfield_boundary"], P["odd"]["w"])
    assert j >= 1 and rem == 0 and j < P["odd"]["nwrow"]
    # funnel
    r = recs["funnel"]
    assert {l["logv"] for l in L["funnel"]} >= set(range(2, 10)) | {0}
    assert have("funnel", lambda l: l["nv"] == 1) and have("funnel", lambda l: l["nw"] <= 64)
    assert have("funnel", lambda l: l["nw"] <= 8 and l["nh0"] <= 4)
    assert r["block_enc_arg"] == 0 and P["funnel"]["block"] <= 128 and (r["rate"], r["nreq"]) != FIXED_RATE_NREQ
    # tall: both row lengths beyond the LDS-resident encoder (4096); lig::extend_slab encodes the rows after IQUAD in one call
    # of nrow - 3 rows, and gf_rs_rows_big takes its tower variant from 32 rows on
    r, p = recs["tall"], P["tall"]
    assert r["block_enc_arg"] == p["block_enc"] and p["block"] > 4096 and p["nrow"] >= 32 and p["nrow"] - p["iw"] >= 32
    assert r["npub_in"] >= 1 + 5 + r["noutput_inputs"] and r["first_output_input"] < r["npub_in"]
    j, rem = divmod(r["ligero_subfield_boundary"], p["w"])
    assert j >= 2 and rem != 0 and p["nwrow"] >= j + 2  # >= 2 subfield-only rows, a mixed row, >= 1 full row
    oc = opened(r)
    assert len(oc["runs"][0::2]) > 1 and oc["sub"] > 0 and all(n > 0 for n in oc["runs"])
    # long: the largest block_enc of the field; few rows: the plain variant; the last coset partial for both row lengths
    r, p = recs["long"], P["long"]
    assert r["block_enc_arg"] == p["block_enc"] == (1 << 16) - 1 and p["nrow"] < 32
    for n in (p["block"], p["dblock"]):
        fftn = 1 << (n - 1).bit_length()
        assert n > 4096 and p["block_enc"] > fftn and p["block_enc"] % fftn != 0
    assert r["noutput_inputs"] == 2 and L["long"][0]["logv"] == 1
    # across the cases
    for logv in range(10):  # the direct EQ kernel below 6, the first sizes of the table split from 6 on
        assert [n for n in CASES for l in L[n] if l["logv"] == logv], logv
    assert [n for n in CASES for l in L[n] if l["nw"] % 2 == 0 and not pow2(l["nw"])]
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
        pytest.skip("oracle/_ref/gen_synth_gf is not built (the reference is not on this machine)")
    assert tuple(subprocess.check_output([GEN, "--list"], text=True).split()) == CASES
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            subprocess.run([GEN, name, tmp], check=True, stdout=subprocess.DEVNULL, timeout=600)
            stem = os.path.join(tmp, "synth_gf_" + name)
            rec, raw, W = load_case(name)
            assert open(stem + ".lfc1", "rb").read() == raw, name
            assert open(stem + ".w", "rb").read() == W.tobytes(), name
            assert json.load(open(stem + ".json")) == rec, name


# ---------------------------------------------------------------- the subfield check and the parameter limit (host only)
def test_commit_refuses_a_full_field_witness_below_the_subfield_boundary():
    """LigeroProver::commit's check (ligero_prover.h:63-66) in the host layout every commit path shares, through
    lfgpu_ligero_layout_rows (no device): a legal witness is laid out; a full-field value at subfield_boundary - 1 fails
    with LFGPU_ERR_ARG before a single byte is drawn; the same value AT the boundary is legal.  Fp128 has no proper
    subfield: the same call over that field goes through."""
    import importlib

    from __graft_entry__ import load_package
    pkg = load_package()
    par = importlib.import_module("longfellow_zk_amd.parallel")
    lib = pkg.load_library()
    sub = GfSubfield()
    nw, sfb = 700, 333  # the boundary inside the third of five witness rows (w = 158)
    p = pkg.ligero_param(GF, nw, 0, 4, 12, 1024)
    assert p.w < sfb and sfb % p.w and p.nwrow == 5
    rng = np.random.default_rng(7)
    W = rng.integers(0, 2**64, size=(nw, 2), dtype=np.uint64)
    for i in range(sfb):
        e = sub.of_scalar(int(rng.integers(0, 1 << 16)))
        W[i] = (e & (2**64 - 1), e >> 64)
    W[5], W[6] = (0, 0), (1, 0)
    full = W[sfb].copy()
    assert not sub.contains(elt_int(full)) and all(sub.contains(elt_int(v)) for v in W[:sfb])
    drawn = [0]

    def engine(n):
        drawn[0] += n
        return bytes(n)

    def layout(field, Wx):
        drawn[0] = 0
        return par.layout_rows(lib, field, 4, p, Wx, sfb, [], engine, 0, p.nrow)[0]

    rows = layout(GF, W)
    assert drawn[0] > 0 and (rows[p.iw:p.iw + p.nwrow, p.r:p.r + p.w].reshape(-1, 2)[:nw] == W).all()
    bad = W.copy()
    bad[sfb - 1] = full
    with pytest.raises(RuntimeError, match="failed with code %d" % ERR_ARG):
        layout(GF, bad)
    assert drawn[0] == 0, "the refused call drew from the RandomEngine"
    first = W.copy()  # and at index 0, the other end of the range
    first[0] = full
    with pytest.raises(RuntimeError, match="failed with code %d" % ERR_ARG):
        layout(GF, first)
    ok = W.copy()
    ok[sfb] = W[sfb + 1]
    ok[sfb + 1] = full
    layout(GF, ok)
    assert drawn[0] > 0
    q = pkg.ligero_param(pkg.FIELD_FP128, nw, 0, 4, 12, 1024)
    Wp = bad.copy()
    Wp[:, 1] &= np.uint64(0x7FFFFFFFFFFFFFFF)  # images below p
    par.layout_rows(lib, pkg.FIELD_FP128, 4, q, Wp, sfb, [], engine, 0, q.nrow)


def test_ligero_param_limit_of_the_16_bit_subfield():
    """LigeroParam::layout rejects block_enc >= 2^16 for GF2_128<4> (ligero_param.h:197-202): 65535 lays out as the
    reference recorded it for `long`, 65536 is LFGPU_ERR_ARG, and the search never returns such a value"""
    import ctypes as C

    from __graft_entry__ import load_package
    pkg = load_package()
    recs = records()
    want = recs["long"]["ligero_param"]
    p = pkg.ligero_param(GF, want["nw"], want["nq"], want["rateinv"], want["nreq"], 65535)
    assert {f: getattr(p, f) for f in PARAM_FIELDS} == want
    q = pkg.LigeroParam()
    lib = pkg.load_library()
    assert lib.lfgpu_ligero_param_init(C.byref(q), GF, 4, want["nw"], want["nq"], want["rateinv"], want["nreq"], 65536) == ERR_ARG
    assert lib.lfgpu_ligero_param_init(C.byref(q), GF, 4, want["nw"], want["nq"], want["rateinv"], want["nreq"], 65535) == 0
    for name in ("tall", "wide"):
        t = recs[name]["ligero_param"]
        for rate, nreq in ((t["rateinv"], t["nreq"]), (7, 132), (2, 1000)):
            s = pkg.ligero_param(GF, t["nw"], t["nq"], rate, nreq, 0)
            assert 0 < s.block_enc < 1 << 16 and pow2(s.block_enc), (name, rate, nreq)
    assert pkg.ligero_param(pkg.FIELD_FP128, want["nw"], want["nq"], want["rateinv"], want["nreq"], 65536).block_enc == 65536  # GF only


# ---------------------------------------------------------------- the prover
def _verify(G, gpu, circ, rec, wire, pub):
    tv = G.pkg.FsTranscript(b"test")
    try:
        return G.pkg.zk_verify(gpu, circ, wire, pub, tv, rec["rate"], rec["nreq"], rec["block_enc_arg"])
    finally:
        tv.close()


def _prove(G, zk, W, rec):
    """commit + prove with the fixture's seeds -> (root, wire bytes or None where the witness does not prove)"""
    import ligero_fixture as lf
    ts = G.pkg.FsTranscript(b"test")
    try:
        root = zk.commit(W, lf.LcgRng(rec["rng_seed"]).bytes, ts)
        return root, (zk.wire() if zk.prove(W, ts) else None)
    finally:
        ts.close()


def _check_wire(rec, root, wire, what):
    assert root.hex() == rec["zk_root"], what
    assert wire is not None, what
    for s in rec["sections"]:  # before the length (the Merkle path's varies with the challenges): the first section that differs is named
        assert hashlib.sha256(wire[s["offset"]:s["offset"] + s["bytes"]]).hexdigest() == s["sha256"], (what, s["name"])
    assert len(wire) == rec["zk_wire_bytes"], what
    assert hashlib.sha256(wire).hexdigest() == rec["zk_wire_sha256"], what


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_zk_synth_gf_matches_reference(name):
    """Through the prover-level ABI: header and LigeroParam as the reference computed them, its commitment root, its proof
    bytes -- every section of ZkProof::write on its own first, so that a mismatch names the sumcheck layer or the Ligero
    part -- twice on one ZkProver; the verifier accepts them and rejects a flipped bit in every section and a changed
    public input; a witness with one private input changed does not prove, and the good one then proves to the same bytes.
    tall: the two-byte runs of the opened columns tampered with, every offset computed from the recorded run list."""
    import gpu_util as G
    rec, raw, W = load_case(name)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    ci = circ.info
    assert (ci.field, ci.nl, ci.ninputs, ci.npub_in, ci.nv, ci.logv, ci.subfield_boundary, ci.nterms, ci.nc) == \
        (G.pkg.FIELD_GF2_128, rec["nl"], rec["ninputs"], rec["npub_in"], rec["nv"], rec["logv"], rec["subfield_boundary"], rec["nterms"], 1)
    for i, l in enumerate(rec["layers"]):
        assert circ.layer(i) == dict(logw=l["logw"], nw=l["nw"], nterms=l["nterms"]), i
    zk = G.pkg.ZkProver(gpu, circ, rec["rate"], rec["nreq"], rec["block_enc_arg"])
    assert {f: getattr(zk.param, f) for f in PARAM_FIELDS} == rec["ligero_param"]
    wires = []
    for rep in range(2):
        root, wire = _prove(G, zk, W, rec)
        _check_wire(rec, root, wire, rep)
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
    if name == "tall":
        oc = opened(rec)
        r0, r1, r2 = oc["runs"]  # 16-byte, 2-byte, 16-byte elements, a 4-byte length in front of each
        len0, len1 = oc["offset"], oc["offset"] + 4 + 16 * r0
        sub0, len2 = len1 + 4, len1 + 4 + 2 * r1
        assert len2 + 4 + 16 * r2 == oc["offset"] + oc["bytes"]
        assert [int.from_bytes(wire[at:at + 4], "little") for at in (len0, len1, len2)] == [r0, r1, r2]
        bad = bytearray(wire)  # (a) another element of the subfield in an opened column: the column hash differs
        bad[sub0 + 2 * (r1 // 2) + 1] ^= 0x10
        assert _verify(G, gpu, circ, rec, bytes(bad), pub)[0] is False
        bad = bytearray(wire)  # (b) the boundary between the runs moved by one element, the bytes as they were
        bad[len1:len1 + 4] = (r1 - 1).to_bytes(4, "little")
        bad[len2:len2 + 4] = (r2 + 1).to_bytes(4, "little")
        assert _verify(G, gpu, circ, rec, bytes(bad), pub)[0] is False
        for at in (len0, len1, len2):  # (c) kMaxRunLen is no run length (zk_proof.h:312)
            bad = bytearray(wire)
            bad[at:at + 4] = (1 << 25).to_bytes(4, "little")
            assert _verify(G, gpu, circ, rec, bytes(bad), pub) == (False, "proof does not parse"), at
        for cut in (sub0 + r1, sub0 + r1 + 1):  # (d) the wire ends inside the two-byte run, between and within elements
            assert _verify(G, gpu, circ, rec, wire[:cut], pub) == (False, "proof does not parse"), cut
    Wbad = W.copy()
    Wbad[ci.npub_in + 7, 0] ^= np.uint64(1)  # a private data input that products read (+ 1: it stays in the subfield)
    assert _prove(G, zk, Wbad, rec)[1] is None
    # and the prover is not left in a state: the good witness proves to the same bytes again
    assert _prove(G, zk, W, rec) == (root, wire)
    zk.close()
    circ.close()


@pytest.mark.gpu
def test_zk_commit_refuses_a_full_field_input_below_the_boundary():
    """odd: the full-field value that stands right after the boundary, moved one input down.  ZkProver.commit and
    ZkBatch.commit (both reach lig::layout) fail with LFGPU_ERR_ARG naming the index -- of the Ligero witness, which
    starts at the first private input -- after the pads are drawn, as in the reference; the same objects then commit and
    prove the good witness to the reference's bytes."""
    import gpu_util as G
    import ligero_fixture as lf
    rec, raw, W = load_case("odd")
    sfb, npub = rec["subfield_boundary"], rec["npub_in"]
    Wbad = W.copy()
    Wbad[sfb - 1] = W[sfb]
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    provers = [G.pkg.ZkProver(gpu, circ, rec["rate"], rec["nreq"], rec["block_enc_arg"]) for _ in range(2)]
    msg = r"lfgpu error %d: .*not in subfield: W\[%d\]" % (ERR_ARG, sfb - 1 - npub)
    ts = G.pkg.FsTranscript(b"test")
    with pytest.raises(G.pkg.LfGpuError, match=msg):
        provers[0].commit(Wbad, lf.LcgRng(rec["rng_seed"]).bytes, ts)
    ts.close()
    _check_wire(rec, *_prove(G, provers[0], W, rec), "after the refused commit")
    batch = G.pkg.ZkBatch(gpu, circ, 2)
    tss = [G.pkg.FsTranscript(b"test") for _ in range(2)]
    with pytest.raises(G.pkg.LfGpuError, match=msg + r".*\(statement 1\)"):
        batch.commit(provers, [W, Wbad], [lf.LcgRng(rec["rng_seed"]).bytes for _ in range(2)], tss)
    for t in tss:
        t.close()
    tss = [G.pkg.FsTranscript(b"test") for _ in range(2)]
    roots = batch.commit(provers, [W, W], [lf.LcgRng(rec["rng_seed"]).bytes for _ in range(2)], tss)
    assert batch.prove(provers, [W, W], tss) == [True, True]
    for b in range(2):
        _check_wire(rec, roots[b], provers[b].wire(), "batch statement %d" % b)
    for t in tss:
        t.close()
    batch.close()
    for zk in provers:
        zk.close()
    circ.close()

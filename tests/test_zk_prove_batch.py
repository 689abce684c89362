"""lfgpu_zk_prove_batch: B committed provers of one circuit through one chain of dispatches (batched eval_circuit, one
lfgpu_sumcheck_layer_batch per layer with the batched bind_g, then constraints and Ligero prove per statement).

The reference for every statement is the unchanged single path in the same process: a second ZkProver, the same seeds,
lfgpu_zk_prove.  Statement 0 runs with the fixture's seeds, so its bytes are also pinned by the fixture's zk_wire_sha256
(the REAL reference's proof).  The other statements differ in RandomEngine seed and transcript seed: pads, challenges and
roots differ.  Every batched proof is also verified.

Below the prover: lfgpu_eval_quad_batch against the oracle's eval_quad per statement, and the batched bind_g of
lfgpu_sumcheck_layer_batch against lfgpu_sumcheck_layer at the sizes where the EQ kernel changes its scheme."""
import hashlib
import json
import lzma
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import FP, GF, P
from test_sumcheck_layer_random import make_layer_vec
from test_zk_fp128_synth import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ---------------------------------------------------------------- circuits and seeds
def _flatsha(variant):
    """-> (LFC1 bytes, witness, dict(rate, nreq, block_enc, rng_seed, sha))"""
    raw = lzma.decompress(open(os.path.join(GOLD, "flatsha_nb1.lfc1.xz"), "rb").read())
    W = np.frombuffer(lzma.decompress(open(os.path.join(GOLD, "flatsha_nb1.w.xz"), "rb").read()), dtype=np.uint64).reshape(-1, 2).copy()
    if variant == "flatsha_nb1":
        info = json.load(open(os.path.join(GOLD, "flatsha_nb1.json")))
    else:  # as test_zk_public_inputs_and_subfield_boundary_match_reference loads it
        info = json.load(open(os.path.join(GOLD, "flatsha_nb1_pub9_sfb777.json")))
        b = bytearray(raw)
        b[1 + 9:1 + 12] = info["npub_in"].to_bytes(3, "little")
        b[1 + 12:1 + 15] = info["subfield_boundary"].to_bytes(3, "little")
        raw = bytes(b)
        assert hashlib.sha256(raw).hexdigest() == info["lfc1_sha256"]
    return raw, W, dict(rate=7, nreq=132, block_enc=0, rng_seed=100, sha=info["zk_wire_sha256"])


def _synth(name):
    """an Fp128 case of test_zk_fp128_synth.py, or with the prefix "gf " a GF(2^128) case of test_zk_gf_synth.py"""
    if name.startswith("gf "):
        from test_zk_gf_synth import load_case as load_gf
        rec, raw, W = load_gf(name[3:])
    else:
        rec, raw, W = load_case(name)
    return raw, W, dict(rate=rec["rate"], nreq=rec["nreq"], block_enc=rec["block_enc_arg"], rng_seed=rec["rng_seed"], sha=rec["zk_wire_sha256"])


def load(case):
    return _flatsha(case) if case.startswith("flatsha") else _synth(case)


def seeds(par, b):
    """statement 0: the fixture's; the others: another RandomEngine seed and another transcript seed"""
    return (par["rng_seed"], b"test") if b == 0 else (par["rng_seed"] + 7919 * b, b"test %d" % b)


_single = {}


def want_single(case, b, circ, W, par):
    """lfgpu_zk_prove on a prover of its own with statement b's seeds, once per (case, b)"""
    import gpu_util as G
    import ligero_fixture as lf
    if (case, b) not in _single:
        rs, tss = seeds(par, b)
        zk = G.pkg.ZkProver(G.gpu(), circ, par["rate"], par["nreq"], par["block_enc"])
        ts = G.pkg.FsTranscript(tss)
        root = zk.commit(W, lf.LcgRng(rs).bytes, ts)
        assert zk.prove(W, ts) is True
        _single[(case, b)] = (root, zk.wire(), ts.bytes(32))
        ts.close()
        zk.close()
    return _single[(case, b)]


def commit_all(provers, Ws, par):
    import gpu_util as G
    import ligero_fixture as lf
    tss, roots = [], []
    for b, zk in enumerate(provers):
        rs, seed = seeds(par, b)
        ts = G.pkg.FsTranscript(seed)
        roots.append(zk.commit(Ws[b], lf.LcgRng(rs).bytes, ts))
        tss.append(ts)
    return tss, roots


def check_batch(case, B, nb_max=None):
    import gpu_util as G
    raw, W, par = load(case)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    provers = [G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(B)]
    batch = G.pkg.ZkBatch(gpu, circ, nb_max or B)
    tss, roots = commit_all(provers, [W] * B, par)
    assert batch.prove(provers, [W] * B, tss) == [True] * B
    wires = [zk.wire() for zk in provers]
    assert hashlib.sha256(wires[0]).hexdigest() == par["sha"], "statement 0 vs the reference's proof"
    for b in range(B):
        root, wire, after = want_single(case, b, circ, W, par)
        assert roots[b] == root and wires[b][:32] == root, b
        assert wires[b] == wire, "statement %d vs lfgpu_zk_prove" % b
        assert tss[b].bytes(32) == after, "statement %d: the transcript is not where lfgpu_zk_prove leaves it" % b
        tv = G.pkg.FsTranscript(seeds(par, b)[1])
        assert G.pkg.zk_verify(gpu, circ, wires[b], W[:circ.info.npub_in], tv, par["rate"], par["nreq"], par["block_enc"]) == (True, "ok"), b
        tv.close()
    assert len(set(wires)) == B  # the statements differ
    t0, t1 = provers[0].timings(), provers[B - 1].timings()
    assert (t0["eval_circuit"], t0["sumcheck"], t0["prove"]) == (t1["eval_circuit"], t1["sumcheck"], t1["prove"]) and t0["sumcheck"] > 0
    for ts in tss:
        ts.close()
    batch.close()
    for zk in provers:
        zk.close()
    circ.close()


# ---------------------------------------------------------------- the prover
CASES = [("flatsha_nb1", 3), ("flatsha_nb1_pub9_sfb777", 2), ("funnel", 3), ("funnel", 64), ("odd", 3), ("wide", 2), ("gf funnel", 64), ("gf odd", 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,B", CASES, ids=["%s-B%d" % c for c in CASES])
def test_batch_equals_single_path_and_reference(case, B):
    check_batch(case, B)


@pytest.mark.gpu
def test_batch_of_one_equals_the_single_call_in_a_larger_batch_object():
    check_batch("flatsha_nb1", 1, nb_max=4)


@pytest.mark.gpu
def test_bad_witness_in_one_slot_leaves_the_others_alone():
    """slot 1 of 3 holds the broken witness of test_zk_cxx_driver_rejects_bad_witness_and_bad_circuits"""
    import gpu_util as G
    case = "flatsha_nb1"
    raw, W, par = load(case)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    W2 = W.copy()
    W2[1:, 0] ^= np.uint64(1)
    provers = [G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(3)]
    batch = G.pkg.ZkBatch(gpu, circ, 3)
    Ws = [W, W2, W]
    tss, _ = commit_all(provers, Ws, par)
    assert batch.prove(provers, Ws, tss) == [True, False, True]
    for b in (0, 2):
        _, wire, after = want_single(case, b, circ, W, par)
        assert provers[b].wire() == wire and tss[b].bytes(32) == after, b
    with pytest.raises(G.pkg.LfGpuError):
        provers[1].wire()
    for ts in tss:
        ts.close()
    # the same objects, all three with the good witness
    tss, _ = commit_all(provers, [W] * 3, par)
    assert batch.prove(provers, [W] * 3, tss) == [True] * 3
    for b in range(3):
        assert provers[b].wire() == want_single(case, b, circ, W, par)[1], b
    for ts in tss:
        ts.close()
    batch.close()
    for zk in provers:
        zk.close()
    circ.close()


@pytest.mark.gpu
def test_argument_errors():
    import gpu_util as G
    import importlib
    par_mod = importlib.import_module("longfellow_zk_amd.parallel")
    case = "funnel"
    raw, W, par = load(case)
    gpu = G.gpu()
    circ, circ2 = G.pkg.Circuit(gpu, raw), G.pkg.Circuit(gpu, raw)
    mk = lambda c: G.pkg.ZkProver(gpu, c, par["rate"], par["nreq"], par["block_enc"])  # noqa: E731
    provers = [mk(circ) for _ in range(3)]
    foreign, fresh = mk(circ2), mk(circ)
    batch = G.pkg.ZkBatch(gpu, circ, 2)
    tss, _ = commit_all(provers + [foreign], [W] * 4, par)
    for bad in ([], provers[:3], [provers[0], foreign], [provers[0], fresh], [provers[0], provers[0]]):
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):  # LFGPU_ERR_ARG
            batch.prove(bad, [W] * len(bad), tss[:len(bad)])
    for nb_max in (0, G.pkg.SC_BATCH_MAX + 1):
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):
            G.pkg.ZkBatch(gpu, circ, nb_max)

    class Comm:  # a one-rank communicator: its hooks are never reached
        def __init__(self):
            self.fns = (par_mod.AG_FN(lambda *a: 1), par_mod.A2A_FN(lambda *a: 1), par_mod.BC_FN(lambda *a: 1))
            self.ops = par_mod.CommOps(None, 0, 1, *self.fns)

    provers[1].set_comm(Comm())
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 3:"):  # LFGPU_ERR_UNSUPPORTED
        batch.prove(provers[:2], [W] * 2, tss[:2])
    provers[1].set_comm(None)
    # the context and the batch are usable afterwards (the transcripts above were not touched by the refused calls)
    assert batch.prove(provers[:2], [W] * 2, tss[:2]) == [True, True]
    for b in range(2):
        assert provers[b].wire() == want_single(case, b, circ, W, par)[1], b
    # a P-256 circuit is proved one statement at a time
    fx = json.load(open(os.path.join(GOLD, "small_p256.json")))
    c256 = G.pkg.Circuit(gpu, bytes.fromhex(fx["lfc1"]))
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 3:"):
        G.pkg.ZkBatch(gpu, c256, 2)
    c256.close()
    for ts in tss:
        ts.close()
    batch.close()
    for zk in provers + [foreign, fresh]:
        zk.close()
    circ.close()
    circ2.close()


# ---------------------------------------------------------------- lfgpu_eval_quad_batch
@pytest.mark.gpu
@pytest.mark.parametrize("field", [GF, FP])
def test_eval_quad_batch_matches_oracle_per_statement(field):
    """301 outputs (two blocks), 1021 wires at a stride of 1027; 40 assert-zero terms, one violated in statement 1 only"""
    import torch

    import gpu_util as G
    o = ol.oracle()
    rng = np.random.default_rng(4100 + field)
    B, nv, nw, ldw, ldv = 3, 301, 1021, 1027, 305
    L = make_layer_vec(rng, field, 9, 10, 3000, nv=nv, nw=nw)
    az = rng.choice(L["n"], size=40, replace=False)
    L["vi"][az] = 0
    Ws = [ol.rand_elts(rng, nw, field) for _ in range(B)]
    for W in Ws:
        W[W[:, 0] == 0, 0] = 1  # no wire is zero by chance ...
        W[L["h0"][az]] = 0      # ... and every assert-zero term has a zero hand
    t = int(az[0])  # statement 1: both hands of one assert-zero term are non-zero
    Ws[1][L["h0"][t], 0] |= np.uint64(1)
    Ws[1][L["h1"][t], 0] |= np.uint64(1)
    want, want_ok = [], []
    for W in Ws:
        V = np.zeros((nv, 2), dtype=np.uint64)
        want_ok.append(bool(o.lfo_eval_quad(field, L["n"], P(L["g"]), P(L["h0"]), P(L["h1"]), P(L["vi"]), P(L["kvec"]), nv, P(W), P(V))))
        want.append(V)
    assert want_ok == [True, False, True]
    Wb = np.full((B, ldw, 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for b in range(B):
        Wb[b, :nw] = Ws[b]
    q = G.pkg.Quad(G.gpu(), field, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], nv)
    dW = G.to_dev(Wb)
    dV = torch.full((B * ldv * 16,), 0x5A, dtype=torch.uint8, device="cuda")
    assert q.eval_batch(B, nw, dW.data_ptr(), ldw, dV.data_ptr(), ldv) == [True, False, True]
    got = G.from_dev(dV, np.uint64, (B, ldv, 2))
    for b in (0, 2):
        assert (got[b, :nv] == want[b]).all(), b
    assert (got[:, nv:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()  # nothing is written between the statements
    for bad in (dict(nb=0), dict(nb=65), dict(ldw=nw - 1), dict(ldv=nv - 1), dict(nw=int(max(L["h0"].max(), L["h1"].max())))):
        a = dict(nb=B, nw=nw, ldw=ldw, ldv=ldv)
        a.update(bad)
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):
            q.eval_batch(a["nb"], a["nw"], dW.data_ptr(), a["ldw"], dV.data_ptr(), a["ldv"])
    q.close()
    kvec = np.zeros((len(L["kvec"]), 4), dtype=np.uint64)
    kvec[:, 0] = np.arange(len(kvec))
    q = G.pkg.Quad(G.gpu(), G.pkg.FIELD_P256, L["g"], L["h0"], L["h1"], L["vi"], kvec, nv)
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 3:"):
        q.eval_batch(B, nw, dW.data_ptr(), ldw, dV.data_ptr(), ldv)
    q.close()


# ---------------------------------------------------------------- the batched bind_g at the EQ scheme boundaries
# logv: (logw, terms, nv, nw).  0: no output variable; 5: the last size of the direct product; 6: the first of the factor
# tables; 17: beyond the 2^16 entries the single call's one-launch kernel stops at (65539 outputs: 257 blocks, an odd tail)
BIND_SHAPES = {0: (3, 6, 1, 5), 5: (6, 200, 29, 50), 6: (6, 300, 61, 60), 17: (8, 3000, (1 << 16) + 3, 201)}


def _tup(e):
    return tuple(int(x) for x in e)


@pytest.mark.gpu
@pytest.mark.parametrize("field", [GF, FP])
@pytest.mark.parametrize("logv", sorted(BIND_SHAPES))
def test_batched_bind_g_equals_the_single_layer(field, logv):
    import gpu_util as G
    B = 3
    logw, nterms, nv, nw = BIND_SHAPES[logv]
    rng = np.random.default_rng(5200 + 10 * logv + field)
    L = make_layer_vec(rng, field, logv, logw, nterms, 9, nv, nw)
    L["vi"][::7] = 0  # assert-zero terms: they carry the statement's beta
    st = [dict(W=ol.rand_elts(rng, nw, field), G0=ol.rand_elts(rng, max(1, logv), field), G1=ol.rand_elts(rng, max(1, logv), field),
               alpha=_tup(ol.rand_elts(rng, 1, field)[0]), beta=_tup(ol.rand_elts(rng, 1, field)[0]),
               wc_in=[_tup(e) for e in ol.rand_elts(rng, 2, field)], chal=[_tup(e) for e in ol.rand_elts(rng, 2 * logw, field)]) for _ in range(B)]
    q = G.pkg.Quad(G.gpu(), field, L["g"], L["h0"], L["h1"], L["vi"], L["kvec"], nv)
    want = []
    for s in st:
        ev = []

        def cb(hand, rnd, e, s=s, ev=ev):
            ev.append(tuple(_tup(x) for x in e))
            return s["chal"][len(ev) - 1]

        wc, ch, bq = q.sumcheck_layer(logv, s["G0"], s["G1"], s["alpha"], s["beta"], logw, nw, G.to_dev(s["W"]).data_ptr(), s["wc_in"], cb)
        want.append((ev, [_tup(w) for w in wc], _tup(bq)))
    ldw = nw + 3
    Wb = np.zeros((B, ldw, 2), dtype=np.uint64)
    for b in range(B):
        Wb[b, :nw] = st[b]["W"]
    G0 = np.concatenate([s["G0"][:logv] for s in st]) if logv else np.zeros((1, 2), dtype=np.uint64)
    G1 = np.concatenate([s["G1"][:logv] for s in st]) if logv else np.zeros((1, 2), dtype=np.uint64)
    got = [[] for _ in range(B)]
    ncall = [0]

    def cbb(hand, rnd, evals):
        for b in range(B):
            got[b].append(tuple(_tup(x) for x in evals[b]))
        ncall[0] += 1
        return [st[b]["chal"][ncall[0] - 1] for b in range(B)]

    for rep in range(2):  # twice: the side clears leave the accumulators ready for the next layer on this context
        for g in got:
            del g[:]
        ncall[0] = 0
        wc, ch, bq = q.sumcheck_layer_batch(logv, G0, G1, [s["alpha"] for s in st], [s["beta"] for s in st], logw, nw, G.to_dev(Wb).data_ptr(), ldw,
                                            [s["wc_in"] for s in st], cbb)
        for b in range(B):
            assert (got[b], [_tup(w) for w in wc[b]], _tup(bq[b])) == want[b], (rep, b)
    q.close()


# ---------------------------------------------------------------- the C++ example
@pytest.mark.gpu
def test_cxx_example_check_mode():
    from test_zk_batch_abi import build_example
    exe = build_example()
    raw, W, _ = load("flatsha_nb1")
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "c.lfc1"), "wb").write(raw)
        open(os.path.join(tmp, "w.bin"), "wb").write(W.tobytes())
        out = subprocess.run([exe, os.path.join(tmp, "c.lfc1"), os.path.join(tmp, "w.bin"), "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["B"] == 3 and res["batch_equals_sequential"] is True and res["bench_passes"] == 0

"""lfgpu_zk_prove_batch256: B committed provers of one Fp256Base circuit through one chain of dispatches (batched eval_circuit,
one sumcheck_layer_batch256 per layer, then the constraints per statement, one EQ launch chain, one
lfgpu_ligero_prove_batch256 and one lfgpu_ligero_open_batch256).

No tolerances: everything is compared byte for byte.  The expected values come from the REAL reference's recorded
zk_wire_sha256 of tests/golden/synth_p256.json (statement 0 runs with the fixture's seeds) and from the unchanged single path
in the same process (a second ZkProver, the same seeds, lfgpu_zk_prove) for every statement.  The cases are the small shapes
where the lock-step can go wrong:
  funnel B=3   logv = 0, layers of 4 .. 400 wires: every round-hand below the 2048 bound of the one-launch step, the EQ kernel at
               its direct sizes, a layer with 4 hand pairs
  funnel B=64  LFGPU_SC_BATCH_MAX: the 2 KiB challenge argument block and the full mailbox
  odd    B=3   odd wire counts at every layer, a hand pair shared by 4996 terms: crosses the 2048 hand-off inside a layer
  tall   B=2   10 public inputs (the single read-back of the tables' public parts), subfield boundary inside the witness, a
               40 000-element dense block, block_enc_arg = 16384
  funnel B=1   in a batch object of nb_max = 4"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_zk_p256_synth import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "LFGPU_LIGERO_PROVE_BATCH256"


def load(case):
    """-> (LFC1 bytes, witness [ninputs, 4], dict(rate, nreq, block_enc, rng_seed, sha))"""
    rec, raw, W = load_case(case)
    return raw, W, dict(rate=rec["rate"], nreq=rec["nreq"], block_enc=rec["block_enc_arg"], rng_seed=rec["rng_seed"], sha=rec["zk_wire_sha256"])


def seeds(par, b):
    """statement 0: the fixture's; the others: another RandomEngine seed and another transcript seed"""
    return (par["rng_seed"], b"test") if b == 0 else (par["rng_seed"] + 7919 * b, b"test %d" % b)


_single = {}


def want_single(case, b, circ, W, par, nreq=None):
    """lfgpu_zk_prove on a prover of its own with statement b's seeds, once per (case, b, nreq) -> (root, wire, transcript after)"""
    import gpu_util as G
    import ligero_fixture as lf
    nreq = par["nreq"] if nreq is None else nreq
    if (case, b, nreq) not in _single:
        rs, tss = seeds(par, b)
        zk = G.pkg.ZkProver(G.gpu(), circ, par["rate"], nreq, par["block_enc"])
        ts = G.pkg.FsTranscript(tss)
        root = zk.commit(W, lf.LcgRng(rs).bytes, ts)
        assert zk.prove(W, ts) is True
        _single[(case, b, nreq)] = (root, zk.wire(), ts.bytes(32))
        ts.close()
        zk.close()
    return _single[(case, b, nreq)]


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
    assert circ.info.field == G.pkg.FIELD_P256
    provers = [G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(B)]
    batch = G.pkg.ZkBatch256(gpu, circ, nb_max or B)
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
    t = [zk.timings() for zk in provers]
    for k in ("eval_circuit", "sumcheck", "prove", "constraints", "ligero_prove"):  # the batch's phase times, for every member
        assert len({x[k] for x in t}) == 1, k
    assert t[0]["sumcheck"] > 0 and t[0]["ligero_prove"] > 0
    for ts in tss:
        ts.close()
    batch.close()
    for zk in provers:
        zk.close()
    circ.close()


CASES = [("funnel", 3), ("funnel", 64), ("odd", 3), ("tall", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,B", CASES, ids=["%s-B%d" % c for c in CASES])
def test_batch_equals_single_path_and_reference(case, B):
    check_batch(case, B)


@pytest.mark.gpu
def test_batch_of_one_equals_the_single_call_in_a_larger_batch_object():
    check_batch("funnel", 1, nb_max=4)


@pytest.mark.gpu
def test_bad_witness_in_one_slot_leaves_the_others_alone():
    """slot 1 of 3 holds a witness with one private input changed (the one test_zk_synth_p256_matches_reference breaks)"""
    import gpu_util as G
    case = "funnel"
    raw, W, par = load(case)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    W2 = W.copy()
    W2[circ.info.npub_in + 7, 0] ^= np.uint64(1)
    provers = [G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(3)]
    batch = G.pkg.ZkBatch256(gpu, circ, 3)
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
def test_mixed_ligero_parameters_take_the_per_statement_tail():
    """provers of one circuit with two different nreq: a valid batch (the sumcheck does not look at LigeroParam), but the tableaux
    differ in shape, so constraints, Ligero prove and opening run per statement: the same bytes"""
    import gpu_util as G
    case = "funnel"
    raw, W, par = load(case)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    nreqs = [par["nreq"], par["nreq"] + 3, par["nreq"]]
    provers = [G.pkg.ZkProver(gpu, circ, par["rate"], n, par["block_enc"]) for n in nreqs]
    assert provers[0].param.nreq != provers[1].param.nreq
    batch = G.pkg.ZkBatch256(gpu, circ, 3)
    tss, roots = commit_all(provers, [W] * 3, par)
    assert batch.prove(provers, [W] * 3, tss) == [True] * 3
    for b in range(3):
        root, wire, after = want_single(case, b, circ, W, par, nreqs[b])
        assert roots[b] == root and provers[b].wire() == wire and tss[b].bytes(32) == after, b
        tv = G.pkg.FsTranscript(seeds(par, b)[1])
        assert G.pkg.zk_verify(gpu, circ, wire, W[:circ.info.npub_in], tv, par["rate"], nreqs[b], par["block_enc"]) == (True, "ok"), b
        tv.close()
    t0, t2 = provers[0].timings(), provers[2].timings()
    assert (t0["eval_circuit"], t0["sumcheck"], t0["prove"]) == (t2["eval_circuit"], t2["sumcheck"], t2["prove"])
    for ts in tss:
        ts.close()
    batch.close()
    for zk in provers:
        zk.close()
    circ.close()


class _UnsizedTranscript:
    """a transcript whose hooks lack write_elt_sized / write_elt_array_sized (what a caller built for the 16-byte fields has)"""

    def __init__(self, ts):
        self.ts = ts

    def ops(self):
        o = self.ts.ops()
        o.write_elt_sized = None
        o.write_elt_array_sized = None
        return o


@pytest.mark.gpu
def test_argument_errors():
    import importlib

    import gpu_util as G
    par_mod = importlib.import_module("longfellow_zk_amd.parallel")
    case = "funnel"
    raw, W, par = load(case)
    gpu = G.gpu()
    circ, circ2 = G.pkg.Circuit(gpu, raw), G.pkg.Circuit(gpu, raw)
    mk = lambda c: G.pkg.ZkProver(gpu, c, par["rate"], par["nreq"], par["block_enc"])  # noqa: E731
    provers = [mk(circ) for _ in range(3)]
    foreign, fresh = mk(circ2), mk(circ)
    batch = G.pkg.ZkBatch256(gpu, circ, 2)
    tss, _ = commit_all(provers + [foreign], [W] * 4, par)
    for bad in ([], provers[:3], [provers[0], foreign], [provers[0], fresh], [provers[0], provers[0]]):
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):  # LFGPU_ERR_ARG
            batch.prove(bad, [W] * len(bad), tss[:len(bad)])
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):  # the 32-byte hooks are missing in slot 1
        batch.prove(provers[:2], [W] * 2, [tss[0], _UnsizedTranscript(tss[1])])
    L = gpu.L  # NULL arguments with a live batch
    ok = (C.c_int * 2)()
    assert L.lfgpu_zk_prove_batch256(batch.h, None, 2, None, None, ok) == 1
    for nb_max in (0, G.pkg.SC_BATCH_MAX + 1):
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):
            G.pkg.ZkBatch256(gpu, circ, nb_max)

    class Comm:  # a one-rank communicator: its hooks are never reached
        def __init__(self):
            self.fns = (par_mod.AG_FN(lambda *a: 1), par_mod.A2A_FN(lambda *a: 1), par_mod.BC_FN(lambda *a: 1))
            self.ops = par_mod.CommOps(None, 0, 1, *self.fns)

    provers[1].set_comm(Comm())
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 3:"):  # LFGPU_ERR_UNSUPPORTED
        batch.prove(provers[:2], [W] * 2, tss[:2])
    provers[1].set_comm(None)
    # the context and the batch are usable afterwards, and no refused call has touched a transcript or drawn from it: the proofs
    # and the transcripts' end states are the single path's
    assert batch.prove(provers[:2], [W] * 2, tss[:2]) == [True, True]
    for b in range(2):
        _, wire, after = want_single(case, b, circ, W, par)
        assert provers[b].wire() == wire and tss[b].bytes(32) == after, b
    # a circuit over a 16-byte field belongs to ZkBatch
    from test_zk_fp128_synth import load_case as load_fp
    _, raw16, _ = load_fp("funnel")
    c16 = G.pkg.Circuit(gpu, raw16)
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:.*lfgpu_zk_batch_new"):
        G.pkg.ZkBatch256(gpu, c16, 2)
    c16.close()
    for ts in tss:
        ts.close()
    batch.close()
    for zk in provers + [foreign, fresh]:
        zk.close()
    circ.close()
    circ2.close()


@pytest.mark.gpu
def test_per_statement_tail_switch_gives_the_same_bytes():
    """LFGPU_LIGERO_PROVE_BATCH256 is read once per process: one child per setting proves `odd` at B = 3 and prints the SHA-256s"""
    raw, W, par = load("odd")
    exe = os.path.join(ROOT, "tests", "zk_prove_batch256_child.py")
    got = {}
    for setting in ("0", "1"):
        env = dict(os.environ)
        env[SWITCH] = setting
        out = subprocess.run([sys.executable, exe, "odd", "3"], capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
        got[setting] = json.loads(out.stdout.strip().splitlines()[-1])
        assert got[setting]["switch"] == setting
    assert got["0"]["sha256"] == got["1"]["sha256"] and len(set(got["1"]["sha256"])) == 3
    assert got["1"]["sha256"][0] == par["sha"], "statement 0 vs the reference's proof"
    # the batched tail reports the batch's phase times for every member; per statement they are each statement's own
    assert len(set(got["1"]["ligero_prove"])) == 1 and len(set(got["0"]["ligero_prove"])) > 1


@pytest.mark.gpu
def test_cxx_example_check_mode():
    from test_zk_batch256_abi import build_example
    exe = build_example()
    raw, W, _ = load("funnel")
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "c.lfc1"), "wb").write(raw)
        open(os.path.join(tmp, "w.bin"), "wb").write(W.tobytes())
        out = subprocess.run([exe, os.path.join(tmp, "c.lfc1"), os.path.join(tmp, "w.bin"), "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["B"] == 3 and res["field"] == 1 and res["batch_equals_sequential"] is True and res["bench_passes"] == 0

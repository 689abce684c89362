"""lfgpu_zk_commit_batch256: the commits of B provers of one Fp256Base circuit through one chain of dispatches (the pads per
statement, ONE lfgpu_ligero_commit_batch256, the roots into the transcripts), then lfgpu_zk_prove_batch256 or lfgpu_zk_prove.

No tolerances: everything is compared byte for byte.  The reference for every statement is the unchanged single path in the
same process (want_single of test_zk_prove_batch256.py: a ZkProver of its own, the same seeds, lfgpu_zk_commit +
lfgpu_zk_prove).  Statement 0 runs with the fixture's seeds, so its root is also zk_root and its proof zk_wire_sha256 of
tests/golden/synth_p256.json -- the REAL reference's values.  The shapes are the fixtures' ligero_param, the smallest at which
the chain can go wrong:
  funnel B=3   21 rows, block 42 / dblock 83, block_enc 256: below the 512-point LDS tile, no stage launches
  funnel B=64  LFGPU_SC_BATCH_MAX: the full pointer tables
  wide   B=3   18 rows, block_enc 1024: 16 `block` rows a statement, an odd number of low-degree rows in all -- an imaginary
               half stays empty under either pairing
  odd    B=3   20 rows, block_enc 4096, block_ext 3187: 3 stage launches per direction, Merkle levels above 10
  tall   B=2   21 rows, block 2730 / dblock 5459, block_enc 16384: 5 stage launches per direction, the largest image
  funnel B=1   in a batch object of nb_max = 4"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_zk_p256_synth import records
from test_zk_prove_batch256 import _UnsizedTranscript, load, seeds, want_single

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def engines(par, B, first=0):
    import ligero_fixture as lf
    return [lf.LcgRng(seeds(par, first + b)[0]).bytes for b in range(B)]


def transcripts(par, B, first=0):
    import gpu_util as G
    return [G.pkg.FsTranscript(seeds(par, first + b)[1]) for b in range(B)]


def setup(case, B, nb_max=None):
    import gpu_util as G
    raw, W, par = load(case)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    assert circ.info.field == G.pkg.FIELD_P256
    provers = [G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(B)]
    return gpu, circ, W, par, provers, G.pkg.ZkBatch256(gpu, circ, nb_max or B)


def teardown(circ, provers, batch, tss=()):
    for ts in tss:
        ts.close()
    batch.close()
    for zk in provers:
        zk.close()
    circ.close()


# ---------------------------------------------------------------- commit by batch, prove by batch
def check_commit_batch(case, B, nb_max=None):
    import gpu_util as G
    gpu, circ, W, par, provers, batch = setup(case, B, nb_max)
    rec = records()[case]
    lp = rec["ligero_param"]
    p = provers[0].param
    assert (p.nrow, p.block, p.dblock, p.block_enc, p.block_ext) == (lp["nrow"], lp["block"], lp["dblock"], lp["block_enc"], lp["block_ext"])
    tss = transcripts(par, B)
    roots = batch.commit(provers, [W] * B, engines(par, B), tss)
    assert roots[0].hex() == rec["zk_root"], "statement 0 vs the reference's root"
    assert batch.prove(provers, [W] * B, tss) == [True] * B
    wires = [zk.wire() for zk in provers]
    assert hashlib.sha256(wires[0]).hexdigest() == par["sha"], "statement 0 vs the reference's proof"
    for b in range(B):
        root, wire, after = want_single(case, b, circ, W, par)
        assert roots[b] == root, "root %d vs lfgpu_zk_commit" % b
        assert wires[b] == wire, "statement %d vs lfgpu_zk_prove" % b
        assert tss[b].bytes(32) == after, "statement %d: the transcript is not where the single path leaves it" % b
        tv = G.pkg.FsTranscript(seeds(par, b)[1])
        assert G.pkg.zk_verify(gpu, circ, wires[b], W[:circ.info.npub_in], tv, par["rate"], par["nreq"], par["block_enc"]) == (True, "ok"), b
        tv.close()
    assert len(set(roots)) == B
    commit_ms = [zk.timings()["commit"] for zk in provers]
    assert len(set(commit_ms)) == 1 and commit_ms[0] > 0
    teardown(circ, provers, batch, tss)


CASES = [("funnel", 3), ("funnel", 64), ("wide", 3), ("odd", 3), ("tall", 2)]


@pytest.mark.parametrize("case,B", CASES, ids=["%s-B%d" % c for c in CASES])
def test_batched_commit_equals_single_path_and_reference(case, B):
    check_commit_batch(case, B)


def test_batch_of_one_in_a_larger_batch_object():
    check_commit_batch("funnel", 1, nb_max=4)


# ---------------------------------------------------------------- mixed use
def test_commit_by_batch_then_prove_singly():
    case, B = "odd", 3
    gpu, circ, W, par, provers, batch = setup(case, B)
    tss = transcripts(par, B)
    roots = batch.commit(provers, [W] * B, engines(par, B), tss)
    for b in range(B):
        root, wire, after = want_single(case, b, circ, W, par)
        assert provers[b].prove(W, tss[b]) is True
        assert (roots[b], provers[b].wire(), tss[b].bytes(32)) == (root, wire, after), b
    teardown(circ, provers, batch, tss)


# ---------------------------------------------------------------- re-commit
def test_recommit_replaces_the_commitments_and_a_bad_witness_fails_only_its_slot():
    """slot 1 of the second commit holds the broken witness of test_bad_witness_in_one_slot_leaves_the_others_alone"""
    import gpu_util as G
    import ligero_fixture as lf
    case, B = "funnel", 3
    gpu, circ, W, par, provers, batch = setup(case, B)
    tss = transcripts(par, B)
    first = batch.commit(provers, [W] * B, engines(par, B), tss)
    assert first == [want_single(case, b, circ, W, par)[0] for b in range(B)]
    for ts in tss:
        ts.close()
    W2 = W.copy()
    W2[circ.info.npub_in + 7, 0] ^= np.uint64(1)
    Ws = [W, W2, W]
    tss = transcripts(par, B, first=3)  # other seeds: statements 3, 4, 5
    roots = batch.commit(provers, Ws, engines(par, B, first=3), tss)
    assert not set(roots) & set(first)
    # the broken witness commits fine: its root is what lfgpu_zk_commit gives for it
    zk1 = G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"])
    t1 = G.pkg.FsTranscript(seeds(par, 4)[1])
    assert roots[1] == zk1.commit(W2, lf.LcgRng(seeds(par, 4)[0]).bytes, t1)
    t1.close()
    zk1.close()
    assert batch.prove(provers, Ws, tss) == [True, False, True]
    for b in (0, 2):
        root, wire, after = want_single(case, 3 + b, circ, W, par)
        assert (roots[b], provers[b].wire(), tss[b].bytes(32)) == (root, wire, after), b
    with pytest.raises(G.pkg.LfGpuError):
        provers[1].wire()
    teardown(circ, provers, batch, tss)


# ---------------------------------------------------------------- argument errors
def test_argument_errors():
    import importlib

    import gpu_util as G
    from test_zk_fp128_synth import load_case as load_fp
    par_mod = importlib.import_module("longfellow_zk_amd.parallel")
    case = "funnel"
    raw, W, par = load(case)
    gpu = G.gpu()
    circ, circ2 = G.pkg.Circuit(gpu, raw), G.pkg.Circuit(gpu, raw)
    mk = lambda c, nreq=par["nreq"]: G.pkg.ZkProver(gpu, c, par["rate"], nreq, par["block_enc"])  # noqa: E731
    provers = [mk(circ) for _ in range(3)]
    foreign, other_nreq = mk(circ2), mk(circ, par["nreq"] + 3)
    rec16, raw16, W16 = load_fp("funnel")
    circ16 = G.pkg.Circuit(gpu, raw16)
    prover16 = G.pkg.ZkProver(gpu, circ16, rec16["rate"], rec16["nreq"], rec16["block_enc_arg"])
    batch = G.pkg.ZkBatch256(gpu, circ, 2)
    tss = transcripts(par, 3)
    fresh = transcripts(par, 3)
    before = [ts.bytes(32) for ts in fresh]  # what an untouched transcript with these seeds yields
    for ts in fresh:
        ts.close()
    eng = engines(par, 3)
    drawn = [0]

    def counting(n):
        drawn[0] += 1
        return bytes(n)

    for bad in ([], provers[:3], [provers[0], foreign], [provers[0], provers[0]], [provers[0], other_nreq], [provers[0], prover16]):
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):  # LFGPU_ERR_ARG
            batch.commit(bad, [W] * len(bad), [counting] * len(bad), tss[:len(bad)])
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):  # the 32-byte hooks are missing in slot 1
        batch.commit(provers[:2], [W] * 2, [counting] * 2, [tss[0], _UnsizedTranscript(tss[1])])
    L = gpu.L  # NULL arguments with a live batch
    assert L.lfgpu_zk_commit_batch256(batch.h, None, 2, None, None, None, None, None) == 1

    class Comm:  # a one-rank communicator: its hooks are never reached
        def __init__(self):
            self.fns = (par_mod.AG_FN(lambda *a: 1), par_mod.A2A_FN(lambda *a: 1), par_mod.BC_FN(lambda *a: 1))
            self.ops = par_mod.CommOps(None, 0, 1, *self.fns)

    provers[1].set_comm(Comm())
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 3:"):  # LFGPU_ERR_UNSUPPORTED
        batch.commit(provers[:2], [W] * 2, [counting] * 2, tss[:2])
    provers[1].set_comm(None)
    assert drawn[0] == 0, "a refused call drew from a RandomEngine"
    # the batch is usable afterwards, and the refused calls left the transcripts alone: roots, proofs and the transcripts' end
    # states are the single path's
    roots = batch.commit(provers[:2], [W] * 2, eng[:2], tss[:2])
    assert batch.prove(provers[:2], [W] * 2, tss[:2]) == [True, True]
    for b in range(2):
        root, wire, after = want_single(case, b, circ, W, par)
        assert (roots[b], provers[b].wire(), tss[b].bytes(32)) == (root, wire, after), b
    assert tss[2].bytes(32) == before[2], "a refused call moved a transcript"
    teardown(circ, provers + [foreign, other_nreq], batch, tss)
    prover16.close()
    circ16.close()
    circ2.close()


# ---------------------------------------------------------------- the A/B switch and the chunk boundary, one process each
@pytest.mark.parametrize("case", ["funnel", "odd"])
@pytest.mark.parametrize("setting", ["LFGPU_COMMIT_BATCH256=0", "LFGPU_CB_CHUNK=2"])
def test_switches_reproduce_the_default_bytes(setting, case):
    """B = 5 with chunks of 2: the last chunk is short.  The default's bytes are the single path's (the tests above)."""
    import gpu_util as G
    B = 5
    env = {k: v for k, v in os.environ.items() if k not in ("LFGPU_COMMIT_BATCH256", "LFGPU_CB_CHUNK")}
    k, v = setting.split("=")
    env[k] = v
    child = os.path.join(ROOT, "tests", "zk_commit_batch256_child.py")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, child, case, str(B)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    raw, W, par = load(case)
    circ = G.pkg.Circuit(G.gpu(), raw)
    for b in range(B):
        root, wire, after = want_single(case, b, circ, W, par)
        assert (got["roots"][b], got["wires"][b], got["after"][b]) == (root.hex(), hashlib.sha256(wire).hexdigest(), after.hex()), b
    circ.close()


# ---------------------------------------------------------------- the C++ example
def test_cxx_example_check_mode():
    from test_zk_commit_batch256_abi import build_example
    exe = build_example()
    raw, W, _ = load("funnel")
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "c.lfc1"), "wb").write(raw)
        open(os.path.join(tmp, "w.bin"), "wb").write(W.tobytes())
        out = subprocess.run([exe, os.path.join(tmp, "c.lfc1"), os.path.join(tmp, "w.bin"), "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["B"] == 3 and res["field"] == 1 and res["roots_equal"] is True and res["proofs_equal"] is True and res["bench_passes"] == 0

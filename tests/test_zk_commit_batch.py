"""lfgpu_zk_commit_batch: the commits of B provers of one circuit through one chain of dispatches (fill_pad per statement, ONE
batched Ligero commit, the roots into the transcripts), then lfgpu_zk_prove_batch or lfgpu_zk_prove.

The reference for every statement is the unchanged single path in the same process (want_single of test_zk_prove_batch.py: a
ZkProver of its own, the same seeds, lfgpu_zk_commit + lfgpu_zk_prove).  Statement 0 runs with the fixture's seeds, so its
proof is also pinned by the fixture's zk_wire_sha256 -- the REAL reference's proof."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from test_zk_prove_batch import commit_all, load, seeds, want_single

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
    provers = [G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(B)]
    return gpu, circ, W, par, provers, G.pkg.ZkBatch(gpu, circ, nb_max or B)


def teardown(circ, provers, batch, tss=()):
    for ts in tss:
        ts.close()
    batch.close()
    for zk in provers:
        zk.close()
    circ.close()


# ---------------------------------------------------------------- commit by batch, prove by batch
CASES = [("flatsha_nb1", 3), ("flatsha_nb1_pub9_sfb777", 2), ("funnel", 64), ("odd", 3), ("tall", 2), ("long", 2), ("gf long", 2)]


@pytest.mark.parametrize("case,B", CASES, ids=["%s-B%d" % c for c in CASES])
def test_batched_commit_equals_single_path_and_reference(case, B):
    import gpu_util as G
    gpu, circ, W, par, provers, batch = setup(case, B)
    tss = transcripts(par, B)
    roots = batch.commit(provers, [W] * B, engines(par, B), tss)
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


# ---------------------------------------------------------------- mixed use
def test_commit_by_batch_then_prove_singly():
    case, B = "flatsha_nb1", 3
    gpu, circ, W, par, provers, batch = setup(case, B)
    tss = transcripts(par, B)
    roots = batch.commit(provers, [W] * B, engines(par, B), tss)
    for b in range(B):
        root, wire, after = want_single(case, b, circ, W, par)
        assert provers[b].prove(W, tss[b]) is True
        assert (roots[b], provers[b].wire(), tss[b].bytes(32)) == (root, wire, after), b
    teardown(circ, provers, batch, tss)


def test_commit_singly_then_prove_by_batch_control():
    case, B = "odd", 3
    gpu, circ, W, par, provers, batch = setup(case, B)
    tss, roots = commit_all(provers, [W] * B, par)
    assert batch.prove(provers, [W] * B, tss) == [True] * B
    for b in range(B):
        root, wire, after = want_single(case, b, circ, W, par)
        assert (roots[b], provers[b].wire(), tss[b].bytes(32)) == (root, wire, after), b
    teardown(circ, provers, batch, tss)


# ---------------------------------------------------------------- re-commit
def test_recommit_replaces_the_commitments_and_a_bad_witness_fails_only_its_slot():
    """slot 1 of the second commit holds the broken witness of test_bad_witness_in_one_slot_leaves_the_others_alone"""
    import gpu_util as G
    import ligero_fixture as lf
    case, B = "flatsha_nb1", 3
    gpu, circ, W, par, provers, batch = setup(case, B)
    tss = transcripts(par, B)
    first = batch.commit(provers, [W] * B, engines(par, B), tss)
    assert first == [want_single(case, b, circ, W, par)[0] for b in range(B)]
    for ts in tss:
        ts.close()
    W2 = W.copy()
    W2[1:, 0] ^= np.uint64(1)
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
    par_mod = importlib.import_module("longfellow_zk_amd.parallel")
    case = "funnel"
    raw, W, par = load(case)
    gpu = G.gpu()
    circ, circ2 = G.pkg.Circuit(gpu, raw), G.pkg.Circuit(gpu, raw)
    mk = lambda c, nreq=par["nreq"]: G.pkg.ZkProver(gpu, c, par["rate"], nreq, par["block_enc"])  # noqa: E731
    provers = [mk(circ) for _ in range(3)]
    foreign, other_nreq = mk(circ2), mk(circ, par["nreq"] - 1)
    batch = G.pkg.ZkBatch(gpu, circ, 2)
    tss = transcripts(par, 3)
    eng = engines(par, 3)
    drawn = [0]

    def counting(n):
        drawn[0] += 1
        return bytes(n)

    for bad in ([], provers[:3], [provers[0], foreign], [provers[0], provers[0]], [provers[0], other_nreq]):
        with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 1:"):  # LFGPU_ERR_ARG
            batch.commit(bad, [W] * len(bad), [counting] * len(bad), tss[:len(bad)])

    class Comm:  # a one-rank communicator: its hooks are never reached
        def __init__(self):
            self.fns = (par_mod.AG_FN(lambda *a: 1), par_mod.A2A_FN(lambda *a: 1), par_mod.BC_FN(lambda *a: 1))
            self.ops = par_mod.CommOps(None, 0, 1, *self.fns)

    provers[1].set_comm(Comm())
    with pytest.raises(G.pkg.LfGpuError, match="lfgpu error 3:"):  # LFGPU_ERR_UNSUPPORTED
        batch.commit(provers[:2], [W] * 2, [counting] * 2, tss[:2])
    provers[1].set_comm(None)
    assert drawn[0] == 0, "a refused call drew from a RandomEngine"
    # the batch is usable afterwards, and the refused calls left the transcripts alone
    roots = batch.commit(provers[:2], [W] * 2, eng[:2], tss[:2])
    assert batch.prove(provers[:2], [W] * 2, tss[:2]) == [True, True]
    for b in range(2):
        root, wire, after = want_single(case, b, circ, W, par)
        assert (roots[b], provers[b].wire(), tss[b].bytes(32)) == (root, wire, after), b
    teardown(circ, provers + [foreign, other_nreq], batch, tss)
    circ2.close()


# ---------------------------------------------------------------- the A/B switch and the chunk boundary, one process each
@pytest.mark.parametrize("case", ["funnel", "flatsha_nb1"])
@pytest.mark.parametrize("setting", ["LFGPU_COMMIT_BATCH=0", "LFGPU_CB_CHUNK=2"])
def test_switches_reproduce_the_default_bytes(setting, case):
    """B = 5 with chunks of 2: the last chunk is short.  The default's bytes are the single path's (the tests above)."""
    import gpu_util as G
    B = 5
    env = {k: v for k, v in os.environ.items() if k not in ("LFGPU_COMMIT_BATCH", "LFGPU_CB_CHUNK")}
    k, v = setting.split("=")
    env[k] = v
    child = os.path.join(ROOT, "tests", "zk_commit_batch_child.py")
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
    from test_zk_commit_batch_abi import build_example
    exe = build_example()
    raw, W, _ = load("flatsha_nb1")
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "c.lfc1"), "wb").write(raw)
        open(os.path.join(tmp, "w.bin"), "wb").write(W.tobytes())
        out = subprocess.run([exe, os.path.join(tmp, "c.lfc1"), os.path.join(tmp, "w.bin"), "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["B"] == 3 and res["roots_equal"] is True and res["proofs_equal"] is True and res["bench_passes"] == 0

"""lfgpu_zk_prove_batch with the batched Ligero prove: after the lock-step sumcheck the constraints' EQ tables, the row
combinations and the openings of all statements run in three chains (one lf_raw_eq2_batch launch, one
lfgpu_ligero_prove_batch, one lfgpu_ligero_open_batch) instead of once per statement.

Every check is test_zk_prove_batch.py's check_batch: each statement against lfgpu_zk_prove on a prover of its own (wire
bytes, transcript end state), statement 0 against the fixture's wire SHA-256 (the real reference's proof), zk_verify on every
proof.  LFGPU_LIGERO_PROVE_BATCH and LFGPU_LP_CHUNK are read once per process, so every setting runs in a child."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_zk_prove_batch import check_batch, commit_all, load, want_single

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("LFGPU_LIGERO_PROVE_BATCH", "LFGPU_LP_CHUNK")
# pub9: npub = 9, the read-back of the public part of every statement's EQ table
CASES = [("flatsha_nb1", 3), ("flatsha_nb1_pub9_sfb777", 2), ("funnel", 64), ("gf odd", 3)]
SETTINGS = [{"LFGPU_LIGERO_PROVE_BATCH": "1"}, {"LFGPU_LIGERO_PROVE_BATCH": "0"}, {"LFGPU_LIGERO_PROVE_BATCH": "1", "LFGPU_LP_CHUNK": "2"}]


def child(case, B, setting):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(setting)
    exe = os.path.join(ROOT, "tests", "zk_prove_batch_ligero_child.py")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, exe, case, str(B)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("setting", SETTINGS, ids=["batch", "per-statement", "batch-chunk2"])
@pytest.mark.parametrize("case,B", CASES, ids=["%s-B%d" % c for c in CASES])
def test_same_bytes_under_every_setting(case, B, setting):
    t = child(case, B, setting)
    assert len(t["constraints"]) == B and min(t["constraints"]) > 0 and min(t["ligero_prove"]) > 0
    if setting["LFGPU_LIGERO_PROVE_BATCH"] == "0":
        # the statements' own times: intervals of one call that do not overlap, so together they fit into the call (B times a
        # phase of the whole batch would be counted B times over)
        assert sum(t["constraints"]) + sum(t["ligero_prove"]) <= t["prove"][0], t
    else:  # the batch's phase times, the same for every member
        assert len(set(t["constraints"])) == 1 and len(set(t["ligero_prove"])) == 1, t


def test_timings_are_the_batch_phase_times_on_the_default_path():
    """constraints and Ligero prove of a batch are one phase each: the same value for every member (per statement before the
    batched Ligero prove existed, and with the switch off).  In a child without either switch in its environment."""
    t = child("flatsha_nb1", 3, {})
    for key in ("constraints", "ligero_prove"):
        assert len(t[key]) == 3 and len(set(t[key])) == 1 and t[key][0] > 0, (key, t)


def test_bad_witness_in_one_slot_on_the_batched_path():
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
    with pytest.raises(G.pkg.LfGpuError):  # slot 1 holds no proof ...
        provers[1].wire()
    # ... and its transcript is where lfgpu_zk_prove leaves it after the same witness
    import ligero_fixture as lf
    from test_zk_prove_batch import seeds
    rs, seed = seeds(par, 1)
    zk = G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"])
    ts = G.pkg.FsTranscript(seed)
    zk.commit(W2, lf.LcgRng(rs).bytes, ts)
    assert zk.prove(W2, ts) is False
    assert tss[1].bytes(32) == ts.bytes(32)
    for x in tss + [ts, zk, batch] + provers + [circ]:
        x.close()


def test_one_batch_object_twice_on_recommitted_provers():
    """the EQ slabs of the batch and the context's pooled scratch are reused: the same bytes"""
    import gpu_util as G
    case = "flatsha_nb1_pub9_sfb777"
    raw, W, par = load(case)
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    provers = [G.pkg.ZkProver(gpu, circ, par["rate"], par["nreq"], par["block_enc"]) for _ in range(3)]
    batch = G.pkg.ZkBatch(gpu, circ, 3)
    for rep in range(2):
        tss, _ = commit_all(provers, [W] * 3, par)
        assert batch.prove(provers, [W] * 3, tss) == [True] * 3
        for b in range(3):
            _, wire, after = want_single(case, b, circ, W, par)
            assert provers[b].wire() == wire and tss[b].bytes(32) == after, (rep, b)
        for ts in tss:
            ts.close()
    for x in [batch] + provers + [circ]:
        x.close()


def test_provers_with_different_ligero_parameters_keep_the_per_statement_tail():
    """two provers of one circuit made with nreq 132 and 131: a valid batch (the sumcheck does not look at the Ligero parameters)
    whose tableaux differ in shape; every proof is lfgpu_zk_prove's and the transcripts end where it leaves them"""
    import gpu_util as G
    import ligero_fixture as lf
    from test_zk_prove_batch import seeds
    raw, W, par = load("flatsha_nb1")
    gpu = G.gpu()
    circ = G.pkg.Circuit(gpu, raw)
    nreqs = [par["nreq"], par["nreq"] - 1]
    want = []
    for b, nreq in enumerate(nreqs):
        rs, seed = seeds(par, b)
        zk = G.pkg.ZkProver(gpu, circ, par["rate"], nreq, par["block_enc"])
        ts = G.pkg.FsTranscript(seed)
        zk.commit(W, lf.LcgRng(rs).bytes, ts)
        assert zk.prove(W, ts) is True
        want.append((zk.wire(), ts.bytes(32)))
        ts.close()
        zk.close()
    provers = [G.pkg.ZkProver(gpu, circ, par["rate"], nreq, par["block_enc"]) for nreq in nreqs]
    batch = G.pkg.ZkBatch(gpu, circ, 2)
    tss, _ = commit_all(provers, [W] * 2, par)
    assert batch.prove(provers, [W] * 2, tss) == [True, True]
    for b in range(2):
        wire = provers[b].wire()
        assert wire == want[b][0], "statement %d vs lfgpu_zk_prove" % b
        assert tss[b].bytes(32) == want[b][1], b
        tv = G.pkg.FsTranscript(seeds(par, b)[1])
        assert G.pkg.zk_verify(gpu, circ, wire, W[:circ.info.npub_in], tv, par["rate"], nreqs[b], par["block_enc"]) == (True, "ok"), b
        tv.close()
    assert len(want[0][0]) != len(want[1][0])  # the parameters do differ
    for x in tss + [batch] + provers + [circ]:
        x.close()


def test_batch_of_one_in_a_larger_batch_object():
    check_batch("flatsha_nb1", 1, nb_max=4)

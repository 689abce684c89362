"""tests/concurrent_parity.py can fail: run_lockstep driven by fake workers (no GPU), and the section locator on the reference's
own flatsha_nb1 proof.  The GPU cases of tests/test_zk_concurrent_parity.py never mutate the library on purpose; that a wrong
byte in one result of one worker would be reported, and as exactly that, is shown here."""
import hashlib
import json
import lzma
import os
import threading
import time
from types import SimpleNamespace

import concurrent_parity as cp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K, NJOBS = 6, 12


def canned(i, j):
    return b"worker %d job %d " % (i, j) * 5


class Fake:
    """sleeps briefly and returns canned bytes; counts its calls and sees how many workers are inside job() at once"""
    inside, peak, lock = 0, 0, threading.Lock()

    def __init__(self, i, wrong=None, raises=None):
        self.i, self.wrong, self.raises, self.calls = i, wrong, raises, []

    def job(self, j):
        self.calls.append(j)
        with Fake.lock:
            Fake.inside += 1
            Fake.peak = max(Fake.peak, Fake.inside)
        try:
            time.sleep(0.005)
            if self.raises == j:
                raise RuntimeError("lfgpu error 3: an illegal memory access was encountered (worker %d)" % self.i)
            out = bytearray(canned(self.i, j))
            if self.wrong == j:
                out[7] ^= 0x01
            return bytes(out)
        finally:
            with Fake.lock:
                Fake.inside -= 1

    def describe_mismatch(self, j, got):
        return "first byte that differs: %d" % cp.first_difference(got, canned(self.i, j))


EXPECTED = [[hashlib.sha256(canned(i, j)).hexdigest() for j in range(NJOBS)] for i in range(K)]


def test_all_results_match():
    Fake.peak = 0
    ws = [Fake(i) for i in range(K)]
    rep = cp.run_lockstep(ws, NJOBS, EXPECTED)
    assert rep == {"done": [NJOBS] * K, "started": [NJOBS] * K, "failure": None}
    assert all(w.calls == list(range(NJOBS)) for w in ws)  # every job once, in order
    assert Fake.peak > 1  # the workers did run at the same time


def test_one_wrong_byte_is_reported_as_exactly_that():
    ws = [Fake(i, wrong=4 if i == 3 else None) for i in range(K)]
    rep = cp.run_lockstep(ws, NJOBS, EXPECTED)
    f = rep["failure"]
    assert (f["worker"], f["job"], f["kind"]) == (3, 4, "mismatch")
    assert EXPECTED[3][4] in f["detail"] and "first byte that differs: 7" in f["detail"]
    assert rep["done"][3] == 4 and ws[3].calls == [0, 1, 2, 3, 4]  # the job is not run again, nothing after it
    for i in (0, 1, 2, 4, 5):  # the others finish the call they are in and stop: well short of their 12 jobs of ~5 ms each
        assert ws[i].calls == list(range(len(ws[i].calls))) and 1 <= len(ws[i].calls) < NJOBS, (i, ws[i].calls)
        assert rep["started"][i] == len(ws[i].calls) and rep["done"][i] == len(ws[i].calls)


def test_a_raising_worker_is_reported_with_its_text():
    ws = [Fake(i, raises=2 if i == 1 else None) for i in range(K)]
    rep = cp.run_lockstep(ws, NJOBS, EXPECTED)
    f = rep["failure"]
    assert (f["worker"], f["job"], f["kind"]) == (1, 2, "exception")
    assert "RuntimeError" in f["detail"] and "an illegal memory access was encountered (worker 1)" in f["detail"]
    assert ws[1].calls == [0, 1, 2] and rep["done"][1] == 2
    assert all(len(w.calls) < NJOBS for w in ws)  # nobody starts further work after the error


def test_only_the_first_failure_is_kept():
    ws = [Fake(i, wrong=0) for i in range(K)]  # everybody is wrong at once
    rep = cp.run_lockstep(ws, NJOBS, EXPECTED)
    assert rep["failure"]["job"] == 0 and rep["done"] == [0] * K and rep["started"] == [1] * K


def test_first_difference():
    a = bytes(range(200))
    assert cp.first_difference(a, a) is None
    assert cp.first_difference(a, a[:150]) == 150 and cp.first_difference(a[:10], a) == 10
    for off in (0, 1, 99, 199):
        b = bytearray(a)
        b[off] ^= 0x80
        b[199] ^= 1
        assert cp.first_difference(a, bytes(b)) == off


def test_section_locator_on_the_reference_proof_of_flatsha_nb1():
    """the recorded layout: the reference's component dump of its flatsha_nb1 proof, re-serialised to the wire (pinned by the
    recorded SHA-256 of the reference's own ZkProof::write) with the layers' logw read from the circuit file"""
    from synth_fixture import read_lfc1_16
    from test_zk_cxx import wire_from_components
    info = json.load(open(os.path.join(GOLD, "flatsha_nb1.json")))
    circ = read_lfc1_16(lzma.decompress(open(os.path.join(GOLD, "flatsha_nb1.lfc1.xz"), "rb").read()))
    logws = [ly["logw"] for ly in circ["layers"]]
    p = SimpleNamespace(block=info["zk_block"], dblock=info["zk_dblock"], r=cp.NREQ, nreq=cp.NREQ, nrow=info["zk_nrow"])
    wire = wire_from_components(lzma.decompress(open(os.path.join(GOLD, "flatsha_nb1.zkproof.xz"), "rb").read()), logws, p)
    assert len(wire) == info["zk_wire_bytes"] and hashlib.sha256(wire).hexdigest() == info["zk_wire_sha256"]
    secs = cp.wire_sections(wire, 16, logws, p, 2)
    names = [s[0] for s in secs]
    assert names == ["commitment"] + ["sumcheck layer %d" % i for i in range(info["nl"])] + \
        ["Ligero y_ldt", "Ligero y_dot", "Ligero y_quad", "nonces", "opened columns", "Merkle path"]
    assert secs[0][1] == 0 and secs[-1][2] == len(wire) and all(a[2] == b[1] and a[1] < a[2] for a, b in zip(secs, secs[1:]))
    by = {s[0]: s for s in secs}
    assert sum(b - a for n, a, b in secs if n.startswith("sumcheck")) == 16 * sum(4 * l + 2 for l in logws) == 16 * (2 * info["round_hands"] + 2 * info["nl"])
    assert by["Ligero y_ldt"][2] - by["Ligero y_ldt"][1] == 16 * p.block and by["Ligero y_dot"][2] - by["Ligero y_dot"][1] == 16 * p.dblock
    assert by["Ligero y_quad"][2] - by["Ligero y_quad"][1] == 16 * (p.r + p.dblock - p.block)
    assert by["nonces"][2] - by["nonces"][1] == 32 * p.nreq
    assert by["opened columns"][2] - by["opened columns"][1] >= 4 + 2 * p.nrow * p.nreq
    for name, a, b in secs:  # a differing byte at the first, a middle and the last offset of every section
        for off in (a, (a + b) // 2, b - 1):
            assert cp.locate(secs, off) == name
            bad = bytearray(wire)
            bad[off] ^= 0x20
            bad[-1] ^= 1  # a later difference does not move the answer
            d = cp.describe_wire_difference(bytes(bad), wire, secs)
            assert "offset %d, in %s (+%d)" % (off, name, off - a) in d, d
    assert cp.locate(secs, len(wire)) == "past the end"
    assert "offset %d, in past the end" % len(wire) in cp.describe_wire_difference(wire + b"\0", wire, secs)
    coarse = cp.coarse_sections(secs)
    assert [s[0] for s in coarse] == ["commitment", "sumcheck", "Ligero y_ldt", "Ligero y_dot", "Ligero y_quad", "nonces", "opened columns", "Merkle path"]
    assert coarse[1][1] == 32 and coarse[1][2] == by["Ligero y_ldt"][1]

"""Throughput mode ("independent proofs are trivially parallel"): K provers in K host threads on ONE
device -- one lfgpu context with its own stream each (lfgpu_own_stream), one copy of the circuit in HBM (lfgpu_circuit_share)
-- must every one produce the reference's wire bytes, and the resident sumcheck kernels must stay co-resident under it: the
per-device CU budget (csrc/ctx.h, lf_cu_acquire) is what guarantees that, exercised here with 8 provers of the 32-block
circuit (up to 64 workgroups per grid each) and with a budget far below what they ask for.

What is compared, and when (tools/zk_throughput.py): every worker proves once with the fixtures' RandomEngine and transcript seed
while it is being built -- the other workers idle -- and asserts the reference's wire SHA-256.  With --check-every 2, as in
every run here, each worker's timed jobs 0, 2, 4, ... are that same proof again, made while the other workers are proving, with
the same assertion; the jobs between them draw from a C-speed engine and are only required to prove (ok == 1).  Every proof of
a fixed job list compared byte for byte, other circuits and the verifier under load: tests/test_zk_concurrent_parity.py.

The reference's loop: lib/circuits/sha/flatsha256_circuit_test.cc:510-536 (one proof after the other on one core)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "zk_throughput.py")
CHECK = ["--check-every", "2"]


def _run(args, env_extra, timeout=600):
    e = dict(os.environ)
    for k in list(e):
        if k.startswith("LFGPU_"):
            del e[k]
    e.update(env_extra)
    r = subprocess.run([sys.executable, TOOL] + args, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_eight_concurrent_provers_emit_reference_wire_bytes():
    """8 threads on flatsha-32: every worker asserts the reference's wire SHA-256 once on an idle device and then in every second
    timed proof, while the other seven are proving"""
    res = _run(["--jobs", "flatsha32", "--k", "8", "--seconds", "1.0"] + CHECK, {})
    k8 = res["flatsha32"]["k"]["8"]
    assert k8["proofs"] >= 8, k8
    assert k8["checked_min_per_worker"] >= 1, k8


@pytest.mark.gpu
def test_concurrent_mdoc_pairs_emit_reference_wire_bytes():
    """4 threads, each proving the mdoc pair (GF2_128 hash circuit + Fp256Base signature circuit: both resident-grid kernels live at
    once); the wire SHA-256 of both proofs asserted on an idle device and in every second timed pair, under load"""
    res = _run(["--jobs", "mdoc", "--k", "4", "--seconds", "1.0"] + CHECK, {})
    assert res["mdoc"]["k"]["4"]["proofs"] >= 4
    assert res["mdoc"]["k"]["4"]["checked_min_per_worker"] >= 1, res["mdoc"]["k"]["4"]


@pytest.mark.gpu
@pytest.mark.parametrize("budget", ["0", "3", "70"])
def test_concurrent_provers_with_a_short_cu_budget(budget):
    """budget 0: no resident kernel ever; 3 / 70: the grids wait for room or start late and small -- no timeout, and the
    reference's bytes in every second timed proof of every worker, made under that load"""
    res = _run(["--jobs", "flatsha32", "--k", "4", "--seconds", "0.5"] + CHECK, {"LFGPU_CU_BUDGET": budget})
    assert res["flatsha32"]["k"]["4"]["proofs"] >= 4
    assert res["flatsha32"]["k"]["4"]["checked_min_per_worker"] >= 1, res["flatsha32"]["k"]["4"]

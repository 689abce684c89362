"""Throughput mode, every single result compared byte for byte: tests/concurrent_parity.py run as one child process per case.

K workers in K host threads on one device, each with a context and stream of its own and a shared copy of its circuit.  Every
worker first runs its job list alone on the idle device (the serial path, which the rest of the suite pins to the reference),
then all run at once, and the SHA-256 of every result must be the serial one -- or, for the anchor jobs, which replay the
fixtures' RandomEngine and transcript seed, the reference's recorded zk_wire_sha256.  A mismatch names worker, job, the first
differing offset and the section of the proof it lies in.  The job counts are fixed, so the same results are compared on
every run.  State that exists only in this mode: the per-device CU budget of the resident sumcheck grids (csrc/core.hip), the
LFGPU_EQ_FUSED default from 6 provers on, circuit arrays shared through lfgpu_circuit_share with per-handle caches, function
statics read without a lock, per-context caches that grow on first use, pinned read-back buffers and device mailboxes.

  same_circuit               8 provers of flatsha_nb1 (GF(2^128)): more than 6, the fused EQ path by default; 10 proofs each,
                             jobs 0 and 5 anchored to the reference
  mixed_fields               2 x flatsha_nb1 (GF), 2 x flatsha_fp_nb1 (Fp128), 2 x mdoc_sig (Fp256Base, a resident grid of its
                             own), 2 x flatsha_nb32 (GF, up to 64 workgroups per grid); 6 proofs each, job 0 anchored
  mixed_fields_short_budget  the same with LFGPU_CU_BUDGET=3: the grids wait for room, start late and small, or give up
  batches                    4 workers (2 x GF, 2 x Fp128), 3 x (ZkBatch.commit + ZkBatch.prove) of 4 statements, expected from
                             ZkProver.commit / prove of the same seeds
  verify_under_load          4 provers (GF, Fp128) + 4 verifiers of the reference's own proofs and of copies with one bit
                             flipped in section j; 8 jobs each
  kernel_abi                 6 workers, 3 passes each through 11 kernel-level calls against the CPU oracle, entered at
                             different positions so that different kernels overlap

The mdoc hash circuit (93 MB) is left to tests/test_zk_concurrent.py.

Wall time per case on an MI355X, child process start to end (serial pass / concurrent pass inside it):
  kernel_abi 2.1 s (0.01 / 0.04; 1.9 s are the start of the process, the context and the oracle's results), same_circuit 2.9 s
  (0.73 / 0.28), batches 2.8 s (0.44 / 0.56), verify_under_load 2.5 s (0.36 / 0.16), mixed_fields 3.1 s (0.84 / 0.33),
  mixed_fields_short_budget 3.3 s (0.86 / 0.35)
The children's timeouts are about ten times that: a resident grid that never gets placed ends the case, not the session."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "concurrent_parity.py")
MIXED = [{"kind": "zk", "stem": s, "count": 2} for s in ("flatsha_nb1", "flatsha_fp_nb1", "mdoc_sig", "flatsha_nb32")]
# case -> (spec, jobs per worker, results anchored to the reference's recorded SHA-256, timeout of the child in seconds)
CASES = {
    "same_circuit": ({"workers": [{"kind": "zk", "stem": "flatsha_nb1", "count": 8}], "njobs": 10, "anchor_every": 5}, [10] * 8, 16, 30),
    "mixed_fields": ({"workers": MIXED, "njobs": 6, "anchor_every": 6}, [6] * 8, 8, 30),
    "mixed_fields_short_budget": ({"workers": MIXED, "njobs": 6, "anchor_every": 6, "env": {"LFGPU_CU_BUDGET": "3"}}, [6] * 8, 8, 30),
    "batches": ({"workers": [{"kind": "batch", "stem": s, "count": 2} for s in ("flatsha_nb1", "flatsha_fp_nb1")], "njobs": 3}, [3] * 4, 0, 30),
    "verify_under_load": ({"workers": [{"kind": k, "stem": s, "count": 2} for k in ("zk", "verify") for s in ("flatsha_nb1", "flatsha_fp_nb1")],
                           "njobs": 8}, [8] * 8, 0, 30),
    "kernel_abi": ({"workers": [{"kind": "kernel", "count": 6}], "njobs": 3}, [33] * 6, 0, 30),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_concurrent_results_are_the_serial_ones(case):
    spec, njobs, anchored, timeout = CASES[case]
    r = subprocess.run([sys.executable, CHILD, json.dumps(spec)], capture_output=True, text=True, timeout=timeout)
    lines = r.stdout.strip().splitlines()
    assert lines, r.stderr[-4000:]
    rep = json.loads(lines[-1])
    print(case, json.dumps(rep))
    assert rep["failure"] is None, (rep, r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert rep["done"] == njobs and rep["compared"] == sum(njobs) and rep["anchored"] == anchored, rep

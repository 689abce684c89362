"""Pass A's tile loop (csrc/fft.hip, fp_fft_tile_1024x4_persist): the ISA it compiles to, and its results next to the one-tile-
per-workgroup launches and the oracle.  LFGPU_FP_PERSIST is read once per process, so each setting runs in a child process of
its own (tests/fp_tile_child.py) on the same inputs: 0 = fp_fft_tile_1024x4 in the caller's grid order, unset = one tile per
workgroup in the XCD-aware tile order (default), 2 = the tile loop."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fft_isa
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "fp_tile_child.py")
KERNEL = "_Z26fp_fft_tile_1024x4_persistI8Fp128OpsEv8TilePlanPK5elt_tjS4_jj"

P_HI = 0xFFFFF00000000000
MONT_ONE = [0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFF]
EDGES = [[0, 0], [1, 0], [0, P_HI], MONT_ONE, [0xFFFFFFFFFFFFFFFF, P_HI - 1], [0, 1 << 44]]


def test_pass_a_persistent_isa():
    """No scratch, at most 128 VGPRs (two 512-thread workgroups per CU), and the inter-pass twiddles loaded once per workgroup:
    the kernel holds 17 global loads in all (one stage twiddle, eight inter-pass twiddles, the eight tile loads of the loop),
    and the tile's eight are all issued before the loop's first wait on vector memory."""
    fft_isa.assert_no_scratch_within_128_vgprs(KERNEL)
    fft_isa.assert_global_loads(KERNEL, 17)
    fft_isa.assert_no_vmcnt_wait_among_loads(KERNEL, last=8)


# (logn, rows, ld, direction): the flagship n = 2^20 both ways with 1, 2, 3 and 5 rows (3 and 5 split unevenly between the two
# workgroups of a column block), a strided ld, and n = 2^21 .. 2^23, whose inner 2^20-point transforms run the loop on n / 2^20 rows
CASES = [(20, r, 1 << 20, d) for r in (1, 2, 3, 5) for d in "bf"]
CASES += [(20, 3, (1 << 20) + 64, "f"), (20, 2, (1 << 20) + 4, "b")]
CASES += [(logn, 1, 1 << logn, d) for logn in (21, 22, 23) for d in "bf"]


def _key(case):
    return "c_%d_%d_%d_%s" % case


def _inputs():
    rng = np.random.default_rng(20261017)
    cases = {}
    for logn, rows, ld, d in CASES:
        n = 1 << logn
        a = np.empty((rows, ld, 2), dtype=np.uint64)
        a[..., 0] = rng.integers(0, 2**64, size=(rows, ld), dtype=np.uint64)
        a[..., 1] = rng.integers(0, P_HI, size=(rows, ld), dtype=np.uint64)
        a[:, n:] = [0xDEADBEEFDEADBEEF, 0xFFFFFFFFFFFFFFFF]  # beyond the row: must stay as it is
        for r in range(rows):
            for i, e in enumerate(EDGES):
                a[r, (i * 977 + r * 131) % n] = e
        cases[_key((logn, rows, ld, d))] = a
    return cases


def _child(env_value, cin, cout):
    env = dict(os.environ)
    env.pop("LFGPU_FP_PERSIST", None)
    env.pop("LFGPU_FP_TILE1024", None)
    if env_value is not None:
        env["LFGPU_FP_PERSIST"] = env_value
    r = subprocess.run([sys.executable, CHILD, cin, cout], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(cout)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pass_a_persist")
    cases = _inputs()
    cin = str(d / "cases.npz")
    np.savez(cin, **cases)
    order = _child(None, cin, str(d / "order.npz"))
    loop = _child("2", cin, str(d / "loop.npz"))
    old = _child("0", cin, str(d / "old.npz"))
    return cases, loop, order, old


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_key)
def test_pass_a_persistent_matches_one_tile_launches_and_oracle(runs, case):
    """the default, the tile loop (LFGPU_FP_PERSIST=2) and fp_fft_tile_1024x4 (=0) byte-identical and equal to the oracle's
    fftb / fftf; row padding (ld > n) untouched"""
    cases, loop, order, old = runs
    logn, rows, ld, d = case
    k, n = _key(case), 1 << logn
    assert loop[k].tobytes() == old[k].tobytes()
    assert order[k].tobytes() == old[k].tobytes()
    o = ol.oracle()
    want = cases[k].copy()
    for r in range(rows):
        row = np.ascontiguousarray(want[r, :n])
        (o.lfo_fp_fftf if d == "f" else o.lfo_fp_fftb)(ol.P(row), n, o.lfo_fp_omega32(), 1 << 32)
        want[r, :n] = row
    assert (order[k] == want).all()

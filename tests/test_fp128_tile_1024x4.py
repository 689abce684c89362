"""K1's specialised 1024 x 4 tile kernel (csrc/fft.hip, fp_fft_tile_1024x4): the ISA it compiles to, and its results next to
the generic fp_fft_tile's and the oracle's.  LFGPU_FP_TILE1024 is read once per process, so each path runs in a child process
of its own (tests/fp_tile_child.py) on the same inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fft_isa
import oracle_lib as ol
from oracle_lib import FP, P, arr, elt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "fp_tile_child.py")
KERNELS = ("_Z18fp_fft_tile_1024x4I8Fp128OpsLb0ELb1EEv8TilePlanPK5elt_tjS4_j",  # pass A: columns contiguous, inter-pass twiddles
           "_Z18fp_fft_tile_1024x4I8Fp128OpsLb1ELb0EEv8TilePlanPK5elt_tjS4_j")  # pass B: points contiguous

P_HI = 0xFFFFF00000000000
MONT_ONE = [0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFF]  # 2^128 mod p = 2^108 - 1
EDGES = [[0, 0], [1, 0], [0, P_HI], MONT_ONE, [0xFFFFFFFFFFFFFFFF, P_HI - 1], [0, 1 << 44]]  # p - 1 = {0, P_HI}


def test_tile_1024x4_isa():
    """Both instantiations compile for gfx950 without scratch, within 128 VGPRs (4 waves per SIMD, two 512-thread workgroups
    per CU) and with all eight tile loads (and the stage twiddle's) issued before the first wait on vector memory."""
    for k in KERNELS:
        fft_isa.assert_no_scratch_within_128_vgprs(k)
        assert fft_isa.dwordx4_loads_before_first_vmcnt_wait(k) >= 8, (k, fft_isa.vm_stream(k)[0])


# (logn, rows, ld, direction): n = 2^13 .. 2^23 both ways (pass B's tile from 2^13, pass A's as well at 2^20, both passes of
# the inner 2^20-point transforms beyond it), single rows, row counts that are not multiples of anything, strided rows
CASES = [(logn, 3 if logn <= 16 else (2 if logn <= 20 else 1), 1 << logn, d) for logn in range(13, 24) for d in "bf"]
CASES += [(13, 1, 1 << 13, "b"), (14, 3, (1 << 14) + 5, "b"), (17, 5, (1 << 17) + 1, "f"), (20, 3, (1 << 20) + 64, "b"),
          (20, 1, 1 << 20, "f")]


def _key(case):
    return "c_%d_%d_%d_%s" % case


def _inputs():
    rng = np.random.default_rng(20261016)
    cases = {}
    for logn, rows, ld, d in CASES:
        n = 1 << logn
        a = np.empty((rows, ld, 2), dtype=np.uint64)
        a[..., 0] = rng.integers(0, 2**64, size=(rows, ld), dtype=np.uint64)
        a[..., 1] = rng.integers(0, P_HI, size=(rows, ld), dtype=np.uint64)
        a[:, n:] = [0xDEADBEEFDEADBEEF, 0xFFFFFFFFFFFFFFFF]  # beyond the row: not an element, must stay as it is
        for r in range(rows):  # edge values (Montgomery 1 among them) at a few positions, different in each row
            for i, e in enumerate(EDGES):
                a[r, (i * 977 + r * 131) % n] = e
        cases[_key((logn, rows, ld, d))] = a
    return cases


def _child(env_value, cin, cout):
    env = dict(os.environ)
    env.pop("LFGPU_FP_TILE1024", None)
    if env_value is not None:
        env["LFGPU_FP_TILE1024"] = env_value
    r = subprocess.run([sys.executable, CHILD, cin, cout], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(cout)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile1024x4")
    cases = _inputs()
    cin = str(d / "cases.npz")
    np.savez(cin, **cases)
    spec = _child(None, cin, str(d / "spec.npz"))
    gen = _child("0", cin, str(d / "gen.npz"))
    return cases, spec, gen


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_key)
def test_tile_1024x4_matches_generic_and_oracle(runs, case):
    """byte-identical to the generic kernel and to the oracle's fftb / fftf; row padding (ld > n) untouched"""
    cases, spec, gen = runs
    logn, rows, ld, d = case
    k, n = _key(case), 1 << logn
    assert spec[k].tobytes() == gen[k].tobytes()
    o = ol.oracle()
    want = cases[k].copy()
    for r in range(rows):
        row = np.ascontiguousarray(want[r, :n])
        (o.lfo_fp_fftf if d == "f" else o.lfo_fp_fftb)(P(row), n, o.lfo_fp_omega32(), 1 << 32)
        want[r, :n] = row
    assert (spec[k] == want).all()


@pytest.mark.gpu
def test_fp_mul_by_montgomery_one_is_identity():
    """Rounds 1-3 of the specialised tile (and pass A's inter-pass product) multiply by w^0 = Montgomery 1 where the generic
    kernel skips the product: that is exact because fp_mul(a, 1) = a for every a < p (the edges of p included)."""
    import torch

    import gpu_util as G
    o = ol.oracle()
    rng = np.random.default_rng(7)
    n = 1 << 16
    x = np.empty((n, 2), dtype=np.uint64)
    x[:, 0] = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    x[:, 1] = rng.integers(0, P_HI + 1, size=n, dtype=np.uint64)
    x[x[:, 1] == P_HI, 0] = 0  # keep every value < p
    x[:len(EDGES)] = EDGES
    assert arr(o.lfo_fp_of_scalar(1)).tolist() == MONT_ONE
    one = np.tile(np.array(MONT_ONE, dtype=np.uint64), (n, 1))
    dout = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    dx, done = G.to_dev(x), G.to_dev(one)
    G.gpu().field_binop(FP, 2, n, dx.data_ptr(), done.data_ptr(), dout.data_ptr())
    assert (G.from_dev(dout, np.uint64, (n, 2)) == x).all()
    assert (arr(o.lfo_fp_mul(elt(x[3]), elt(MONT_ONE))) == x[3]).all()

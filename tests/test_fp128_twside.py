"""K1 at n = 2^20 with the inter-pass product on pass B's load side (csrc/fft.hip, fp_fft_tile_1024x4_tws): the ISA of the two
kernels, and the default launches next to LFGPU_FP_TWSIDE=0 (the product in pass A, as before) and the oracle.  The switch is read
once per process, so each setting runs in a child process of its own (tests/fp_tile_child.py) on the same inputs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fft_isa
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "fp_tile_child.py")
PASS_A = "_Z22fp_fft_tile_1024x4_twsI8Fp128OpsLb0EEv8TilePlanPK5elt_tjS4_j"
PASS_B = "_Z22fp_fft_tile_1024x4_twsI8Fp128OpsLb1EEv8TilePlanPK5elt_tjS4_j"
# kernel: (global loads, VALU ceiling = the count of the built code, 8 elements per thread).  Floors of the arithmetic: 332 per
# element without the inter-pass product, 387 with it.  The pair it replaces: pass B fp_fft_tile_1024x4<.., true, false> 2843
# (no product), pass A fp_fft_tile_1024x4_persist 3332 (with the product); 6175 together against 6090 here.
KERNELS = {
    PASS_A: (9, 2824),   # 353.0 per element
    PASS_B: (17, 3266),  # 408.2 per element
}

P_HI = 0xFFFFF00000000000
MONT_ONE = [0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFF]
EDGES = [[0, 0], [1, 0], [0, P_HI], MONT_ONE, [0xFFFFFFFFFFFFFFFF, P_HI - 1], [0, 1 << 44]]  # 0, 1, p - 1, Montgomery 1, ...


def test_twside_kernels_isa():
    """No scratch, at most 128 VGPRs, every global load a dwordx4 and all of them (the tile's points, pass B's inter-pass
    twiddles, the stage twiddle) issued before the first wait on vector memory; VALU counts pinned; no SCC reader of the
    compiler's after an SCC write inside an asm statement."""
    for k, (nloads, pinned) in KERNELS.items():
        fft_isa.assert_no_scratch_within_128_vgprs(k)
        assert not any(op.startswith(("scratch_", "buffer_")) for op in fft_isa.kernel(k).ops), k
        fft_isa.assert_global_loads(k, nloads)
        fft_isa.assert_no_vmcnt_wait_among_loads(k)
        valu = fft_isa.valu(k)
        print(k, "VALU", valu)
        assert valu <= pinned, (k, valu, pinned)
        fft_isa.assert_scc_clean(k)


def test_no_scalar_memory_writes_in_sources():
    """no source file of the tree names a scalar store, a scalar atomic or a scalar data-cache write-back (documents may)"""
    words = ["s_" + w for w in ("store_dword", "buffer_store_", "scratch_store_", "atomic_", "buffer_atomic_", "dcache_wb", "dcache_discard")]
    pat = re.compile(r"(?<![A-Za-z0-9_])(" + "|".join(re.escape(w) for w in words) + ")", re.I)  # a mnemonic, not limbs_atomic_add
    skip_dirs = {".git", "_ref", "build", "__pycache__", ".pytest_cache"}
    source = (".hip", ".h", ".hpp", ".c", ".cc", ".cpp", ".py", ".sh", ".s", ".S", ".inc", ".cmake", ".mk")
    bad = []
    for d, dirs, files in os.walk(ROOT):
        dirs[:] = [x for x in dirs if x not in skip_dirs]
        for f in files:
            if not (f.endswith(source) or f in ("Makefile", "CMakeLists.txt")):
                continue
            path = os.path.join(d, f)
            with open(path, "rb") as fh:
                if pat.search(fh.read().decode("latin-1")):
                    bad.append(os.path.relpath(path, ROOT))
    assert not bad, bad


# (logn, rows, ld, direction): n = 2^20 both ways with 1, 2, 3 and 5 rows, a strided ld, n = 2^21 .. 2^23 (their inner 2^20-point
# transforms take the same selection, with strided outputs), and n = 2^13 and 2^16, whose pass A is another tile shape: they stay
# on the plan with the product in pass A whatever the switch says
CASES = [(20, r, 1 << 20, d) for r in (1, 2, 3, 5) for d in "bf"]
CASES += [(20, 3, (1 << 20) + 64, "f"), (20, 2, (1 << 20) + 4, "b")]
CASES += [(logn, 1, 1 << logn, d) for logn in (21, 22, 23) for d in "bf"]
CASES += [(13, 3, (1 << 13) + 4, "f"), (13, 2, 1 << 13, "b"), (16, 2, 1 << 16, "f"), (16, 3, (1 << 16) + 8, "b")]


def _key(case):
    return "c_%d_%d_%d_%s" % case


def _inputs():
    rng = np.random.default_rng(20261018)
    cases = {}
    for logn, rows, ld, d in CASES:
        n = 1 << logn
        a = np.empty((rows, ld, 2), dtype=np.uint64)
        a[..., 0] = rng.integers(0, 2**64, size=(rows, ld), dtype=np.uint64)
        a[..., 1] = rng.integers(0, P_HI, size=(rows, ld), dtype=np.uint64)
        a[:, n:] = [0xDEADBEEFDEADBEEF, 0xFFFFFFFFFFFFFFFF]  # beyond the row: must stay as it is
        for r in range(rows):
            for i, e in enumerate(EDGES):
                a[r, (i * 1009 + r * 257 + 5) % n] = e
        cases[_key((logn, rows, ld, d))] = a
    return cases


def _child(env_value, cin, cout):
    env = dict(os.environ)
    for v in ("LFGPU_FP_TWSIDE", "LFGPU_FP_PERSIST", "LFGPU_FP_TILE1024", "LFGPU_FP_TW", "LFGPU_TILE_LOG"):
        env.pop(v, None)
    if env_value is not None:
        env["LFGPU_FP_TWSIDE"] = env_value
    r = subprocess.run([sys.executable, CHILD, cin, cout], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(cout)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("twside")
    cases = _inputs()
    cin = str(d / "cases.npz")
    np.savez(cin, **cases)
    new = _child(None, cin, str(d / "new.npz"))
    old = _child("0", cin, str(d / "old.npz"))
    return cases, new, old


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_key)
def test_twside_matches_product_in_pass_a_and_oracle(runs, case):
    """the default and LFGPU_FP_TWSIDE=0 byte-identical and equal to the oracle's fftb / fftf; row padding (ld > n) untouched"""
    cases, new, old = runs
    logn, rows, ld, d = case
    k, n = _key(case), 1 << logn
    assert new[k].tobytes() == old[k].tobytes()
    o = ol.oracle()
    want = cases[k].copy()
    for r in range(rows):
        row = np.ascontiguousarray(want[r, :n])
        (o.lfo_fp_fftf if d == "f" else o.lfo_fp_fftb)(ol.P(row), n, o.lfo_fp_omega32(), 1 << 32)
        want[r, :n] = row
    assert (new[k] == want).all()

"""K1 at n = 2^20 with lazy butterfly sums (csrc/fft.hip, fp_fft_tile_1024x4_tws; csrc/fp_tile_arith.h): the ISA of the default
kernels and of their canonical partners (LFGPU_FP_LAZY=0), and the two next to each other and to the oracle.

A value in [p, 2^128) turns up with probability 2^-20 per intermediate on random data, so the inputs here are built to make them:
  lo / hi  one half of the row p - 1, the other uniform in [1, 2^108 - 2]: every stage-0 sum of pass A lies in [p, 2^128);
  aout     the columns are inverse transforms of small values (< 2^107), so pass A's outputs are small field elements: a lazy sum
           u + t >= p with a small residue is that residue + p, and pass A stores it so;
  fin      the row is the inverse transform of small values X with X[i] >= X[i + n/2], which makes u and t of pass B's last stage
           small field elements with u >= t: the canonicalisation meets u + p, and left out it would store u + p - t.
A Python-integer model of one 1024-point transform of a tile under the kernel's policy counts what these inputs reach."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fft_isa
import oracle_lib as ol
from test_fp_tile_arith import P, R_INV, ROOT
from test_fp128_twside import EDGES, P_HI

CHILD = os.path.join(ROOT, "tests", "fp_tile_child.py")
ARGS = "I8Fp128OpsLb%dEEv8TilePlanPK5elt_tjS4_j"
# kernel: (global loads, VALU ceiling = the count of the built code, 8 elements per thread).  The lazy counts are the derived ones:
# 36 (pass A) and 32 (pass B) of a thread's 40 butterflies save 3 instructions, and pass B's last stage adds 4 x 8.
KERNELS = {
    "_Z22fp_fft_tile_1024x4_tws" + ARGS % 0: (9, 2716),  # 339.5 per element
    "_Z22fp_fft_tile_1024x4_tws" + ARGS % 1: (17, 3202),  # 400.2 per element
    "_Z28fp_fft_tile_1024x4_tws_canon" + ARGS % 0: (9, 2824),
    "_Z28fp_fft_tile_1024x4_tws_canon" + ARGS % 1: (17, 3266),
}
T128 = 2**128
N = 1 << 20
PAD = [0xDEADBEEFDEADBEEF, 0xFFFFFFFFFFFFFFFF]


def test_lazy_kernels_isa():
    """No scratch, at most 128 VGPRs, every global load a dwordx4 and all of them issued before the first wait on vector memory;
    VALU counts pinned; no SCC reader of the compiler's after an SCC write inside an asm statement."""
    for k, (nloads, pinned) in KERNELS.items():
        fft_isa.assert_no_scratch_within_128_vgprs(k)
        assert not any(op.startswith(("scratch_", "buffer_")) for op in fft_isa.kernel(k).ops), k
        fft_isa.assert_global_loads(k, nloads)
        fft_isa.assert_no_vmcnt_wait_among_loads(k)
        valu = fft_isa.valu(k)
        print(k, "VALU", valu)
        assert valu <= pinned, (k, valu, pinned)
        fft_isa.assert_scc_clean(k)


# ------------------------------------------------------------------ inputs
def _fft(a, n, d):
    """the oracle's fftb / fftf, in place, on every row of the contiguous (rows, n, 2) array a"""
    o = ol.oracle()
    f = o.lfo_fp_fftf if d == "f" else o.lfo_fp_fftb
    for r in range(a.shape[0]):
        f(ol.P(a[r]), n, o.lfo_fp_omega32(), 1 << 32)


def _random(rng, shape):
    a = np.empty(shape + (2,), dtype=np.uint64)
    a[..., 0] = rng.integers(0, 2**64, size=shape, dtype=np.uint64)
    a[..., 1] = rng.integers(0, P_HI, size=shape, dtype=np.uint64)
    return a


def _small(rng, shape, bits):
    a = np.empty(shape + (2,), dtype=np.uint64)
    a[..., 0] = rng.integers(0, 2**64, size=shape, dtype=np.uint64)
    a[..., 1] = rng.integers(0, 1 << (bits - 64), size=shape, dtype=np.uint64)
    return a


def _rnd(rng, n, r=0):
    a = _random(rng, (n,))
    for i, e in enumerate(EDGES):
        a[(i * 1009 + r * 257 + 5) % n] = e
    return a


def _flood(rng, swap):
    a = np.empty((N, 2), dtype=np.uint64)
    a[:] = [0, P_HI]  # p - 1
    u = _small(rng, (N // 2,), 108)  # [1, 2^108 - 2]
    u[:, 0] = np.clip(u[:, 0], np.uint64(1), np.uint64(2**64 - 2))
    if swap:
        a[:N // 2] = u
    else:
        a[N // 2:] = u
    return a


def _aout(rng, d):
    """pass A's output Y[j1][k2] (the 1024-point transform of column k2) = 1024 y, y < 2^97"""
    y = _small(rng, (1024, 1024), 97)  # [j1][k2]
    cols = np.ascontiguousarray(y.transpose(1, 0, 2))  # [k2][j1]
    _fft(cols, 1024, "b" if d == "f" else "f")  # the other direction: 1024 x the inverse
    return np.ascontiguousarray(cols.transpose(1, 0, 2)).reshape(N, 2)  # a[1024 k1 + k2]


def _fin(rng, d):
    """the transform X of the row = n x with x[i] = g + h, x[i + n/2] = g - h, 0 <= h <= g < 2^60: pass B's last stage pairs these two
    outputs, so its u = n g and t = n h are small field elements, and without the canonicalisation u - t would be stored as n (g - h) + p"""
    g = rng.integers(0, 2**60, size=N // 2, dtype=np.uint64)
    h = rng.integers(0, 2**60, size=N // 2, dtype=np.uint64) % (g + np.uint64(1))
    x = np.zeros((1, N, 2), dtype=np.uint64)
    x[0, :N // 2, 0] = g + h
    x[0, N // 2:, 0] = g - h
    _fft(x, N, "b" if d == "f" else "f")  # the other direction: n x the inverse
    return x[0]


STRUCTURED = ("lo", "hi", "aout", "fin")
# (name, logn, rows, ld, direction): the fifth field is the row stride, as fp_tile_child.py reads it
CASES = [(name, 20, 1, N, d) for d in "bf" for name in ("rnd",) + STRUCTURED]
CASES += [("mix", 20, 3, N + 64, d) for d in "bf"]  # rows: rnd, lo, fin
CASES += [("rnd", 21, 1, 1 << 21, d) for d in "bf"]


def _key(case):
    return "%s_%d_%d_%d_%s" % case


@functools.lru_cache(maxsize=None)
def _structured(name, d):
    rng = np.random.default_rng([20261020, STRUCTURED.index(name), "bf".index(d)])
    a = {"lo": lambda: _flood(rng, False), "hi": lambda: _flood(rng, True), "aout": lambda: _aout(rng, d), "fin": lambda: _fin(rng, d)}[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(20261021)
    cases = {}
    for case in CASES:
        name, logn, rows, ld, d = case
        n = 1 << logn
        a = np.empty((rows, ld, 2), dtype=np.uint64)
        a[:, n:] = PAD  # beyond the row: must stay as it is
        if name == "mix":
            a[0, :n], a[1, :n], a[2, :n] = _rnd(rng, n, 1), _structured("lo", d), _structured("fin", d)
        elif name == "rnd":
            a[0, :n] = _rnd(rng, n)
        else:
            a[0, :n] = _structured(name, d)
        cases[_key(case)] = a
    return cases


# ------------------------------------------------------------------ the coverage model
def _ints(a):
    return [l | (h << 64) for l, h in zip(a[..., 0].reshape(-1).tolist(), a[..., 1].reshape(-1).tolist())]


@functools.lru_cache(maxsize=None)
def _root(d):
    """w_n, n = 2^20, as a plain integer: the oracle's root of order 2^32 out of Montgomery form, to the power 2^12; inverted for fftf"""
    e = ol.oracle().lfo_fp_omega32()
    w = pow((int(e.l[0]) | (int(e.l[1]) << 64)) * R_INV % P, 1 << 12, P)
    return pow(w, -1, P) if d == "f" else w


COUNTS = ("lazy add u", "lazy sub u", "product a", "final canon", "round-0 full add inputs", "final canon decides")
BITREV10 = [int(format(i, "010b")[::-1], 2) for i in range(1024)]


def tile_model(x, w1024, out_canon, cnt):
    """One 1024-point transform of a tile as t4_stages runs it: the values as 128-bit integers, the policy of the default kernels.
    x: the 1024 points, canonical (pass A: the caller's; pass B: after the inter-pass product).  Stage s pairs positions i and
    i + 2^s of the bit-reversed order with w_1024^((i mod 2^s) 2^(9-s)); round 0 (s < 3) leaves the w^0 products out, its sums
    (2,3), (6,7), (4,5) at stage 0 and (4,6) at stage 1 are full adds; every other sum is lazy; out_canon (pass B): the last stage
    makes u canonical and adds in full.  cnt counts the values >= p met as a lazy add's / sub's u, as a product's a and by the
    canonicalisation (and how often a stored value depends on it), and the canonical inputs of the full adds of round 0."""
    X = [x[BITREV10[i]] for i in range(1024)]
    wt = [1] * 512
    for i in range(1, 512):
        wt[i] = wt[i - 1] * w1024 % P
    for s in range(10):
        half = 1 << s
        last = out_canon and s == 9
        for i in range(1024):
            if i & half:
                continue
            jj, a = i & (half - 1), i & 7
            u, v = X[i], X[i + half]
            if s < 3 and jj == 0:
                assert v < P, (s, i)  # not multiplied: it has to be canonical as it stands
                t = v
            else:
                cnt["product a"] += v >= P
                t = v * wt[jj << (9 - s)] % P
            full0 = s < 3 and ((s == 0 and a != 0) or (s == 1 and a == 4))
            if last:
                cnt["final canon"] += u >= P
                cnt["final canon decides"] += u + t >= 2 * P or u - t >= P  # what fpt_add / fpt_sub would store differs
                u %= P
            if last or full0:
                assert u < P and t < P, (s, i)
                cnt["round-0 full add inputs"] += 2 * full0
                X[i] = (u + t) % P
            else:
                cnt["lazy add u"] += u >= P
                X[i] = u + t if u + t < T128 else u + t - P
            cnt["lazy sub u"] += u >= P
            X[i + half] = u - t if u >= t else u - t + P
    assert all(0 <= v < T128 for v in X)
    return X


def _dft1024(x, d):
    """the oracle's 1024-point transform of the integers x (< p), as integers"""
    a = np.array([[v & (2**64 - 1), v >> 64] for v in x], dtype=np.uint64).reshape(1, 1024, 2)
    _fft(a, 1024, d)
    return _ints(a)


def _model_case(name, d, cols, rows, cnt):
    """pass A's transforms of the columns `cols` and pass B's of the rows `rows` of one structured input; each is checked
    against the oracle's 1024-point transform.  What pass A stores is the a of pass B's first product."""
    wn = _root(d)
    w1024 = pow(wn, 1024, P)
    a = _structured(name, d).reshape(1024, 1024, 2)  # [k1][k2]
    for k2 in cols:
        x = _ints(a[:, k2])
        y = tile_model(x, w1024, False, cnt)
        assert [v % P for v in y] == _dft1024(x, d), (name, d, k2)
        cnt["product a"] += sum(v >= P for v in y)
    if rows:
        y = np.ascontiguousarray(a.transpose(1, 0, 2))  # [k2][k1] -> the oracle's pass A -> [k2][j1]
        _fft(y, 1024, d)
        for j1 in rows:
            z = [v * pow(wn, j1 * k2, P) % P for k2, v in enumerate(_ints(y[:, j1]))]
            out = tile_model(z, w1024, True, cnt)
            assert out == _dft1024(z, d), (name, d, j1)


def test_structured_inputs_reach_the_lazy_paths():
    """over the structured inputs, in the tiles modelled (a few of each case's 2 x 256), each kind of non-canonical value is met
    at least 100 times, and the full adds of round 0 see canonical inputs only (the model asserts it)"""
    total = dict.fromkeys(COUNTS, 0)
    for d in "bf":
        for name, cols, rows in (("lo", range(4), ()), ("hi", range(4), ()), ("aout", (0, 5), (0, 3)), ("fin", (), (0, 1, 2, 7))):
            cnt = dict.fromkeys(COUNTS, 0)
            _model_case(name, d, cols, rows, cnt)
            print(name, d, cnt)
            for c in COUNTS:
                total[c] += cnt[c]
    print("total", total)
    for c in COUNTS:
        assert total[c] >= 100, (c, total)


# ------------------------------------------------------------------ on the GPU
def _child(lazy, cin, cout):
    env = dict(os.environ)
    for v in ("LFGPU_FP_LAZY", "LFGPU_FP_TWSIDE", "LFGPU_FP_PERSIST", "LFGPU_FP_TILE1024", "LFGPU_FP_TW", "LFGPU_FP_ROWFAST", "LFGPU_TILE_LOG"):
        env.pop(v, None)
    if lazy is not None:
        env["LFGPU_FP_LAZY"] = lazy
    r = subprocess.run([sys.executable, CHILD, cin, cout], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(cout)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lazy")
    cin = str(d / "cases.npz")
    np.savez(cin, **_inputs())
    return _child(None, cin, str(d / "lazy.npz")), _child("0", cin, str(d / "canon.npz"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_key)
def test_lazy_matches_canonical_and_oracle(runs, case):
    """the default and LFGPU_FP_LAZY=0 byte-identical and equal to the oracle's fftb / fftf; row padding (ld > n) untouched"""
    lazy, canon = runs
    name, logn, rows, ld, d = case
    k, n = _key(case), 1 << logn
    assert lazy[k].tobytes() == canon[k].tobytes()
    want = _inputs()[k].copy()
    rowsn = np.ascontiguousarray(want[:, :n])
    _fft(rowsn, n, d)
    want[:, :n] = rowsn
    assert (lazy[k] == want).all()

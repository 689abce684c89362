"""The lazy u side of K1's butterflies (csrc/fp_tile_arith.h): fpt_add_lazy(u, t) and fpt_sub(u, t) with u any 128-bit value
congruent to the element and t < p, fpt_mul(a, w) with a lazy, and fpt_canon.

A word-by-word model of fpt_add_lazy and fpt_canon (32-bit limbs, the carry mask, the borrow-in chain) and the model of
fpt_mul's reduction from test_fp_tile_redc.py are checked against Python integers, with every case of each reached at least 100
times; on the GPU the four routines run on the same edge grid and on 2^20 random pairs."""
import os
import subprocess

import numpy as np
import pytest

from test_fp_tile_arith import MONT_ONE, P, R_INV, ROOT, _hipcc
from test_fp_tile_redc import CASES as REDC_CASES
from test_fp_tile_redc import M32, P3, _add_chain, _from_words, _sub_chain, redc_model

CHECK = os.path.join(ROOT, "tests", "fp_tile_lazy_check.hip")
T128 = 2**128
U_EDGES = [0, 1, P - 1, P, P + 1, T128 - 1, T128 - 2**108, 2**108 - 1]
T_EDGES = [0, 1, P - 1, MONT_ONE]
ADD_CASES = ("carry, folded", "no carry, result < p", "no carry, result in [p, 2^128)")
CANON_CASES = ("canon subtracts", "canon keeps")


def _words(x):
    return [(x >> (32 * i)) & M32 for i in range(4)]


def add_lazy_model(u, t):
    """fpt_add_lazy: four carry adds, then - p under the carry mask (v_cndmask for limb 3, the mask as borrow-in)"""
    s, c = _add_chain(_words(u), _words(t))
    e3 = P3 if c else 0  # v_cndmask_b32
    d, _ = _sub_chain(s, [0, 0, 0, e3], c)  # 3 v_subbrev_co + v_subb_co
    r = _from_words(d)
    return r, ADD_CASES[0] if c else ADD_CASES[1] if r < P else ADD_CASES[2]


def canon_model(u):
    """fpt_canon: the trial u - p and four selects under its borrow"""
    w = _words(u)
    d, b = _sub_chain(w, [1, 0, 0, P3])
    return _from_words(w if b else d), CANON_CASES[1] if b else CANON_CASES[0]


def _rand_lazy(rng, n):
    """n values, half from [p, 2^128) and half from [0, 2^128)"""
    raw = [int.from_bytes(rng.bytes(16), "little") for _ in range(n)]
    return [P + x % (T128 - P) if i & 1 else x for i, x in enumerate(raw)]


def _rand_canon(rng, n):
    return [int.from_bytes(rng.bytes(16), "little") % P for _ in range(n)]


def test_add_lazy_and_canon_models():
    rng = np.random.default_rng(20261017)
    pairs = [(u, t) for u in U_EDGES for t in T_EDGES]
    pairs += list(zip(_rand_lazy(rng, 40000), _rand_canon(rng, 40000)))
    # small t under a u just above p: the sum stays in [p, 2^128)
    pairs += [(u, t % 2**100) for u, t in zip(_rand_lazy(rng, 2000), _rand_canon(rng, 2000))]
    counts = dict.fromkeys(ADD_CASES + CANON_CASES, 0)
    for u, t in pairs:
        r, case = add_lazy_model(u, t)
        assert r < T128 and (r - u - t) % P == 0, (hex(u), hex(t), hex(r))
        assert r == (u + t if u + t < T128 else u + t - P), (hex(u), hex(t), hex(r))
        counts[case] += 1
        r, case = canon_model(u)
        assert r == u % P, (hex(u), hex(r))
        counts[case] += 1
    print(counts)
    for c, k in counts.items():
        assert k >= 100, (c, counts)


def _lazy_product_pairs(rng):
    """(a, w), a in [p, 2^128), w < p, reaching every case of the reduction: U = 0 needs T_lo = 0 (w = 0, or a and w multiples
    of 2^64), k = 0 needs t0 a multiple of 2^20"""
    hi = lambda: int(rng.integers((P >> 64) + 1, 2**64, dtype=np.uint64))
    pairs = [(a, w) for a in U_EDGES if a >= P for w in T_EDGES]
    pairs += list(zip(_rand_lazy(rng, 20000)[1::2], _rand_canon(rng, 10000)))
    pairs += [(a, 0) for a in _rand_lazy(rng, 300)[1::2]]
    pairs += [(hi() << 64, int(rng.integers(1, 2**63)) << 64) for _ in range(150)]
    pairs += [(a >> 20 << 20, w) for a, w in zip(_rand_lazy(rng, 600)[1::2], _rand_canon(rng, 300))]
    pairs += [(a, w >> 20 << 20) for a, w in zip(_rand_lazy(rng, 600)[1::2], _rand_canon(rng, 300))]
    return [(a, w) for a, w in pairs if P <= a < T128 and w < P]


def test_redc_model_takes_a_lazy_operand():
    counts = dict.fromkeys(REDC_CASES, 0)
    for a, w in _lazy_product_pairs(np.random.default_rng(109)):
        got, cases = redc_model(a * w)
        assert got == (a % P) * w * R_INV % P, (hex(a), hex(w), hex(got))
        for c in cases:
            counts[c] += 1
    print(counts)
    for c, k in counts.items():
        assert k >= 100, (c, counts)


def _ints(a):
    """(n, 2) uint64 limbs -> Python integers"""
    return [l | (h << 64) for l, h in zip(a[:, 0].tolist(), a[:, 1].tolist())]


@pytest.mark.gpu
def test_lazy_arith_device(tmp_path):
    exe = tmp_path / "fp_tile_lazy_check"
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", str(exe), CHECK])
    rng = np.random.default_rng(20261019)
    nrand = 1 << 20
    edge = np.array([[u & (2**64 - 1), u >> 64, t & (2**64 - 1), t >> 64] for u in U_EDGES for t in T_EDGES], dtype=np.uint64)
    rnd = rng.integers(0, 2**64, size=(nrand, 4), dtype=np.uint64)
    rnd[:, 3] = rng.integers(0, P >> 64, size=nrand, dtype=np.uint64)  # t < p
    # every second u in [p, 2^128): the top 20 bits set and the lowest one (p = 2^128 - 2^108 + 1)
    rnd[1::2, 1] = (rnd[1::2, 1] >> np.uint64(20)) | np.uint64(P >> 64)
    rnd[1::2, 0] |= np.uint64(1)
    arr = np.concatenate([edge, rnd])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    arr.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(fout, dtype=np.uint64).reshape(len(arr), 4, 2)
    us, ts = _ints(arr[:, 0:2]), _ints(arr[:, 2:4])
    assert sum(u >= P for u in us) >= nrand // 2 and all(t < P for t in ts)
    add, sub, mul, can = (_ints(got[:, i]) for i in range(4))
    for i, (u, t) in enumerate(zip(us, ts)):
        ok = (add[i] - u - t) % P == 0 and (sub[i] - u + t) % P == 0 and mul[i] == u * t * R_INV % P and can[i] == u % P
        assert ok, (hex(u), hex(t), hex(add[i]), hex(sub[i]), hex(mul[i]), hex(can[i]))

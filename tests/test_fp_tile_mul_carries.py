"""The carries that fpt_mul (csrc/fp_tile_arith.h) does not capture: the first v_mad_u64_u32 of columns 3, 4 and 5 of the product
scan T = a w is a_i * b3, and b3 <= 0xfffff000 for every w < p = 2^128 - 2^108 + 1, so

    {acc.hi, ov} + a_i b3  <  2^34 + (2^32 - 1) 0xfffff000  =  2^64 - 2^44 + 2^34 - 2^32 + 2^12  <  2^64

whatever a is (lazy values included): that mad needs no v_addc behind it, and the column's second mad is the one whose capture
writes ov.  52 VALU instructions per product instead of 55.

A word-by-word model of the column schedule on Python integers (32-bit limbs, a 64-bit accumulator that wraps, ov) asserts at every
uncaptured mad that the true sum is below 2^64 and that T = a w exactly; through the reduction's model of test_fp_tile_redc.py the
result is a w / 2^128 mod p.  The bound is tight in its assumption: with b3 = 0xffffffff (no field element) column 3's uncaptured
mad wraps, and with column 3's second mad uncaptured as well (a1 b2: nothing bounds it) the structured inputs below wrap too.  On the
GPU fpt_mul runs on the same structured pairs and on random ones, 2^20 in all; the VALU counts of the four 2^20-point tile kernels
are pinned at the derived figures, 3 less per product than in test_fp128_lazy_fft.py."""
import os
import subprocess

import numpy as np
import pytest

import fft_isa
from test_fp_tile_arith import EDGES, MONT_ONE, P, R_INV, ROOT, _hipcc
from test_fp_tile_redc import M32, redc_model

CHECK = os.path.join(ROOT, "tests", "fp_tile_mul_check.hip")
T128 = 2**128
M64 = 2**64 - 1
MAD, MADW, MADC = "no capture", "capture writes ov", "capture adds to ov"
# fpt_mul's columns: (i, j, what becomes of the carry-out of acc += a_i * b_j)
SCHEDULE = (
    ((0, 0, MAD),),
    ((0, 1, MAD), (1, 0, MADW)),
    ((0, 2, MADW), (1, 1, MADC), (2, 0, MADC)),
    ((0, 3, MAD), (1, 2, MADW), (2, 1, MADC), (3, 0, MADC)),
    ((1, 3, MAD), (2, 2, MADW), (3, 1, MADC)),
    ((2, 3, MAD), (3, 2, MADW)),
    ((3, 3, MAD),),
)
# column 2's first mad (a0 b2) uncaptured as well: see test_column_2_first_mad_never_carries
SCHEDULE_COL2 = SCHEDULE[:2] + (((0, 2, MAD), (1, 1, MADW), (2, 0, MADC)),) + SCHEDULE[3:]
# column 3's second mad (a1 b2) uncaptured as well, for which no bound holds (the sensitivity check of the inputs)
SCHEDULE_COL3 = SCHEDULE[:3] + (((0, 3, MAD), (1, 2, MAD), (2, 1, MADW), (3, 0, MADC)),) + SCHEDULE[4:]

W_TOP = 0xFFFFEFFF_FFFFFFFF_FFFFFFFF_FFFFFFFF  # the largest w < p with b3 < 0xfffff000: b3 = 0xfffff000 - 1, the rest all ones
# w that push the incoming accumulator and the b3 product up together; p - 1 = (0, 0, 0, 0xfffff000) has the largest b3 there is
W_STRUCT = [W_TOP, P - 1, P - 2, 0xFFFFEFFF << 96, (0xFFFFEFFF << 96) | M32, W_TOP ^ (M32 << 64), W_TOP ^ (M32 << 32), W_TOP - 1,
            (0xFFFFEFFF << 96) | (M32 << 64), MONT_ONE, 1, 0]
# lazy a: all limbs 0xffffffff, and others in [p, 2^128)
A_LAZY = [T128 - 1, P, P + 1, T128 - 2, T128 - 2**107, T128 - 2**32, T128 - 2**64 - 1, T128 - 2**96, P + (MONT_ONE >> 1), (P + 2**107) | M64,
          T128 - 2**33, T128 - 2**65 - 2**31]


class Wrap(AssertionError):
    """an uncaptured mad's true sum reached 2^64"""


def _words(x):
    return [(x >> (32 * i)) & M32 for i in range(4)]


def mul_model(a, w, schedule=SCHEDULE):
    """T = (t0 .. t7) as fpt_mul forms it: the carry of column k goes to ov, the high half of column k + 1's accumulator"""
    aw, bw = _words(a), _words(w)
    acc, ov, t = 0, 0, []
    for k, col in enumerate(schedule):
        for i, j, kind in col:
            s = acc + aw[i] * bw[j]  # v_mad_u64_u32
            acc, c = s & M64, s >> 64
            if kind == MAD:
                if c:
                    raise Wrap((k, i, j, hex(a), hex(w)))
            elif kind == MADW:
                ov = c
            else:
                ov += c
        if k < 6:
            t.append(acc & M32)
            acc = (acc >> 32) | (ov << 32) if k else acc >> 32  # FPT_COL; column 0 has no carry
        else:
            t += [acc & M32, acc >> 32]
    return sum(x << (32 * i) for i, x in enumerate(t))


def _structured_pairs():
    pairs = [(a, w) for a in EDGES for w in EDGES]
    pairs += [(a, w) for a in A_LAZY for w in W_STRUCT + EDGES]
    pairs += [(a, w) for a in EDGES for w in W_STRUCT]
    assert all(a < T128 and w < P for a, w in pairs)
    return pairs


def _check_pair(a, w):
    T = mul_model(a, w)
    assert T == a * w, (hex(a), hex(w), hex(T))
    got, _ = redc_model(T)
    assert got == a * w * R_INV % P, (hex(a), hex(w), hex(got))


def test_mul_model_structured():
    pairs = _structured_pairs()
    assert (T128 - 1, W_TOP) in pairs and (T128 - 1, P - 1) in pairs
    for a, w in pairs:
        _check_pair(a, w)


def test_mul_model_random():
    rng = np.random.default_rng(20261018)
    for _ in range(100000):
        raw = rng.bytes(32)
        _check_pair(int.from_bytes(raw[:16], "little"), int.from_bytes(raw[16:], "little") % P)


def test_bound_needs_w_below_p():
    """b3 = 0xffffffff: column 3's accumulator comes in at about 2 * 2^32 * 2^32 and a0 b3 = 2^64 - 2^33 + 1 wraps it.  Model only:
    no kernel is called with such a w."""
    with pytest.raises(Wrap) as e:
        mul_model(T128 - 1, T128 - 1)
    assert e.value.args[0][:3] == (3, 0, 3)
    # the same a against the largest field elements stays below 2^64 at every uncaptured mad
    for w in (P - 1, W_TOP):
        assert mul_model(T128 - 1, w) == (T128 - 1) * w


def test_structured_inputs_reach_the_carries():
    """With one more mad of column 3 uncaptured (a1 b2, which nothing bounds) the structured pair (all ones, W_TOP) wraps, and so
    do at least 100 of the structured pairs: the inputs reach the carries that matter."""
    with pytest.raises(Wrap) as e:
        mul_model(T128 - 1, W_TOP, SCHEDULE_COL3)
    assert e.value.args[0][:3] == (3, 1, 2)
    wraps = 0
    for a, w in _structured_pairs():
        try:
            assert mul_model(a, w, SCHEDULE_COL3) == a * w
        except Wrap:
            wraps += 1
    print("wraps", wraps)
    assert wraps >= 100, wraps


def test_column_2_first_mad_never_carries():
    """Not used by fpt_mul, which keeps column 2's three captures; recorded because it is easy to take for granted the other way.
    Column 1's true sum is at most (2^32 - 2) + 2 (2^32 - 1)^2 = 2^65 - 3 2^32, so column 2's accumulator comes in at no more than
    2^33 - 3, and a0 b2 <= 2^64 - 2^33 + 1 brings it to 2^64 - 2 at the most: that mad cannot carry for any a and any w, field
    element or not.  The maximum is reached by all ones on both sides, and the structured pairs stay below 2^64 as well."""
    aw = [M32] * 4
    s1 = (aw[0] * aw[0] >> 32) + 2 * aw[0] * aw[1]
    assert s1 == 2**65 - 3 * 2**32 and (s1 >> 32) + aw[0] * aw[2] == 2**64 - 2
    for a, w in _structured_pairs():
        assert mul_model(a, w, SCHEDULE_COL2) == a * w


def _limbs(x):
    return [x & M64, x >> 64]


def _ints(a):
    """(n, 2) uint64 limbs -> Python integers"""
    return [l | (h << 64) for l, h in zip(a[:, 0].tolist(), a[:, 1].tolist())]


@pytest.mark.gpu
def test_mul_carries_device(tmp_path):
    exe = tmp_path / "fp_tile_mul_check"
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", str(exe), CHECK])
    n = 1 << 20
    st = np.array([_limbs(a) + _limbs(w) for a, w in _structured_pairs()], dtype=np.uint64)
    st = np.tile(st, (-(-(1 << 16) // len(st)), 1))  # repeated: every lane position of a wave meets them
    rng = np.random.default_rng(20261020)
    rnd = rng.integers(0, 2**64, size=(n - len(st), 4), dtype=np.uint64)
    rnd[:, 3] = rng.integers(0, P >> 64, size=len(rnd), dtype=np.uint64)  # w < p
    # every second a in [p, 2^128): the top 20 bits set and the lowest one
    rnd[1::2, 1] = (rnd[1::2, 1] >> np.uint64(20)) | np.uint64(P >> 64)
    rnd[1::2, 0] |= np.uint64(1)
    arr = np.concatenate([st, rnd])
    assert len(arr) == n
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    arr.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = _ints(np.fromfile(fout, dtype=np.uint64).reshape(n, 2))
    As, Ws = _ints(arr[:, 0:2]), _ints(arr[:, 2:4])
    assert sum(a >= P for a in As) >= n // 4 and all(w < P for w in Ws)
    for a, w, g in zip(As, Ws, got):
        assert g == a * w * R_INV % P, (hex(a), hex(w), hex(g))


ARGS = "I8Fp128OpsLb%dEEv8TilePlanPK5elt_tjS4_j"
# VALU ceilings, 8 elements per thread: the counts of test_fp128_lazy_fft.py less 3 for each of a thread's products, 33 in pass A
# and 41 in pass B
KERNELS = {
    "_Z22fp_fft_tile_1024x4_tws" + ARGS % 0: 2716 - 3 * 33,  # 2617
    "_Z22fp_fft_tile_1024x4_tws" + ARGS % 1: 3202 - 3 * 41,  # 3079
    "_Z28fp_fft_tile_1024x4_tws_canon" + ARGS % 0: 2824 - 3 * 33,  # 2725
    "_Z28fp_fft_tile_1024x4_tws_canon" + ARGS % 1: 3266 - 3 * 41,  # 3143
}


def test_tile_kernels_valu_after_dead_captures():
    for k, pinned in KERNELS.items():
        fft_isa.assert_no_scratch_within_128_vgprs(k)
        valu = fft_isa.valu(k)
        print(k, "VALU", valu)
        assert valu <= pinned, (k, valu, pinned)

"""The Montgomery reduction step of fpt_mul (csrc/fp_tile_arith.h): W = T_hi - U + (U >> 20) + cy, plus p when W < 0.

A word-by-word model of the asm on Python integers (the same words, carries and lane masks) is checked against
a * b / 2^128 mod p on products and against T / 2^128 mod p on structured 256-bit T, with each of the step's five cases
reached at least 100 times: U = 0, t0 mod 2^20 = 0 with U != 0, cy = 1, the + p fix taken and not taken.  The tile
kernels' VALU counts are pinned from the gfx950 ISA, and on the GPU fpt_mul runs on inputs that reach every case."""
import subprocess

import numpy as np
import pytest

import fft_isa
from test_fp_tile_arith import CHECK, EDGES, P, P_HI, R_INV, _hipcc, _limbs

M32 = 2**32 - 1
P3 = 0xFFFFF000  # p's top word
CASES = ("U = 0", "t0 mod 2^20 = 0, U != 0", "cy = 1", "+p taken", "+p not taken")
# the words that structured inputs are built from: the carries and the 20-bit boundary of the reduction
WORDS = [0, 1, 2, 2**12, 2**20 - 1, 2**20, 2**20 + 1, 0xFFF00000, 0xFFFFF000, 0xFFFFF001, 2**31, M32 - 1, M32]


def _sub_chain(x, y, bin_=0):
    """v_sub_co / v_subb_co over four words: (words, borrow-out)"""
    out = []
    for xi, yi in zip(x, y):
        d = xi - yi - bin_
        out.append(d & M32)
        bin_ = int(d < 0)
    return out, bin_


def _add_chain(x, y, cin=0):
    """v_add_co / v_addc_co over four words: (words, carry-out)"""
    out = []
    for xi, yi in zip(x, y):
        s = xi + yi + cin
        out.append(s & M32)
        cin = s >> 32
    return out, cin


def redc_model(T):
    """fpt_mul's reduction of the 256-bit product T = (t0 .. t7): (result, the set of CASES it went through)"""
    t = [(T >> (32 * i)) & M32 for i in range(8)]
    k = (t[0] << 12) & M32
    s = t[3] + k  # v_add_co_u32 u3, cy
    u3, cy = s & M32, s >> 32
    sh = [((t[1] << 32 | t[0]) >> 20) & M32, ((t[2] << 32 | t[1]) >> 20) & M32, ((u3 << 32 | t[2]) >> 20) & M32,
          u3 >> 20]  # 3 v_alignbit_b32 + v_lshrrev_b32
    d, b = _sub_chain(t[4:], [t[0], t[1], t[2], u3])  # T_hi - U
    d, c = _add_chain(d, sh, cy)  # + (U >> 20) + cy
    neg = b & (1 - c)  # s_andn2_b64
    d, _ = _add_chain(d, [0, 0, 0, P3 if neg else 0], neg)  # v_cndmask_b32 + 4 v_addc_co
    U = t[0] | t[1] << 32 | t[2] << 64 | u3 << 96
    cases = set()
    if U == 0:
        cases.add(CASES[0])
    elif k == 0:
        cases.add(CASES[1])
    if cy:
        cases.add(CASES[2])
    cases.add(CASES[3] if neg else CASES[4])
    return d[0] | d[1] << 32 | d[2] << 64 | d[3] << 96, cases


def _rand_elt(rng):
    x = int.from_bytes(rng.bytes(16), "little") % P
    if rng.integers(4) == 0:  # top 20 bits set
        x = (x | (P_HI << 64)) % P
    return x


def _from_words(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def _product_pairs(rng):
    pairs = [(a, b) for a in EDGES for b in EDGES]
    pairs += [(_rand_elt(rng), _rand_elt(rng)) for _ in range(100000)]
    # U = 0 needs T_lo = 0: a zero operand, or a = 2^64 a', b = 2^64 b' (T = 2^128 a' b'), 2^64 * 2^64 among them
    pairs += [(0, _rand_elt(rng)) for _ in range(100)] + [(_rand_elt(rng), 0) for _ in range(100)]
    pairs += [(2**64, 2**64)] + [(int(rng.integers(1, 2**63)) << 64, int(rng.integers(1, 2**63)) << 64) for _ in range(200)]
    return pairs


def _structured_T(rng, n):
    """n 256-bit T with words from WORDS and T_hi < p (so that T < p 2^128, as every product of two canonical values)"""
    out = []
    while len(out) < n:
        T = _from_words(rng.choice(WORDS, 8).tolist())
        if T >> 128 < P:
            out.append(T)
    return out


def _check(items, want):
    counts = dict.fromkeys(CASES, 0)
    for x in items:
        T, ref = want(x)
        got, cases = redc_model(T)
        assert got == ref, (hex(T), hex(got), hex(ref))
        for c in cases:
            counts[c] += 1
    return counts


def test_redc_model_products():
    rng = np.random.default_rng(20261016)
    counts = _check(_product_pairs(rng), lambda ab: (ab[0] * ab[1], ab[0] * ab[1] * R_INV % P))
    print("products:", counts)
    assert counts["U = 0"] >= 100, counts


def test_redc_model_structured():
    rng = np.random.default_rng(108)
    Ts = _structured_T(rng, 100000)
    # T_lo = 0 (U = 0, the result is T_hi), on its own
    Ts += [T >> 128 << 128 for T in _structured_T(rng, 1000)]
    counts = _check(Ts, lambda T: (T, T * R_INV % P))
    print("structured T:", counts)
    for c in CASES:
        assert counts[c] >= 100, (c, counts)


def _device_pairs(rng):
    """(a, 1) and (a, 2^j), a's words from WORDS (so T is a shifted), plus (0, x), (x, 0) and (2^64, 2^64); random pairs
    add the fix not taken with U != 0, which shifted values seldom reach (T_hi must be about U)"""
    As = sorted({a for a in (_from_words(rng.choice(WORDS, 4).tolist()) for _ in range(6000)) if a < P})
    pairs = [(a, 1) for a in As]
    pairs += [(a, 1 << j) for j in range(128) for a in rng.choice(As, 64).tolist()]
    pairs += [(0, a) for a in As[:200]] + [(a, 0) for a in As[:200]] + [(2**64, 2**64)]
    pairs += [(_rand_elt(rng), _rand_elt(rng)) for _ in range(2000)]
    return pairs


def test_device_pairs_cover_every_case():
    """the pairs that test_tile_redc_device runs reach every case of the reduction step at least 100 times"""
    counts = _check(_device_pairs(np.random.default_rng(7)), lambda ab: (ab[0] * ab[1], ab[0] * ab[1] * R_INV % P))
    print("device pairs:", counts)
    for c in CASES:
        assert counts[c] >= 100, (c, counts)


@pytest.mark.gpu
def test_tile_redc_device(tmp_path):
    exe = tmp_path / "fp_tile_arith_check"
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", str(exe), CHECK])
    pairs = _device_pairs(np.random.default_rng(7))
    arr = np.array([_limbs(a) + _limbs(b) for a, b in pairs], dtype=np.uint64)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    arr.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout), "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(fout, dtype=np.uint64).reshape(len(pairs), 3, 2)
    for (a, b), g in zip(pairs, got):
        val = [int(g[i][0]) | (int(g[i][1]) << 64) for i in range(3)]
        assert val == [a * b * R_INV % P, (a + b) % P, (a - b) % P], (hex(a), hex(b), [hex(v) for v in val])


# VALU instructions in each kernel's body after the shorter reduction (55 instead of 63 per product; 33 products per
# thread in pass B, 41 in pass A); the parent's pins are those of test_fp_tile_arith.py
KERNELS = {
    "_Z18fp_fft_tile_1024x4I8Fp128OpsLb1ELb0EEv8TilePlanPK5elt_tjS4_j": 2843,  # pass B, 355.4 per element (parent: 3124)
    "_Z18fp_fft_tile_1024x4I8Fp128OpsLb0ELb1EEv8TilePlanPK5elt_tjS4_j": 3302,  # pass A, one-tile launch (parent: 3652)
    "_Z26fp_fft_tile_1024x4_persistI8Fp128OpsEv8TilePlanPK5elt_tjS4_jj": 3332,  # pass A, XCD-aware order (parent: 3685)
}


def test_tile_kernels_redc_isa():
    for k, pinned in KERNELS.items():
        fft_isa.assert_no_scratch_within_128_vgprs(k)
        valu = fft_isa.valu(k)
        print(k, "VALU", valu)
        assert valu <= pinned, (k, valu, pinned)
        fft_isa.assert_scc_clean(k)

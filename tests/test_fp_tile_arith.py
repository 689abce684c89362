"""The Fp128 arithmetic of K1's 1024 x 4 tile kernels (csrc/fp_tile_arith.h: fpt_mul, fpt_add, fpt_sub): its values against
Python integers and against fields.h's fp_mul / fp_add / fp_sub on the GPU, and the VALU instruction counts of the kernels
that use it, pinned from the gfx950 ISA so that later edits cannot raise them unnoticed."""
import os
import subprocess

import numpy as np
import pytest

import fft_isa
from fft_isa import FFT, ROOT, SCC_READ, SCC_WRITE, hipcc as _hipcc  # noqa: F401 (other test files import them from here)

CHECK = os.path.join(ROOT, "tests", "fp_tile_arith_check.hip")

P = 2**128 - 2**108 + 1
R_INV = pow(2**128, -1, P)
P_HI = 0xFFFFF00000000000
MONT_ONE = 2**128 % P
# the edge values of tests/test_fp128_tile_1024x4.py (0, 1, p - 1, 2^128 mod p, ...) and some with the top 20 bits set
EDGES = [0, 1, P - 1, MONT_ONE, ((P_HI - 1) << 64) | 0xFFFFFFFFFFFFFFFF, 1 << 108, P - 2, P_HI << 64, (P_HI << 64) - 1,
         P - MONT_ONE, (P - 1) >> 1, 2**127, 0xFFFFFFFF, 1 << 96, (1 << 96) - 1]

# VALU instructions in the body of each kernel (8 elements per thread and tile, fully unrolled: static = dynamic count)
KERNELS = {
    "_Z18fp_fft_tile_1024x4I8Fp128OpsLb1ELb0EEv8TilePlanPK5elt_tjS4_j": 3124,  # pass B, 390.5 per element (parent: 3559)
    "_Z18fp_fft_tile_1024x4I8Fp128OpsLb0ELb1EEv8TilePlanPK5elt_tjS4_j": 3652,  # pass A, one-tile launch (parent: 4161)
    "_Z26fp_fft_tile_1024x4_persistI8Fp128OpsEv8TilePlanPK5elt_tjS4_jj": 3685,  # pass A, XCD-aware order (parent: 4207)
}


def test_tile_kernels_valu_counts():
    for k, pinned in KERNELS.items():
        fft_isa.assert_no_scratch_within_128_vgprs(k)
        valu = fft_isa.valu(k)
        assert valu <= pinned, (k, valu, pinned)
        fft_isa.assert_scc_clean(k)


def _limbs(x):
    return [x & (2**64 - 1), x >> 64]


@pytest.mark.gpu
def test_tile_arith_values(tmp_path):
    exe = tmp_path / "fp_tile_arith_check"
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", str(exe), CHECK])
    rng = np.random.default_rng(20261016)
    pairs = [(a, b) for a in EDGES for b in EDGES]
    for _ in range(20000):
        a, b = (int.from_bytes(rng.bytes(16), "little") % P for _ in range(2))
        if rng.integers(4) == 0:  # top 20 bits set
            a = (a | (P_HI << 64)) % P
        pairs.append((a, b))
    pairs += [(a, MONT_ONE) for a, _ in pairs[:2000]]  # products with Montgomery 1: w^0
    arr = np.array([_limbs(a) + _limbs(b) for a, b in pairs], dtype=np.uint64)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    arr.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout), str(4 << 20)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(fout, dtype=np.uint64).reshape(len(pairs), 3, 2)
    for (a, b), g in zip(pairs, got):
        val = [int(g[i][0]) | (int(g[i][1]) << 64) for i in range(3)]
        assert val == [a * b * R_INV % P, (a + b) % P, (a - b) % P], (hex(a), hex(b), [hex(v) for v in val])

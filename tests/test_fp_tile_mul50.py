"""fpt_mul (csrc/fp_tile_arith.h) at 50 VALU instructions: column 1's first v_mad_u64_u32 reads {acc0.hi, 0} as its addend and
writes a fresh pair (no 64-bit move for column 0), column 2's first mad (a0 b2) has no capture (SCHEDULE_COL2 of
test_fp_tile_mul_carries.py, whose model this file runs on the structured pairs and on 10^5 random ones), and the reduction keeps U
and U >> 20 in the registers of t0..t3, which holds pass A at 71 VGPRs.

Without a GPU: the ISA of the seven 1024 x 4 tile kernels (VALU ceilings of the four _tws kernels, no v_mov_b64, no scratch).  On the
GPU: fpt_mul, fpt_sub and fpt_add_lazy on 2^20 operand sets against Python integers, with all lanes active and inside a divergent
branch (even lanes, lane 63, lanes 0-31: the lanes outside keep a sentinel, every lane stores a marker behind the branch), among them
waves in which every lane takes the routine's conditional +-p and waves in which none does; and the
transform at 2^20 x 2 rows and 2^13 x 4 rows, default and LFGPU_FP_LAZY=0, against the oracle.
"""
import os
import subprocess

import numpy as np
import pytest

import fft_isa
import test_fp128_lazy_fft as LF
from test_fp128_tile_isa_pins import PINS
from test_fp_tile_arith import EDGES, P, R_INV, ROOT, _hipcc
from test_fp_tile_lazy import T_EDGES, U_EDGES
from test_fp_tile_mul_carries import SCHEDULE_COL2, _structured_pairs, mul_model
from test_fp_tile_redc import redc_model

CHECK = os.path.join(ROOT, "tests", "fp_tile_lanes_check.hip")
T128 = 2**128
ARGS = "I8Fp128OpsLb%dEEv8TilePlanPK5elt_tjS4_j"
# VALU ceilings = the counts of the built code, 8 elements per thread: the counts built before this change (one below the pins of
# test_fp_tile_mul_carries.py in each kernel) less 2 for each of a thread's products, 33 in pass A and 41 in pass B: the 64-bit
# move of column 0 and the capture of a0 b2.  Pass B's allocator saves one more move.
KERNELS = {
    "_Z22fp_fft_tile_1024x4_tws" + ARGS % 0: 2616 - 2 * 33,  # 2550, 318.8 per element
    "_Z22fp_fft_tile_1024x4_tws" + ARGS % 1: 3078 - 2 * 41 - 1,  # 2995, 374.4 per element
    "_Z28fp_fft_tile_1024x4_tws_canon" + ARGS % 0: 2724 - 2 * 33,  # 2658
    "_Z28fp_fft_tile_1024x4_tws_canon" + ARGS % 1: 3142 - 2 * 41,  # 3060
}


# ------------------------------------------------------------------ ISA
def test_tws_kernels_valu_ceilings():
    assert list(KERNELS.values()) == [2550, 2995, 2658, 3060]
    for k, pinned in KERNELS.items():
        valu = fft_isa.valu(k)
        print(k, "VALU", valu)
        assert valu <= pinned, (k, valu, pinned)


# v_mov_b32 ceilings = the counts of the built code: one per column of a product, 6 (at most 7 per product: 231 and 287 with
# 33 and 41 products), the rest the butterflies' own moves; with no v_mov_b64 left this pins column 0's single move
MOVES = dict(zip(KERNELS, (228, 276, 228, 277)))


def test_tws_kernels_mov_ceilings():
    for k, pinned in MOVES.items():
        ops = fft_isa.kernel(k).ops
        mov32 = sum(op.startswith("v_mov_b32") for op in ops)
        print(k, "v_mov_b32", mov32)
        assert mov32 <= pinned, (k, mov32, pinned)
        assert not any(op.startswith(("v_mov_b64", "v_pk_mov_b32", "v_lshrrev_b64")) for op in ops), k


@pytest.mark.parametrize("name", PINS)
def test_tile_kernels_registers_and_moves(name):
    """all seven: no scratch, at most 128 VGPRs, no 64-bit move, no SCC reader of the compiler's behind an asm's SCC write"""
    fft_isa.assert_no_scratch_within_128_vgprs(name)
    fft_isa.assert_scc_clean(name)
    assert not any(op.startswith("v_mov_b64") for op in fft_isa.kernel(name).ops), name


# ------------------------------------------------------------------ the product's schedule
def test_mul_model_with_column_2_uncaptured():
    """what fpt_mul now does: MAD, MADW, MADC in column 2; T = a w exactly and no uncaptured mad wraps (the model raises)"""
    rng = np.random.default_rng(20261022)
    pairs = _structured_pairs()
    for _ in range(100000):
        raw = rng.bytes(32)
        pairs.append((int.from_bytes(raw[:16], "little"), int.from_bytes(raw[16:], "little") % P))
    for a, w in pairs:
        assert mul_model(a, w, SCHEDULE_COL2) == a * w, (hex(a), hex(w))


# ------------------------------------------------------------------ the three routines on the GPU
N_SETS = 1 << 20
N_STRUCT = 1 << 16
PATTERNS = ("all lanes", "even lanes", "lane 63", "lanes 0-31")
MARK = 0x5EED0000
# blocks of 128 consecutive operand sets (two waves of the check program, which start at multiples of 64) in which every lane /
# no lane takes the conditional +-p of one routine, behind the structured block
WAVE_KINDS = ("sub borrows", "sub does not borrow", "add carries", "add does not carry", "mul adds p", "mul does not add p")


def _fix_taken(kind, u, t):
    """from the integers: does fpt_sub(u, t) add p, fpt_add_lazy(u, t) subtract p, fpt_mul(u, t)'s reduction add p (W < 0)"""
    if kind.startswith("sub"):
        return u < t
    if kind.startswith("add"):
        return u + t >= T128
    return "+p taken" in redc_model(u * t)[1]


def _rand_sets(rng, n):
    """u uniform, every second one in [p, 2^128) (the top 20 bits set and the lowest one); t < p"""
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, P >> 64, size=n, dtype=np.uint64)
    a[1::2, 1] = (a[1::2, 1] >> np.uint64(20)) | np.uint64(P >> 64)
    a[1::2, 0] |= np.uint64(1)
    return a


def _ints(a):
    """(n, 2) uint64 limbs -> Python integers"""
    return [l | (h << 64) for l, h in zip(a[:, 0].tolist(), a[:, 1].tolist())]


def _limbs(xs):
    """Python integers < 2^128 -> (n, 2) uint64 limbs"""
    return np.frombuffer(b"".join(x.to_bytes(16, "little") for x in xs), dtype=np.uint64).reshape(-1, 2)


@pytest.fixture(scope="module")
def operands():
    """(the 2^20 operand sets as (n, 4) uint64, the reference (n, 3, 2): fpt_mul, fpt_sub, fpt_add_lazy), computed once"""
    rng = np.random.default_rng(20261023)
    pairs = _structured_pairs() + [(u, t) for u in U_EDGES for t in T_EDGES + EDGES]
    assert len(pairs) % 2 == 1  # odd: tiled, every lane position of a wave meets every pair
    st = np.concatenate([_limbs([a for a, _ in pairs]), _limbs([w for _, w in pairs])], axis=1)
    st = np.tile(st, (-(-N_STRUCT // len(st)), 1))[:N_STRUCT]
    cand = _rand_sets(rng, 4096)
    cu, ct = _ints(cand[:, 0:2]), _ints(cand[:, 2:4])
    blocks = []
    for kind in WAVE_KINDS:
        rows = [i for i in range(len(cand)) if _fix_taken(kind, cu[i], ct[i]) == ("not" not in kind)][:128]
        assert len(rows) == 128, kind
        blocks.append(cand[rows])
    arr = np.concatenate([st] + blocks + [_rand_sets(rng, N_SETS - N_STRUCT - 128 * len(WAVE_KINDS))])
    assert arr.shape == (N_SETS, 4)
    us, ts = _ints(arr[:, 0:2]), _ints(arr[:, 2:4])
    assert sum(u >= P for u in us) >= N_SETS // 4 and all(t < P for t in ts)
    # both outcomes of each conditional +-p are common: the borrow of u - t, the carry of u + t
    assert min(sum(u < t for u, t in zip(us, ts)), sum(u >= t for u, t in zip(us, ts))) >= N_SETS // 8
    assert min(sum(u + t >= T128 for u, t in zip(us, ts)), sum(u + t < T128 for u, t in zip(us, ts))) >= N_SETS // 8
    ref = np.stack([_limbs([u * t * R_INV % P for u, t in zip(us, ts)]), _limbs([u - t if u >= t else u - t + P for u, t in zip(us, ts)]),
                    _limbs([u + t if u + t < T128 else u + t - P for u, t in zip(us, ts)])], axis=1)
    # from the reference: for each routine, two whole waves in which all 64 lanes take the fix and two in which none does
    for k, kind in enumerate(WAVE_KINDS):
        for lo in (N_STRUCT + 128 * k, N_STRUCT + 128 * k + 64):
            assert lo % 64 == 0
            taken = [_fix_taken(kind, us[i], ts[i]) for i in range(lo, lo + 64)]
            assert not any(taken) if "not" in kind else all(taken), (kind, lo)
            r = 1 if kind.startswith("sub") else 2
            if r == 1 or kind.startswith("add"):  # the fix shows in the stored value: u - t + p, u + t - p
                exact = [us[i] - ts[i] + P * taken[i - lo] if r == 1 else us[i] + ts[i] - P * taken[i - lo] for i in range(lo, lo + 64)]
                assert _ints(ref[lo:lo + 64, r]) == exact, (kind, lo)
    arr.setflags(write=False)
    ref.setflags(write=False)
    return arr, ref


def run_check(exe, arr, tmp_path):
    """the check program's output: (4 patterns, n, 3, 2) results and (4, n) markers"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    arr.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    n = len(arr)
    raw = np.fromfile(fout, dtype=np.uint8)
    assert len(raw) == 4 * n * 48 + 4 * n * 4
    return raw[:4 * n * 48].view(np.uint64).reshape(4, n, 3, 2), raw[4 * n * 48:].view(np.uint32).reshape(4, n)


def compare(got, marks, ref):
    """active lanes equal the reference, the others' slots still hold the sentinel, and every lane stored its marker"""
    n = len(ref)
    lane = np.arange(n) & 63
    active = (np.ones(n, bool), lane % 2 == 0, lane == 63, lane < 32)
    for p, name in enumerate(PATTERNS):
        on = active[p]
        bad = np.flatnonzero((got[p][on] != ref[on]).any(axis=(1, 2)))
        assert not len(bad), (name, len(bad), np.flatnonzero(on)[bad[:4]], got[p][on][bad[:4]], ref[on][bad[:4]])
        assert (got[p][~on] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), name
        assert (marks[p] == (np.arange(n, dtype=np.uint32) ^ np.uint32(MARK))).all(), name


@pytest.mark.gpu
def test_arith_all_lanes_and_divergent_device(operands, tmp_path):
    exe = tmp_path / "fp_tile_lanes_check"
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", str(exe), CHECK])
    arr, ref = operands
    got, marks = run_check(exe, arr, tmp_path)
    compare(got, marks, ref)


# ------------------------------------------------------------------ the transform
N20, N13 = 1 << 20, 1 << 13
# (name, logn, rows, ld, direction), as fp_tile_child.py reads the key
FFT_CASES = [("mul50", 20, 2, N20, d) for d in "bf"] + [("mul50", 13, 4, N13, d) for d in "bf"]


def _flood13(rng, swap):
    """a 2^13 row of the kind of test_fp128_lazy_fft.py's lo / hi: one half p - 1, the other uniform in [1, 2^108 - 2]"""
    a = np.empty((N13, 2), dtype=np.uint64)
    a[:] = [0, LF.P_HI]
    u = LF._small(rng, (N13 // 2,), 108)
    u[:, 0] = np.clip(u[:, 0], np.uint64(1), np.uint64(2**64 - 2))
    if swap:
        a[:N13 // 2] = u
    else:
        a[N13 // 2:] = u
    return a


@pytest.fixture(scope="module")
def fft_runs(tmp_path_factory):
    """(inputs, the default path's outputs, LFGPU_FP_LAZY=0's outputs, the oracle's)"""
    rng = np.random.default_rng(20261024)
    cases = {}
    for case in FFT_CASES:
        _, logn, rows, ld, d = case
        if logn == 20:  # a random row, and one that floods pass A with sums in [p, 2^128)
            a = np.stack([LF._rnd(rng, N20), LF._structured("lo", d)])
        else:
            a = np.stack([LF._rnd(rng, N13), _flood13(rng, False), _flood13(rng, True), LF._rnd(rng, N13, 1)])
        cases[LF._key(case)] = a
    tmp = tmp_path_factory.mktemp("mul50_fft")
    cin = str(tmp / "cases.npz")
    np.savez(cin, **cases)
    lazy, canon = LF._child(None, cin, str(tmp / "lazy.npz")), LF._child("0", cin, str(tmp / "canon.npz"))
    want = {}
    for case in FFT_CASES:
        k = LF._key(case)
        want[k] = cases[k].copy()
        LF._fft(want[k], 1 << case[1], case[4])
    return cases, lazy, canon, want


@pytest.mark.gpu
@pytest.mark.parametrize("case", FFT_CASES, ids=LF._key)
def test_transform_matches_oracle(fft_runs, case):
    """n = 2^20 reaches the _tws pair, n = 2^13 fp_fft_tile_1024x4's pass B; both paths byte-identical to the CPU oracle"""
    _, lazy, canon, want = fft_runs
    k = LF._key(case)
    assert lazy[k].tobytes() == want[k].tobytes()
    assert canon[k].tobytes() == want[k].tobytes()

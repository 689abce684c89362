"""The paired routines of csrc/fp_tile_arith.h (fpt_mul2_t<false>, fpt_mul2_t<true> with wave-uniform twiddles, fpt_bfly2_lazy, its
single form fpt_bfly_lazy, fpt_canon2) on the GPU, on 2^20 operand sets (up, tp, uq, tq) against Python integers and, in the same
lanes, against the single routines: all lanes active for every set, and inside a divergent branch (even lanes, lane 63, lanes
0-31) for the first 2^17, which hold the structured sets and the built waves.  The lanes outside a pattern keep a sentinel and every
lane stores a marker behind the branch.

The carries of the paired routines live in SGPR pairs, which are lane masks under a partial EXEC, and each product or butterfly
of a pair has masks of its own.  So the two halves of a set are drawn independently (one's carries cannot stand in for the
other's), and for each conditional +-p (the borrow of u - t, the carry of u + t, W < 0 in the product's reduction, u >= p in
canon) there are waves in which every lane, no lane and every second lane takes it, for p and for q in all nine combinations.  The
sets of such a wave share tp and tq, so that fpt_mul2_t<true>, whose twiddles are the wave's first set's, meets the same masks."""
import os
import subprocess

import numpy as np
import pytest

from test_fp_tile_arith import EDGES, P, R_INV, ROOT, _hipcc
from test_fp_tile_lazy import T_EDGES, U_EDGES
from test_fp_tile_mul50 import MARK, PATTERNS, _ints, _limbs
from test_fp_tile_mul_carries import _structured_pairs
from test_fp_tile_redc import redc_model

CHECK = os.path.join(ROOT, "tests", "fp_tile_pair_check.hip")
T128 = 2**128
N_SETS, N_STRUCT, N_DIV = 1 << 20, 1 << 16, 1 << 17
KINDS = ("sub", "add", "mul", "canon")
MODES = ("all", "none", "alternating")
N_WAVES = len(KINDS) * len(MODES) ** 2
RES = 13  # values per record of the check program: 12 results and the word of flags
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


def taken(kind, u, t):
    """from the integers: does fpt_sub(u, t) add p, fpt_add_lazy(u, t) subtract p, fpt_mul(u, t)'s reduction add p, fpt_canon(u) subtract p"""
    if kind == "sub":
        return u < t
    if kind == "add":
        return u + t >= T128
    if kind == "mul":
        return "+p taken" in redc_model(u * t)[1]
    return u >= P


def _wanted(mode, lane):
    return mode == "all" or (mode == "alternating" and lane % 2 == 0)


def _rand_u(rng):
    """uniform in [0, 2^128), or with the top 20 bits set (>= p - 1), or within 2^64 of 0 or of 2^128: every outcome can be met for any t"""
    u, how = int.from_bytes(rng.bytes(16), "little"), rng.integers(4)
    return u if how == 0 else u | (P - 1) if how == 1 else u >> 64 if how == 2 else T128 - 1 - (u >> 64)


def _rand_sets(rng, n):
    """n independent (u, t): u uniform, every second one in [p, 2^128) (the top 20 bits and the lowest one set); t < p"""
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, P >> 64, size=n, dtype=np.uint64)
    a[1::2, 1] = (a[1::2, 1] >> np.uint64(20)) | np.uint64(P >> 64)
    a[1::2, 0] |= np.uint64(1)
    return a


def _built_waves(rng):
    """(N_WAVES * 64, 8) uint64 and the (kind, p's mode, q's mode) of each wave"""
    sets, what = [], []
    for kind in KINDS:
        for mp in MODES:
            for mq in MODES:
                tp, tq = (int.from_bytes(rng.bytes(16), "little") % P for _ in range(2))
                for lane in range(64):
                    row = []
                    for t, mode in ((tp, mp), (tq, mq)):
                        u = _rand_u(rng)
                        while taken(kind, u, t) != _wanted(mode, lane):
                            u = _rand_u(rng)
                        row += [u, t]
                    sets.append(row)
                what.append((kind, mp, mq))
    return np.concatenate([_limbs([r[k] for r in sets]) for k in range(4)], axis=1), what


@pytest.fixture(scope="module")
def operands():
    """(the 2^20 operand sets as (n, 8) uint64, the reference (n, 12, 2), the built waves' descriptions), computed once"""
    rng = np.random.default_rng(20261025)
    pairs = _structured_pairs() + [(u, t) for u in U_EDGES for t in T_EDGES + EDGES]
    assert len(pairs) % 2 == 1  # odd: tiled, every lane position of a wave meets every pair as p's
    half = np.concatenate([_limbs([a for a, _ in pairs]), _limbs([w for _, w in pairs])], axis=1)
    st = np.concatenate([np.tile(half, (-(-N_STRUCT // len(half)), 1))[:N_STRUCT], half[rng.integers(0, len(half), N_STRUCT)]], axis=1)
    waves, what = _built_waves(rng)
    n_rand = N_SETS - N_STRUCT - len(waves)
    arr = np.concatenate([st, waves, np.concatenate([_rand_sets(rng, n_rand), _rand_sets(rng, n_rand)], axis=1)])
    assert arr.shape == (N_SETS, 8) and N_STRUCT % 64 == 0 and N_STRUCT + len(waves) <= N_DIV
    up, tp, uq, tq = (_ints(arr[:, 2 * k:2 * k + 2]) for k in range(4))
    assert all(t < P for t in tp) and all(t < P for t in tq)
    wp, wq = ([t[i & ~63] for i in range(N_SETS)] for t in (tp, tq))  # fpt_mul2_t<true>: the wave's first set's

    def mul(us, ts):
        return _limbs([u * t * R_INV % P for u, t in zip(us, ts)])

    def add(us, ts):
        return _limbs([u + t if u + t < T128 else u + t - P for u, t in zip(us, ts)])

    def sub(us, ts):
        return _limbs([u - t if u >= t else u - t + P for u, t in zip(us, ts)])

    def canon(us):
        return _limbs([u - P if u >= P else u for u in us])

    xp, yp = add(up, tp), sub(up, tp)
    ref = np.stack([mul(up, tp), mul(uq, tq), mul(up, wp), mul(uq, wq), xp, yp, add(uq, tq), sub(uq, tq), xp, yp, canon(up), canon(uq)], axis=1)
    # the built waves are what they are meant to be, from the integers; their twiddles are uniform
    for w, (kind, mp, mq) in enumerate(what):
        lo = N_STRUCT + 64 * w
        for us, ts, mode in ((up, tp, mp), (uq, tq, mq)):
            assert len(set(ts[lo:lo + 64])) == 1
            assert [taken(kind, us[i], ts[i]) for i in range(lo, lo + 64)] == [_wanted(mode, lane) for lane in range(64)], (kind, mp, mq)
    assert len(what) == N_WAVES
    arr.setflags(write=False)
    ref.setflags(write=False)
    return arr, ref


def run_check(exe, arr, tmp_path):
    """the check program's output: per pattern the (m, RES, 2) records and the (m,) markers, m = n for all lanes and N_DIV otherwise"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    arr.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout), str(N_DIV)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    sizes = [len(arr)] + [N_DIV] * (len(PATTERNS) - 1)
    raw = np.fromfile(fout, dtype=np.uint8)
    assert len(raw) == sum(sizes) * (RES * 16 + 4)
    recs, marks, at = [], [], 0
    for m in sizes:
        recs.append(raw[at:at + m * RES * 16].view(np.uint64).reshape(m, RES, 2))
        at += m * RES * 16
    for m in sizes:
        marks.append(raw[at:at + 4 * m].view(np.uint32))
        at += 4 * m
    return recs, marks


def compare(recs, marks, ref):
    """active lanes equal the integers and the single routines, the others' records still hold the sentinel, every lane stored its marker"""
    for p, name in enumerate(PATTERNS):
        m = len(recs[p])
        lane = np.arange(m) & 63
        on = (np.ones(m, bool), lane % 2 == 0, lane == 63, lane < 32)[p]
        got = recs[p][on]
        bad = np.flatnonzero((got[:, :12] != ref[:m][on]).any(axis=(1, 2)))
        assert not len(bad), (name, len(bad), np.flatnonzero(on)[bad[:4]], got[bad[:4], :12], ref[:m][on][bad[:4]])
        flags = np.uint64(MARK << 32)  # no bit set: every paired result equals the single routine's
        assert (got[:, 12, 0] == flags).all() and (got[:, 12, 1] == np.uint64(MARK << 32 | MARK)).all(), name
        assert (recs[p][~on] == SENTINEL).all(), name
        assert (marks[p] == (np.arange(m, dtype=np.uint32) ^ np.uint32(MARK))).all(), name


@pytest.mark.gpu
def test_paired_arith_all_lanes_and_divergent_device(operands, tmp_path):
    exe = tmp_path / "fp_tile_pair_check"
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", str(exe), CHECK])
    arr, ref = operands
    recs, marks = run_check(exe, arr, tmp_path)
    compare(recs, marks, ref)


def test_reference_of_the_paired_check(operands):
    """without a GPU: the operand sets hold both outcomes of every conditional +-p often, in p's half and in q's"""
    arr, _ = operands
    for k in (0, 2):
        us, ts = _ints(arr[:, 2 * k:2 * k + 2]), _ints(arr[:, 2 * k + 2:2 * k + 4])
        assert sum(u >= P for u in us) >= N_SETS // 4
        for yes in (sum(u < t for u, t in zip(us, ts)), sum(u + t >= T128 for u, t in zip(us, ts))):
            assert min(yes, N_SETS - yes) >= N_SETS // 8

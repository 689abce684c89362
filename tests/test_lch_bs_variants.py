"""Every A/B setting of the bit-sliced GF(2^128) path (csrc/lch_bs.hip: K2's tower kernels, and the big-row Reed-Solomon
encoder of csrc/rs.hip that works in the same representation) must produce the oracle's bytes in EVERY row.  The switches are
read once per process, so each setting runs in a child process of its own (tests/lch_bs_child.py) on the same inputs; the
expectation is computed once, on the CPU, for all of them.

Where each setting sends the shapes below (bs_geom, bs_passes, lf_bs_tower_op, gf_rs_rows_big):
  * a batch has ceil(rows / 32) * D (row group, coordinate) combos, D = 8 for GF2_128<4> and 4 for <5>.  With >= 64 of them
    the butterflies run in bs_bfly2_kernel (register-resident), in groups of <= 4 index bits with NW = 2^(bits - 1) waves, or
    <= 5 bits with LFGPU_BS_V2_NB=5 (a 5-bit group: NW = 16, the 1024-thread workgroup); LFGPU_BS_NW_MATCH=0 launches every
    group of < 4 bits with NW = 8 (idle waves).  With fewer combos, or with LFGPU_BS_V2=0, they run in bs_bfly_kernel (LDS
    tile of 2^r_log lanes per column pair), in groups of <= 9 - r_log bits: 4, or 3 / 2 with LFGPU_BS_RLOG=6 / 7.
  * LFGPU_BS_CU is the number of inner column bits of a tile, clamped per group to min(CU, lo_bit, r_log): 0 keeps none
    anywhere, 5 takes 0 / 4 / 5 / 5 in the groups of a 4-bit plan where the default takes 0 / 3 / 3 / 3.
  * LFGPU_BS_CIN_WPC / LFGPU_BS_COUT_WPC pick the conversion kernels' instantiation <K, 2 | 3 | 4> (default 2 for K = 4, 4
    for K = 5).
  * LFGPU_LCH_BS=0 sends the FFT to the LDS-tile plan lch_fft_tile (one tile for l <= 12, two passes at l = 13);
    LFGPU_RS_TOWER=0 makes the big-row encoder convert per block: lfgpu_gf2128_lch14_fft on sub-blocks with ld = 2^l.

A child that faults, aborts or hangs is recorded; every later child test of the module then fails without starting a
process."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "lch_bs_child.py")
CHILD_TIMEOUT = 180  # seconds, one child: interpreter + runtime start-up, ~0.5 GB of .npz traffic, a few dozen launches

# (k, l, coset, rows), each in both directions.  Butterfly groups (index bits, from bit 0 up) at 4 / 5 bits per pass:
FFT_CASES = [
    (4, 7, 1 << 7, 250),     # 4+3 / 5+2; 64 combos, ragged last row group (26 rows)
    (4, 9, 0, 270),          # 4,4,1 / 5,4; 72 combos padded to 128: the memset of the padding, a second grid.y tile
    (4, 10, 3 << 10, 250),   # 4,4,2 / 5,5
    (5, 11, 0, 490),         # 4,4,3 / 5,5,1; K = 5, 64 combos, the last row group has 10 rows
    (4, 13, 1 << 13, 250),   # 4,4,4,1 / 5,5,3
    (5, 8, 0, 40),           # 8 combos: bs_bfly_kernel by default; groups 4,4 / 3,3,2 / 2,2,2,2 at r_log 5 / 6 / 7
    (4, 12, 1 << 12, 33),    # 16 combos: bs_bfly_kernel by default; groups 4,4,4 / 3,3,3,3 / 2 x 6
]
# (k, n, m, nrow): rows larger than LDS (l = 13)
RS_CASES = [
    (4, 4100, 8292, 250),    # 64 combos, one partial further coset (100 columns)
    (5, 4100, 8292, 490),    # K = 5, likewise
    (5, 4100, 8192, 70),     # 12 combos (bs_bfly_kernel), m = 2^l: no further coset
]

# (environment, key prefix of the cases the child runs; "" = all)
SETTINGS = [
    ({}, ""),
    ({"LFGPU_LCH_BS": "0"}, "fft_"),
    ({"LFGPU_RS_TOWER": "0"}, "rs_"),
    ({"LFGPU_BS_V2": "0"}, ""),
    ({"LFGPU_BS_V2_NB": "5"}, ""),
    ({"LFGPU_BS_NW_MATCH": "0"}, ""),
    ({"LFGPU_BS_V2": "0", "LFGPU_BS_RLOG": "6"}, ""),
    ({"LFGPU_BS_V2": "0", "LFGPU_BS_RLOG": "7"}, ""),
    ({"LFGPU_BS_CU": "0"}, ""),
    ({"LFGPU_BS_CU": "5"}, ""),
    # the defaults are 2 (K = 4) and 4 (K = 5): none of the three equals the default for both K
    ({"LFGPU_BS_CIN_WPC": "2", "LFGPU_BS_COUT_WPC": "2"}, ""),
    ({"LFGPU_BS_CIN_WPC": "3", "LFGPU_BS_COUT_WPC": "3"}, ""),
    ({"LFGPU_BS_CIN_WPC": "4", "LFGPU_BS_COUT_WPC": "4"}, ""),
]


def _setting_id(s):
    return " ".join("%s=%s" % kv for kv in s[0].items()) or "default"


def inputs():
    """key -> rows x ld x 2 uint64, seeded; ld = 2^l + 5 (FFT) / m + 3 (RS), so every row has a tail that must stay"""
    rng = np.random.default_rng(20261018)
    cases = {}
    for k, l, coset, rows in FFT_CASES:
        ld = (1 << l) + 5
        for d in "fi":
            cases["fft_%d_%d_%d_%d_%s" % (k, l, coset, rows, d)] = ol.rand_elts(rng, rows * ld).reshape(rows, ld, 2)
    for k, n, m, nrow in RS_CASES:
        ld = m + 3
        cases["rs_%d_%d_%d_%d" % (k, n, m, nrow)] = ol.rand_elts(rng, nrow * ld).reshape(nrow, ld, 2)
    return cases


def expected(cases):
    """the oracle on every row of every case; the columns beyond the transform are the input's"""
    o = ol.oracle()
    want = {}
    for key, a in cases.items():
        f = key.split("_")
        w = a.copy()
        if f[0] == "fft":
            k, l, coset, rows = (int(x) for x in f[1:5])
            fn = o.lfo_lch14_ifft if f[5] == "i" else o.lfo_lch14_fft
            for r in range(rows):
                row = np.ascontiguousarray(w[r, :1 << l])
                fn(C.byref(ol.gf_ctx(k)), l, coset, P(row))
                w[r, :1 << l] = row
        else:
            k, n, m, nrow = (int(x) for x in f[1:5])
            for r in range(nrow):
                row = np.ascontiguousarray(w[r, :m])
                o.lfo_lch14_rs_interpolate(C.byref(ol.gf_ctx(k)), n, m, P(row))
                w[r, :m] = row
        want[key] = w
    return want


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    d = tmp_path_factory.mktemp("lch_bs")
    cases = inputs()
    cin = str(d / "cases.npz")
    np.savez(cin, **cases)
    t0 = time.process_time()
    want = expected(cases)
    print("oracle fixture: %.1f s CPU, %.0f MB of cases" % (time.process_time() - t0, sum(a.nbytes for a in cases.values()) / 1e6))
    return d, cin, want


_FAULT = []  # the first child that faulted, aborted or hung: nothing more is started on the GPU after it
_FAULT_CODES = (134, 139, 124, 137)  # abort, segmentation fault, time limit (and their negative forms from subprocess)
_FAULT_TEXT = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR")


def _run_child(name, env_extra, prefix, cin, cout):
    if _FAULT:
        pytest.fail("not started: an earlier child faulted or hung (%s)" % _FAULT[0], pytrace=False)
    env = dict(os.environ)
    for k in list(env):
        if k == "LFGPU_LCH_BS" or k.startswith("LFGPU_RS_") or k.startswith("LFGPU_BS_"):
            del env[k]
    env.update(env_extra)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, CHILD, cin, cout, prefix], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:  # subprocess.run has killed and reaped the child
        _FAULT.append("%s: no result after %d s" % (name, CHILD_TIMEOUT))
        pytest.fail(_FAULT[0], pytrace=False)
    print("child %s: %.1f s" % (name, time.time() - t0))
    if r.returncode < 0 or r.returncode in _FAULT_CODES or any(t in r.stderr for t in _FAULT_TEXT):
        _FAULT.append("%s: exit status %d: %s" % (name, r.returncode, r.stderr[-1500:]))
        pytest.fail(_FAULT[0], pytrace=False)
    assert r.returncode == 0 and "OK" in r.stdout, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return np.load(cout)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", SETTINGS, ids=_setting_id)
def test_every_row_under_setting(golden, setting):
    """one child under `setting`; every byte of every case (all rows, all columns up to ld) is the oracle's"""
    d, cin, want = golden
    env_extra, prefix = setting
    name = _setting_id(setting)
    cout = str(d / "out.npz")
    if os.path.exists(cout):
        os.remove(cout)
    got = _run_child(name, env_extra, prefix, cin, cout)
    keys = [k for k in want if k.startswith(prefix)]
    assert sorted(got.files) == sorted(keys), (name, got.files)
    for key in keys:
        g, w = got[key], want[key]
        assert g.shape == w.shape and g.dtype == w.dtype, (name, key, g.shape, g.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere((g != w).any(axis=-1))
            rows_bad = np.unique(bad[:, 0])
            pytest.fail("%s: case %s differs from the oracle first at row %d, column %d (of ld = %d); %d elements in %d rows differ"
                        % (name, key, bad[0][0], bad[0][1], w.shape[1], len(bad), len(rows_bad)), pytrace=False)

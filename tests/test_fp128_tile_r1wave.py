"""K1 at n = 2^20 with a wave-uniform round 1 (csrc/fft.hip, fp_fft_tile_1024x4_tw2): the ISA of the two kernels next to the pair
they replace as the default (fp_fft_tile_1024x4_tws), and the default launches next to LFGPU_FP_R1WAVE=0, LFGPU_FP_LAZY=0 and
the oracle.  The switches are read once per process, so each setting runs in a child process (tests/fp_tile_child.py).

Round 1 of these kernels branches on the wave's twiddle index j (uniform), so a thread runs one of two paths and the static
instruction count of a path is the kernel's minus the other path's round 1; the kernels mark the two with asm comments."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fft_isa
from test_fp128_lazy_fft import PAD, _fft, _rnd, _structured
from test_fp128_twside import ROOT

CHILD = os.path.join(ROOT, "tests", "fp_tile_child.py")
ARGS = "I8Fp128OpsLb%dEEv8TilePlanPK5elt_tjS4_j"
NEW = "_Z22fp_fft_tile_1024x4_tw2" + ARGS
OLD = "_Z22fp_fft_tile_1024x4_tws" + ARGS
# pass (0 = A, 1 = B): VALU of fp_fft_tile_1024x4_tws, VGPR ceiling (its VGPRs), global loads, and the VALU ceilings of the two paths
# = the counts of the built code.  Per thread of 8 elements: the j > 0 path has round 0's three and round 1's seven twiddles as
# scalar operands (no moves into VGPRs, no LDS twiddle reads in round 1) and pays for the layout's slot arithmetic; the j = 0 path
# has 5 products of 50 and 7 fpt_canon of 8 where the other has 12 products.
PARENT_VALU = {0: 2550, 1: 2995}
VGPRS = {0: 71, 1: 86}
LOADS = {0: 9, 1: 17}
PATH_VALU = {0: {"j > 0": 2536, "j = 0": 2244}, 1: {"j > 0": 2983, "j = 0": 2691}}
PRODUCT_SAVING = 7 * 50 / 8  # 7 of the 12 products of round 1 in one wave of eight, 0.875 products per thread on average


def _region(lines, tag):
    """the instructions' opcodes between the asm comments '; round 1, <tag>' and '; round 1, <tag>: stored'"""
    a, b = lines.index("; round 1, " + tag), lines.index("; round 1, " + tag + ": stored")
    assert a < b
    return [l.split()[0] for l in lines[a:b] if fft_isa._is_instruction(l)]


def _paths(pass_b):
    """path -> (VALU instructions, LDS reads) of a thread on that path"""
    k = fft_isa.kernel(NEW % pass_b)
    total = sum(op.startswith("v_") for op in k.ops), sum(op.startswith("ds_read") for op in k.ops)
    out = {}
    for tag, other in (("j > 0", "j = 0"), ("j = 0", "j > 0")):
        ops = _region(k.lines, other)
        out[tag] = total[0] - sum(op.startswith("v_") for op in ops), total[1] - sum(op.startswith("ds_read") for op in ops)
    return out


@pytest.mark.parametrize("pass_b", [0, 1])
def test_r1wave_kernels_isa(pass_b):
    name, old = NEW % pass_b, OLD % pass_b
    k = fft_isa.kernel(name)
    assert k.desc["private_segment_fixed_size"] == 0
    assert not any(op.startswith(("scratch_", "buffer_", "flat_")) for op in k.ops)
    print(name, "VGPRs", k.desc["next_free_vgpr"])
    assert k.desc["next_free_vgpr"] <= VGPRS[pass_b]
    fft_isa.assert_global_loads(name, LOADS[pass_b])
    assert fft_isa.dwordx4_loads_before_first_vmcnt_wait(name) >= LOADS[pass_b]
    fft_isa.assert_scc_clean(name)
    assert fft_isa.valu(old) == PARENT_VALU[pass_b]  # the figure the savings are counted from
    paths = _paths(pass_b)
    print(name, paths)
    for tag, (valu, _) in paths.items():
        assert valu <= PATH_VALU[pass_b][tag], (tag, valu)
        assert valu < PARENT_VALU[pass_b]
    mean = (7 * paths["j > 0"][0] + paths["j = 0"][0]) / 8
    assert mean <= PARENT_VALU[pass_b] - PRODUCT_SAVING, mean
    old_reads = sum(op.startswith("ds_read") for op in fft_isa.kernel(old).ops)
    assert paths["j > 0"][1] == paths["j = 0"][1] == old_reads - 7  # round 1's seven twiddles come from scalar loads


@pytest.mark.parametrize("pass_b", [0, 1])
def test_r1wave_twiddles_are_scalar_operands(pass_b):
    """round 1 reads no twiddle from LDS and every product there takes a limb of its twiddle from an SGPR; the ten scalar
    twiddle loads (seven of round 1, three of round 0) are issued before the first wait on vector memory"""
    k = fft_isa.kernel(NEW % pass_b)
    for tag, products in (("j > 0", 12), ("j = 0", 5)):
        a, b = k.lines.index("; round 1, " + tag), k.lines.index("; round 1, " + tag + ": stored")
        body = [l for l in k.lines[a:b] if fft_isa._is_instruction(l)]
        assert sum(l.startswith("ds_read_b128") for l in body) == 8 and sum(l.startswith("ds_write_b128") for l in body) == 8
        mads = [l for l in body if l.startswith("v_mad_u64_u32")]
        assert len(mads) == 16 * products
        assert all(any(o.strip().startswith("s") for o in l.split(None, 1)[1].split(",")[2:4]) for l in mads), tag
    first_wait = next(i for i, l in enumerate(k.lines) if l.startswith("s_waitcnt") and "vmcnt" in l)
    assert sum(l.startswith("s_load_dwordx4") for l in k.lines[:first_wait]) >= 10


# ------------------------------------------------------------------ on the GPU
N = 1 << 20
# (name, logn, rows, ld, direction): the smallest shapes that reach the pair.  mix: a random row with the edge values and a row
# built to make non-canonical intermediates (lo / fin of test_fp128_lazy_fft.py), both ways; pad: ld > n; n = 2^21: the inner transforms
CASES = [("mix", 20, 2, N, "b"), ("mix", 20, 2, N, "f"), ("pad", 20, 2, N + 64, "f"), ("rnd", 21, 1, 1 << 21, "b")]
SETTINGS = {"default": {}, "r1wave0": {"LFGPU_FP_R1WAVE": "0"}, "lazy0": {"LFGPU_FP_LAZY": "0"}}


def _key(case):
    return "%s_%d_%d_%d_%s" % case


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(20261022)
    cases = {}
    for case in CASES:
        name, logn, rows, ld, d = case
        n = 1 << logn
        a = np.empty((rows, ld, 2), dtype=np.uint64)
        a[:, n:] = PAD  # beyond the row: must stay as it is
        a[0, :n] = _rnd(rng, n)
        if name == "mix":
            a[1, :n] = _structured("lo" if d == "b" else "fin", d)
        elif name == "pad":
            a[1, :n] = _structured("hi", d)
        cases[_key(case)] = a
    return cases


@functools.lru_cache(maxsize=None)
def _want():
    """the oracle's transforms, computed once"""
    want = {}
    for case in CASES:
        _, logn, _, _, d = case
        w = _inputs()[_key(case)].copy()
        rows = np.ascontiguousarray(w[:, :1 << logn])
        _fft(rows, 1 << logn, d)
        w[:, :1 << logn] = rows
        want[_key(case)] = w
    return want


def _child(setting, cin, cout):
    env = dict(os.environ)
    for v in ("LFGPU_FP_R1WAVE", "LFGPU_FP_LAZY", "LFGPU_FP_TWSIDE", "LFGPU_FP_PERSIST", "LFGPU_FP_TILE1024", "LFGPU_FP_TW", "LFGPU_FP_ROWFAST",
              "LFGPU_TILE_LOG"):
        env.pop(v, None)
    env.update(setting)
    r = subprocess.run([sys.executable, CHILD, cin, cout], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(cout)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("r1wave")
    cin = str(d / "cases.npz")
    np.savez(cin, **_inputs())
    return {name: _child(env, cin, str(d / (name + ".npz"))) for name, env in SETTINGS.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_key)
def test_r1wave_matches_other_kernels_and_oracle(runs, case):
    """the default, LFGPU_FP_R1WAVE=0 and LFGPU_FP_LAZY=0 byte-identical and equal to the oracle's fftb / fftf; row padding untouched"""
    k = _key(case)
    got = runs["default"][k]
    for other in ("r1wave0", "lazy0"):
        assert got.tobytes() == runs[other][k].tobytes(), other
    assert (got == _want()[k]).all()

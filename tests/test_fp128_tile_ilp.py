"""K1 at n = 2^20 with the tile arithmetic issued in pairs (csrc/fft.hip, fp_fft_tile_1024x4_tw2<T4Ilp<Fp128Ops>, ..>, the default;
csrc/fp_tile_arith.h, fpt_mul2_t, fpt_bfly2_lazy, fpt_bfly_lazy, fpt_canon2): the ISA of the two kernels next to
fp_fft_tile_1024x4_tw2<Fp128Ops, ..>, which LFGPU_FP_ILP=0 launches, from the same build; a lint of the one hazard rule the
hand-interleaved asm can break without any model noticing; and the default launches next to LFGPU_FP_ILP=0, LFGPU_FP_R1WAVE=0,
LFGPU_FP_LAZY=0 and the oracle, each setting in a child process (tests/fp_tile_child.py).

A thread runs one of the two round-1 paths (j > 0, j = 0: the kernels mark them with asm comments), so a path's static count is
the kernel's minus the other path's round 1, as in test_fp128_tile_r1wave.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fft_isa
from test_fp128_tile_r1wave import CASES, CHILD, LOADS, PATH_VALU, _inputs, _key, _want

TW2 = "_Z22fp_fft_tile_1024x4_tw2I8Fp128OpsLb%dEEv8TilePlanPK5elt_tjS4_j"
ILP = "_Z22fp_fft_tile_1024x4_tw2I5T4IlpI8Fp128OpsELb%dEEv8TilePlanPK5elt_tjS6_j"
PATHS = ("j > 0", "j = 0")
# pass (0 = A, 1 = B) -> path -> wait states (the sum of imm + 1 over the s_nop) of fp_fft_tile_1024x4_tw2<Fp128Ops, ..>
TW2_WAIT = {0: {"j > 0": 2935, "j = 0": 2622}, 1: {"j > 0": 3401, "j = 0": 3088}}
# ceilings = the counts of the built code of the paired kernels
ILP_WAIT = {0: {"j > 0": 410, "j = 0": 434}, 1: {"j > 0": 595, "j = 0": 617}}
ILP_VALU = PATH_VALU  # the pairs neither add nor remove a VALU instruction
NOT_SALU = ("s_nop", "s_waitcnt", "s_load", "s_barrier")


def _instructions(lines):
    return [l for l in lines if fft_isa._is_instruction(l)]


def _counts(ins):
    """(VALU, SALU, wait states) of a list of instruction lines"""
    ops = [l.split()[0] for l in ins]
    return np.array([sum(op.startswith("v_") for op in ops), sum(op.startswith("s_") and not op.startswith(NOT_SALU) for op in ops),
                     sum(int(l.split()[1], 0) + 1 for l in ins if l.startswith("s_nop"))])


def _region(lines, tag):
    a, b = lines.index("; round 1, " + tag), lines.index("; round 1, " + tag + ": stored")
    assert a < b
    return _instructions(lines[a:b])


def _paths(name):
    """path -> (VALU, SALU, wait states) of a thread on that path"""
    lines = fft_isa.kernel(name).lines
    total = _counts(_instructions(lines))
    return {tag: total - _counts(_region(lines, other)) for tag, other in zip(PATHS, PATHS[::-1])}


@pytest.mark.parametrize("pass_b", [0, 1])
def test_ilp_kernels_isa(pass_b):
    name = ILP % pass_b
    k = fft_isa.kernel(name)
    fft_isa.assert_no_scratch_within_128_vgprs(name)
    assert not any(op.startswith(("scratch_", "buffer_", "flat_")) for op in k.ops)
    print(name, "VGPRs", k.desc["next_free_vgpr"])
    fft_isa.assert_scc_clean(name)
    fft_isa.assert_global_loads(name, LOADS[pass_b])
    assert fft_isa.dwordx4_loads_before_first_vmcnt_wait(name) >= LOADS[pass_b]
    first_wait = next(i for i, l in enumerate(k.lines) if l.startswith("s_waitcnt") and "vmcnt" in l)
    assert sum(l.startswith("s_load_dwordx4") for l in k.lines[:first_wait]) >= 10
    new, old = _paths(name), _paths(TW2 % pass_b)
    for tag in PATHS:
        print(name, tag, "VALU, SALU, wait states:", new[tag], "unpaired:", old[tag])
    for tag in PATHS:
        assert tuple(old[tag][[0, 2]]) == (PATH_VALU[pass_b][tag], TW2_WAIT[pass_b][tag])  # the figures the bounds below start from
        assert new[tag][0] <= PATH_VALU[pass_b][tag] and new[tag][0] <= ILP_VALU[pass_b][tag]
        assert new[tag][1] <= old[tag][1]
        assert 2 * new[tag][2] <= old[tag][2]
        assert new[tag][2] <= ILP_WAIT[pass_b][tag]


@pytest.mark.parametrize("pass_b", [0, 1])
def test_ilp_round_1_regions(pass_b):
    """as fp_fft_tile_1024x4_tw2: round 1 reads no twiddle from LDS, and every product there takes a limb of its twiddle from an SGPR"""
    k = fft_isa.kernel(ILP % pass_b)
    for tag, products in (("j > 0", 12), ("j = 0", 5)):
        body = _region(k.lines, tag)
        assert sum(l.startswith("ds_read_b128") for l in body) == 8 and sum(l.startswith("ds_write_b128") for l in body) == 8
        mads = [l for l in body if l.startswith("v_mad_u64_u32")]
        assert len(mads) == 16 * products
        assert all(any(o.strip().startswith("s") for o in l.split(None, 1)[1].split(",")[2:4]) for l in mads), tag


# ------------------------------------------------------------------ the hazard lint
# gfx950: 2 wait states between a VALU instruction that writes VCC or an SGPR and a VALU instruction that reads it as carry-in or
# as the mask of a v_cndmask.  hipcc pads its own code and nothing inside an asm statement.
CARRY_IN = re.compile(r"v_(addc|subb|subbrev)_co_u32(_e32|_e64)?$|v_cndmask_b32(_e32|_e64)?$")
TWO_DESTS = re.compile(r"v_\w+_co_[ui]32|v_mad_[ui]64_[ui]32|v_div_scale")


def _sregs(operand):
    """the scalar registers an operand names: 'vcc' -> {vcc_lo, vcc_hi}, 's[4:5]' -> {s4, s5}, 's7' -> {s7}"""
    o = operand.strip()
    if o == "vcc":
        return {"vcc_lo", "vcc_hi"}
    if o in ("vcc_lo", "vcc_hi"):
        return {o}
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", o)
    if m:
        return {"s%d" % i for i in range(int(m.group(1)), int(m.group(2)) + 1)}
    return {o} if re.fullmatch(r"s\d+", o) else set()


def _valu_sgpr_writes(line):
    op, rest = line.split(None, 1)
    operands = rest.split(",")
    regs = _sregs(operands[0])
    if TWO_DESTS.match(op) and len(operands) > 1:
        regs |= _sregs(operands[1])
    return regs


def hazards(lines):
    """the (producer, consumer, wait states) triples that break the rule, in program order as the text has it (a label is no
    boundary: the fall-through is the closer predecessor)"""
    ins, bad = _instructions(lines), []
    for i, l in enumerate(ins):
        op = l.split()[0]
        if not CARRY_IN.match(op):
            continue
        need = _sregs(l.split(None, 1)[1].split(",")[-1])
        assert need, l
        states = 0
        for p in reversed(ins[max(0, i - 2):i]):
            if states >= 2:
                break
            if p.startswith("v_") and _valu_sgpr_writes(p) & need:
                bad.append((p, l, states))
                break
            if p.startswith("s_") and not p.startswith("s_nop") and _sregs(p.split(None, 1)[1].split(",")[0]) & need:
                break  # the latest write is an SALU instruction's
            states += int(p.split()[1], 0) + 1 if p.startswith("s_nop") else 1
    return bad


def test_hazard_lint_finds_a_missing_wait_state():
    ok = ["v_add_co_u32_e32 v1, vcc, v2, v3", "s_nop 1", "v_addc_co_u32_e32 v4, vcc, v5, v6, vcc"]
    assert hazards(ok) == []
    assert hazards(ok[:1] + ["v_mov_b32_e32 v9, v8", "v_mov_b32_e32 v7, v8"] + ok[2:]) == []
    assert hazards(ok[:1] + ["s_nop 0"] + ok[2:]) == [(ok[0], ok[2], 1)]
    assert hazards(ok[:1] + ok[2:]) == [(ok[0], ok[2], 0)]
    e64 = ["v_mad_u64_u32 v[2:3], s[8:9], v4, s5, v[2:3]", "v_mov_b32_e32 v7, v8", "v_addc_co_u32_e64 v6, vcc, 0, v6, s[8:9]"]
    assert hazards(e64) == [(e64[0], e64[2], 1)]
    assert hazards(e64[:2] + ["s_nop 0"] + e64[2:]) == []
    assert hazards(["v_sub_co_u32_e64 v1, s[4:5], v2, v3", "s_nop 0", "v_cndmask_b32_e64 v1, 0, v2, s[4:5]"]) == [
        ("v_sub_co_u32_e64 v1, s[4:5], v2, v3", "v_cndmask_b32_e64 v1, 0, v2, s[4:5]", 1)]
    # an SALU write in between is the latest write, and needs none
    assert hazards(["v_addc_co_u32_e64 v1, s[4:5], v2, v3, vcc", "s_andn2_b64 s[4:5], s[6:7], s[4:5]", "v_cndmask_b32_e64 v1, 0, v2, s[4:5]"]) == []


@pytest.mark.parametrize("name", [ILP % 0, ILP % 1, TW2 % 0, TW2 % 1])
def test_carry_hazards(name):
    lines = fft_isa.kernel(name).lines
    consumers = sum(bool(CARRY_IN.match(l.split()[0])) for l in _instructions(lines))
    print(name, "carry-in and mask readers:", consumers)
    assert consumers > 1000
    assert hazards(lines) == []


# ------------------------------------------------------------------ on the GPU
SETTINGS = {"default": {}, "ilp0": {"LFGPU_FP_ILP": "0"}, "r1wave0": {"LFGPU_FP_R1WAVE": "0"}, "lazy0": {"LFGPU_FP_LAZY": "0"}}
SWITCHES = ("LFGPU_FP_ILP", "LFGPU_FP_R1WAVE", "LFGPU_FP_LAZY", "LFGPU_FP_TWSIDE", "LFGPU_FP_PERSIST", "LFGPU_FP_TILE1024", "LFGPU_FP_TW",
            "LFGPU_FP_ROWFAST", "LFGPU_TILE_LOG")


def _child(setting, cin, cout):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(setting)
    r = subprocess.run([sys.executable, CHILD, cin, cout], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(cout)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ilp")
    cin = str(d / "cases.npz")
    np.savez(cin, **_inputs())
    return {name: _child(env, cin, str(d / (name + ".npz"))) for name, env in SETTINGS.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_key)
def test_ilp_matches_other_kernels_and_oracle(runs, case):
    """the four settings byte-identical and equal to the oracle's fftb / fftf; row padding untouched"""
    k = _key(case)
    got = runs["default"][k]
    for other in ("ilp0", "r1wave0", "lazy0"):
        assert got.tobytes() == runs[other][k].tobytes(), other
    assert (got == _want()[k]).all()

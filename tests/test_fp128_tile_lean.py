"""K1 at n = 2^20 without the address arithmetic (csrc/fft.hip, fp_fft_tile_1024x4_lean<T4Ilp<Fp128Ops>, ..>, the default;
csrc/fp_tile_arith.h, fpt_bfly2_full): the ISA of the two kernels next to fp_fft_tile_1024x4_tw2<T4Ilp<Fp128Ops>, ..>, which
LFGPU_FP_LEAN=0 launches, from the same build; Python models of its LDS byte addresses, of its stage-twiddle tables under the bank
model of test_fp128_tile_r1wave_layout.py and of its tile order; fpt_bfly2_full on 2^20 operand sets against Python integers and
the single routines (tests/fp_tile_full_check.hip); and the default launches next to LFGPU_FP_LEAN=0 and the oracle, each setting
in a child process (tests/fp_tile_child.py).

A thread runs one of the two round-1 paths (j > 0, j = 0), so a path's static count is the kernel's minus the other path's round
1, as in test_fp128_tile_ilp.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fft_isa
from test_fp128_tile_ilp import CARRY_IN, ILP, ILP_WAIT, PATHS, SWITCHES, _instructions, _paths, _sregs, _valu_sgpr_writes, hazards
from test_fp128_tile_r1wave import CASES, CHILD, LOADS, PATH_VALU, _inputs, _key, _want
from test_fp128_tile_r1wave_layout import bitrev7, slot_new, swz
from test_fp_tile_arith import P, ROOT, _hipcc
from test_fp_tile_mul50 import MARK, PATTERNS, _ints, _limbs

LEAN = "_Z23fp_fft_tile_1024x4_leanI5T4IlpI8Fp128OpsELb%dEEv8TilePlanPK5elt_tjS6_jj"
# pass (0 = A, 1 = B) -> path -> VALU instructions per thread of 8 elements: ceilings = the counts of the built code.  The pins of
# fp_fft_tile_1024x4_tw2<T4Ilp<..>> are PATH_VALU, 2536 / 2244 and 2983 / 2691; the arithmetic alone (product 50, lazy butterfly
# 18, full butterfly 21, canon 8) is FLOOR.
LEAN_VALU = {0: {"j > 0": 2449, "j = 0": 2157}, 1: {"j > 0": 2894, "j = 0": 2602}}
FLOOR = {0: {"j > 0": 2382, "j = 0": 2088}, 1: {"j > 0": 2826, "j = 0": 2532}}
LEAN_WAIT = {0: {"j > 0": 348, "j = 0": 370}, 1: {"j > 0": 412, "j = 0": 434}}  # ceilings = the built code; 410 / 434 and 595 / 617 before
FULL_PAIRS = {0: 1, 1: 3}  # fpt_bfly2_full: round 0's one pair, and in pass B the last stage of round 3's two groups
CU_LDS = 160 * 1024


def _asm_blocks(lines):
    """the instruction lists of the kernel's asm statements"""
    out, cur = [], None
    for l in lines:
        if l.startswith(";;#ASMSTART"):
            cur = []
        elif l.startswith(";;#ASMEND"):
            out.append(cur)
            cur = None
        elif cur is not None and fft_isa._is_instruction(l):
            cur.append(l)
    return out


def _outside_asm(lines):
    out, inside = [], False
    for l in lines:
        if l.startswith(";;#ASMSTART") or l.startswith(";;#ASMEND"):
            inside = l.startswith(";;#ASMSTART")
        elif not inside and fft_isa._is_instruction(l):
            out.append(l)
    return out


@pytest.mark.parametrize("pass_b", [0, 1])
def test_lean_kernels_isa(pass_b):
    name = LEAN % pass_b
    k = fft_isa.kernel(name)
    fft_isa.assert_no_scratch_within_128_vgprs(name)
    assert not any(op.startswith(("scratch_", "buffer_", "flat_")) for op in k.ops)
    print(name, "VGPRs", k.desc["next_free_vgpr"], "SGPRs", k.desc["next_free_sgpr"])
    fft_isa.assert_scc_clean(name)
    fft_isa.assert_global_loads(name, LOADS[pass_b] + 1)  # + the 64 entries w^(8j), one per lane
    assert fft_isa.dwordx4_loads_before_first_vmcnt_wait(name) >= LOADS[pass_b] + 1
    first_wait = next(i for i, l in enumerate(k.lines) if l.startswith("s_waitcnt") and "vmcnt" in l)
    assert sum(l.startswith("s_load_dwordx4") for l in k.lines[:first_wait]) >= 10
    new, old = _paths(name), _paths(ILP % pass_b)
    for tag in PATHS:
        print(name, tag, "VALU, SALU, wait states:", new[tag], "fp_fft_tile_1024x4_tw2<T4Ilp>:", old[tag], "floor:", FLOOR[pass_b][tag])
    for tag in PATHS:
        assert old[tag][0] == PATH_VALU[pass_b][tag] and old[tag][2] == ILP_WAIT[pass_b][tag]  # the figures the bounds start from
        assert new[tag][0] < PATH_VALU[pass_b][tag]
        assert FLOOR[pass_b][tag] <= new[tag][0] <= LEAN_VALU[pass_b][tag]
        assert new[tag][2] <= LEAN_WAIT[pass_b][tag]
    if pass_b:
        assert new["j > 0"][2] < 595 and new["j = 0"][2] < 617


@pytest.mark.parametrize("pass_b", [0, 1])
def test_lean_addresses(pass_b):
    """Global memory through a scalar base and a 32-bit offset, no 64-bit vector arithmetic outside the products; every LDS access
    16 bytes wide; no static LDS (the tile starts at LDS address 0, which the integer addresses rest on), and the dynamic size
    the host launches with lets two workgroups share a CU."""
    k = fft_isa.kernel(LEAN % pass_b)
    glob = [l for l in k.lines if l.startswith("global_")]
    assert len(glob) == LOADS[pass_b] + 1 + 8
    for l in glob:
        ops = [o.strip() for o in l.split(None, 1)[1].split(",")]
        addr, base = (ops[1], ops[2]) if l.startswith("global_load") else (ops[0], ops[2])
        assert re.fullmatch(r"v\d+", addr) and re.match(r"s\[\d+:\d+\]", base), l
    outside = [l.split()[0] for l in _outside_asm(k.lines)]
    # (the compiler may form a 32-bit offset kb sk + c sc with v_mad_u64_u32 and use the low half: a multiply-add, no address)
    wide = [op for op in outside if re.match(r"v_(lshl_add_u64|lshlrev_b64|lshrrev_b64|ashrrev_i64|add_co_u32|addc_co_u32|add_u64)", op)]
    assert wide == [], wide
    assert not any(op.startswith("v_") and "f32" in op for op in outside)  # the tile order's division went through float
    ds = [op for op in k.ops if op.startswith("ds_")]
    assert set(ds) == {"ds_read_b128", "ds_write_b128"}, set(ds)
    assert k.desc["group_segment_fixed_size"] == 0
    src = open(fft_isa.FFT).read()
    m = re.search(r"enum : u32 \{ T4L_W = (\d+), T4L_W8 = T4L_W \+ (\d+), T4L_LDS = T4L_W8 \+ (\d+) \};", src)
    lds = sum(int(g) for g in m.groups())
    assert m.group(1) == "65536" and lds == 65536 + 8192 + 1024 and 2 * lds <= CU_LDS
    assert src.count("T4L_LDS, c->stream") == 1  # the launch's dynamic LDS size


# ------------------------------------------------------------------ fpt_bfly2_full in the built code
def _mask_reads(line):
    """the scalar registers an instruction reads as carry-in or mask (VALU), or as sources (s_andn2_b64)"""
    op, rest = line.split(None, 1)
    operands = rest.split(",")
    if CARRY_IN.match(op):
        return _sregs(operands[-1])
    if op == "s_andn2_b64":
        return _sregs(operands[1]) | _sregs(operands[2])
    return set()


def full_pair_rule(block):
    """the (producer, consumer, instructions in between) triples of one asm statement that break the 2-wait-state rule of
    fp_tile_arith.h, the SALU readers of a VALU-written mask included; the statement has no s_nop, so every instruction is one"""
    bad = []
    for i, l in enumerate(block):
        need = _mask_reads(l)
        for back in (1, 2):
            if i - back >= 0 and block[i - back].startswith("v_") and _valu_sgpr_writes(block[i - back]) & need:
                bad.append((block[i - back], l, back - 1))
    return bad


@pytest.mark.parametrize("pass_b", [0, 1])
def test_full_pair_in_the_built_code(pass_b):
    """fpt_bfly2_full's statements in the kernel: 42 VALU instructions each, no s_nop, two s_andn2_b64, and the carry rule"""
    k = fft_isa.kernel(LEAN % pass_b)
    blocks = [b for b in _asm_blocks(k.lines) if sum(l.startswith("s_andn2_b64") for l in b) == 2 and any(l.startswith("v_subrev_co_u32") for l in b)
              and not any(l.startswith("v_mad_u64_u32") for l in b)]
    assert len(blocks) == FULL_PAIRS[pass_b]
    for b in blocks:
        assert sum(l.startswith("v_") for l in b) == 42 and len(b) == 44 and not any(l.startswith("s_nop") for l in b)
        assert sum(bool(_mask_reads(l)) for l in b) >= 34
        assert full_pair_rule(b) == [] and hazards(b) == []
    # the rule's checker sees a link that is too short
    b = list(blocks[0])
    i = next(i for i, l in enumerate(b) if l.startswith("s_andn2_b64"))
    b[i - 2], b[i - 4] = b[i - 4], b[i - 2]  # the last v_subb_co_u32 of p's s - p chain next to its s_andn2_b64
    assert full_pair_rule(b) != []


@pytest.mark.parametrize("pass_b", [0, 1])
def test_lean_carry_hazards(pass_b):
    lines = fft_isa.kernel(LEAN % pass_b).lines
    assert sum(bool(CARRY_IN.match(l.split()[0])) for l in _instructions(lines)) > 1000
    assert hazards(lines) == []


# ------------------------------------------------------------------ models of the addresses
def t4l_byte(p, c):
    return ((p << 6) | (c << 4)) ^ ((p >> 3) & 0x70) ^ (p & 0xC0)


def test_lds_byte_addresses():
    """t4l_byte is 16 t4w_slot, and every round's addresses, a base per thread and constants, are those of the slot function"""
    assert all(t4l_byte(p, c) == 16 * slot_new(p, c) for p in range(1024) for c in range(4))
    assert [16 * swz(64 * a) for a in range(4)] == [0, 64, 144, 208] and 16 * swz(128) == 144 and 16 * swz(512) == 64
    for kb in range(128):  # round 0
        for c in range(4):
            s0 = t4l_byte(bitrev7(kb) << 3, c)
            assert all((s0 ^ (64 * (a & 3))) + 256 * (a >> 2) == 16 * slot_new(8 * bitrev7(kb) + a, c) for a in range(8))
    for tid in range(512):
        c = tid & 3
        j, h = tid >> 6, (tid >> 2) & 15  # round 1
        s0 = t4l_byte(h << 6, c) ^ (j << 6)
        assert all(s0 + 512 * a == 16 * slot_new(64 * h + j + 8 * a, c) for a in range(8))
        j = (tid >> 2) & 63  # round 2: group 1 takes group 0's four addresses in the order a ^ 1
        s0 = t4l_byte(((tid >> 8) << 8) | j, c)
        sa = [s0, s0 ^ 64, s0 ^ 144, s0 ^ 208]
        for g in range(2):
            e = tid + 512 * g
            assert (e & 3, (e >> 2) & 63) == (c, j)
            assert all(sa[a ^ g] + 4096 * a + 32768 * g == 16 * slot_new(256 * (e >> 8) + j + 64 * a, c) for a in range(4))
        s0 = t4l_byte(tid >> 2, c)  # round 3
        for g in range(2):
            e = tid + 512 * g
            sg = s0 ^ 144 if g else s0
            assert all((sg ^ (32 * a)) + 16384 * a + 8192 * g == 16 * slot_new((e >> 2) + 256 * a, e & 3) for a in range(4))


T4L_W, T4L_W8 = 65536, 65536 + 8192


def twiddle_reads():
    """(name, [(byte address, twiddle index i of w_1024^i) per thread]) for every stage-twiddle read of rounds 2 and 3"""
    out = []
    r2 = [((tid << 2) & 0x3F0, (tid >> 2) & 63) for tid in range(512)]
    out.append(("round 2, 8j", [(T4L_W8 + j16, 8 * j) for j16, j in r2]))
    out.append(("round 2, 4j", [(T4L_W + 4 * j16, 4 * j) for j16, j in r2]))
    out.append(("round 2, 4j + 256", [(T4L_W + 4 * j16 + 4096, 4 * j + 256) for j16, j in r2]))
    for g in range(2):
        js = [(tid + 512 * g) >> 2 for tid in range(512)]
        wa = [T4L_W + ((tid << 3) & ~31) for tid in range(512)]
        wb = [T4L_W + ((tid << 2) & ~15) for tid in range(512)]
        out.append(("round 3, 2j, g = %d" % g, [(a + 4096 * g, 2 * j) for a, j in zip(wa, js)]))
        out.append(("round 3, j, g = %d" % g, [(b + 2048 * g, j) for b, j in zip(wb, js)]))
        out.append(("round 3, j + 256, g = %d" % g, [(b + 2048 * g + 4096, j + 256) for b, j in zip(wb, js)]))
    return out


def test_stage_twiddle_tables():
    """Each read finds its twiddle: w^i at T4L_W + 16 i, i < 512, and w^(8j) at T4L_W8 + 16 j, j < 64, the indices those of
    t4i_stages4 (j << sh, (j + 2^ST) << sh).  Under the bank model of test_fp128_tile_r1wave_layout.py (ds_read_b128: 16
    consecutive lanes at a time on 64 banks; lanes that read the same address are one access) no group has a conflict; the
    linear table read at i = 8j would have one, which is why the second table is there.  The writes (ds_write_b128, 8 lanes on
    32 banks) are linear in the lane."""
    def ways(addrs, lanes):
        worst = 0
        for g in range(0, len(addrs), lanes):
            res = [a // 16 % lanes for a in set(addrs[g:g + lanes])]
            worst = max(worst, max(res.count(r) for r in set(res)))
        return worst

    for name, reads in twiddle_reads():
        for addr, i in reads:
            assert addr % 16 == 0 and i < 512
            assert addr == T4L_W + 16 * i or (i % 8 == 0 and addr == T4L_W8 + 2 * i), (name, addr, i)
        assert ways([a for a, _ in reads], 16) == 1, name
    assert ways([T4L_W + 16 * 8 * ((tid >> 2) & 63) for tid in range(512)], 16) == 2
    assert ways([T4L_W + 16 * tid for tid in range(512)], 8) == 1 and ways([T4L_W8 + 16 * tid for tid in range(64)], 8) == 1
    for st, sh0 in ((6, 3), (8, 1)):  # t4i_stages4: stage t reads j << (9 - ST - t) and, for t = 1, (j + 2^ST) << (9 - ST - 1)
        assert sh0 == 9 - st and (1 << st) << (sh0 - 1) == 256


def test_tile_order_by_shifts():
    """t4_xcd_order for 2^lcb >= 8 column blocks: quotient and remainder by shifts and masks"""
    for lcb in range(3, 11):
        ncb = 1 << lcb
        for w in list(range(4 * ncb)) + [ncb * 1024 - 1]:
            per, i = ncb >> 3, w >> 3
            want = ((w & 7) * per + i % per, i // per)
            sh = lcb - 3
            assert (((w & 7) << sh) + (i & ((1 << sh) - 1)), i >> sh) == want


# ------------------------------------------------------------------ fpt_bfly2_full on the GPU
CHECK = os.path.join(ROOT, "tests", "fp_tile_full_check.hip")
N_SETS, N_DIV = 1 << 20, 1 << 17
KINDS, MODES = ("sub", "add"), ("all", "none", "alternating")
RES = 5
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
FULL_EDGES = [0, 1, 2, P - 1, P - 2, (P - 1) >> 1, (P + 1) >> 1, 2**108 - 1, 2**108, 2**127, 2**64 - 1, 2**64, 2**96, 2**128 % P, P - 2**128 % P]


def taken(kind, u, t):
    """from the integers: does fpt_sub(u, t) add p; does fpt_add(u, t) subtract p"""
    return u < t if kind == "sub" else u + t >= P


def _rand_canon(rng):
    """uniform below p, or within 2^64 of 0 or of p: every outcome can be met for any partner"""
    u, how = int.from_bytes(rng.bytes(16), "little") % P, rng.integers(3)
    return u if how == 0 else u >> 64 if how == 1 else P - 1 - (u >> 64)


def _built_waves(rng):
    """waves in which every lane, no lane and every second lane takes the +-p, for p's half and for q's in all nine combinations"""
    sets = []
    for kind in KINDS:
        for mp in MODES:
            for mq in MODES:
                for lane in range(64):
                    row = []
                    for mode in (mp, mq):
                        u, t = _rand_canon(rng), _rand_canon(rng)
                        while taken(kind, u, t) != (mode == "all" or (mode == "alternating" and lane % 2 == 0)):
                            u, t = _rand_canon(rng), _rand_canon(rng)
                        row += [u, t]
                    sets.append(row)
    return sets


@pytest.fixture(scope="module")
def operands():
    """(the 2^20 operand sets as (n, 8) uint64, every value < p; the reference (n, 4, 2)), computed once"""
    rng = np.random.default_rng(20261027)
    edge = [(u, t) for u in FULL_EDGES for t in FULL_EDGES]
    assert len(edge) % 2 == 1  # odd: tiled, p's half and q's meet every pair at every lane parity
    sets = _built_waves(rng)
    n_edge = 1 << 12
    sets += [list(edge[i % len(edge)]) + list(edge[(7 * i + 3) % len(edge)]) for i in range(n_edge)]
    raw = rng.integers(0, 2**64, size=(N_SETS - len(sets), 8), dtype=np.uint64)
    raw[:, 1::2] %= np.uint64(P >> 64)  # high limb below p's: the value < p
    raw[1::4, 1] = np.uint64((P >> 64) - 1) - (raw[1::4, 1] >> np.uint64(44))  # u near p: the sum often passes p
    raw[2::4, 5] = np.uint64((P >> 64) - 1) - (raw[2::4, 5] >> np.uint64(44))
    arr = np.concatenate([np.concatenate([_limbs([r[k] for r in sets]) for k in range(4)], axis=1), raw])
    assert arr.shape == (N_SETS, 8) and len(sets) <= N_DIV
    up, tp, uq, tq = (_ints(arr[:, 2 * k:2 * k + 2]) for k in range(4))
    assert all(max(v) < P for v in (up, tp, uq, tq))
    ref = np.stack([_limbs([(u + t) % P for u, t in zip(up, tp)]), _limbs([(u - t) % P for u, t in zip(up, tp)]),
                    _limbs([(u + t) % P for u, t in zip(uq, tq)]), _limbs([(u - t) % P for u, t in zip(uq, tq)])], axis=1)
    w = 0
    for kind in KINDS:  # the built waves are what they are meant to be
        for mp in MODES:
            for mq in MODES:
                for us, ts, mode in ((up, tp, mp), (uq, tq, mq)):
                    assert [taken(kind, us[i], ts[i]) for i in range(64 * w, 64 * w + 64)] == \
                        [mode == "all" or (mode == "alternating" and lane % 2 == 0) for lane in range(64)]
                w += 1
    arr.setflags(write=False)
    ref.setflags(write=False)
    return arr, ref


def test_reference_of_the_full_pair_check(operands):
    """without a GPU: both outcomes of each conditional +-p are frequent in p's half and in q's"""
    arr, _ = operands
    for k in (0, 2):
        us, ts = _ints(arr[:, 2 * k:2 * k + 2]), _ints(arr[:, 2 * k + 2:2 * k + 4])
        for yes in (sum(u < t for u, t in zip(us, ts)), sum(u + t >= P for u, t in zip(us, ts))):
            assert min(yes, N_SETS - yes) >= N_SETS // 8


@pytest.mark.gpu
def test_full_pair_all_lanes_and_divergent_device(operands, tmp_path):
    exe = tmp_path / "fp_tile_full_check"
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-o", str(exe), CHECK])
    arr, ref = operands
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    arr.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout), str(N_DIV)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    sizes = [N_SETS] + [N_DIV] * (len(PATTERNS) - 1)
    raw = np.fromfile(fout, dtype=np.uint8)
    assert len(raw) == sum(sizes) * (RES * 16 + 4)
    at, recs = 0, []
    for m in sizes:
        recs.append(raw[at:at + m * RES * 16].view(np.uint64).reshape(m, RES, 2))
        at += m * RES * 16
    for p, name in enumerate(PATTERNS):
        m = sizes[p]
        marks = raw[at:at + 4 * m].view(np.uint32)
        at += 4 * m
        lane = np.arange(m) & 63
        on = (np.ones(m, bool), lane % 2 == 0, lane == 63, lane < 32)[p]
        got = recs[p][on]
        bad = np.flatnonzero((got[:, :4] != ref[:m][on]).any(axis=(1, 2)))
        assert not len(bad), (name, len(bad), np.flatnonzero(on)[bad[:4]], got[bad[:4], :4], ref[:m][on][bad[:4]])
        assert (got[:, 4, 0] == np.uint64(MARK << 32)).all() and (got[:, 4, 1] == np.uint64(MARK << 32 | MARK)).all(), name  # = fpt_add, fpt_sub
        assert (recs[p][~on] == SENTINEL).all(), name
        assert (marks == (np.arange(m, dtype=np.uint32) ^ np.uint32(MARK))).all(), name


# ------------------------------------------------------------------ the transforms on the GPU
SETTINGS = {"default": {}, "lean0": {"LFGPU_FP_LEAN": "0"}}


def _child(setting, cin, cout):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES + ("LFGPU_FP_LEAN",)}
    env.update(setting)
    r = subprocess.run([sys.executable, CHILD, cin, cout], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(cout)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lean")
    cin = str(d / "cases.npz")
    np.savez(cin, **_inputs())
    return {name: _child(env, cin, str(d / (name + ".npz"))) for name, env in SETTINGS.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_key)
def test_lean_matches_the_pair_it_replaces_and_oracle(runs, case):
    """2^20 x 2 rows both ways (a random row and the rows that force non-canonical intermediates), ld > n, and 2^21 x 1 row: the
    default, LFGPU_FP_LEAN=0 and the oracle's fftb / fftf byte-identical, row padding untouched.  A 2^20 transform runs every
    wave of a tile, so both paths of round 1."""
    k = _key(case)
    got = runs["default"][k]
    assert got.tobytes() == runs["lean0"][k].tobytes()
    assert (got == _want()[k]).all()

"""The LDS layout and the lazy rule of fp_fft_tile_1024x4_tw2 (csrc/fft.hip), the 1024 x 4 tile pair whose round 1 gives a wave
one twiddle index j: a model of every LDS data access of the four rounds under the lane groups of DESIGN 4.1, and a Python-integer
model of the j = 0 wave's round 1, which leaves its seven products by w^0 out.

Bank model: ds_read_b128 is served 16 consecutive lanes at a time on 64 banks, so a group is free of conflicts when its slots
(16 bytes each) are distinct mod 16; ds_write_b128 8 lanes at a time on 32 banks, distinct mod 8.  The figure reported is the
largest number of lanes of one group that meet in one residue (1 = no conflict)."""
import random

import pytest

P = 2**128 - 2**108 + 1
T128 = 2**128


# ------------------------------------------------------------------ the layouts
def swz(p):
    """L(p) of t4w_swz: p6 -> 4, p7 -> 9, p8 -> 2, p9 -> 4"""
    return (p >> 7) ^ ((p >> 4) & 12)


def slot_new(p, c):
    return ((p << 2) | c) ^ swz(p)


def slot_old(p, c):
    """t4_slot: (4p + c) ^ (p >> 7)"""
    return ((p << 2) | c) ^ (p >> 7)


def bitrev7(k):
    return int(format(k, "07b")[::-1], 2)


# ------------------------------------------------------------------ the accesses: name -> one list of 512 (position, column) per instruction
def round0(pass_b):
    """thread (kb, c) writes positions 8 bitrev7(kb) + a; pass A: tid = 4 kb + c, pass B: tid = 128 c + kb"""
    out = []
    for a in range(8):
        ins = []
        for tid in range(512):
            c, kb = (tid >> 7, tid & 127) if pass_b else (tid & 3, tid >> 2)
            ins.append((8 * bitrev7(kb) + a, c))
        out.append(ins)
    return out


def round1(wave):
    """positions 64h + j + 8a; wave: j = tid >> 6, (c, h) = (lane & 3, lane >> 2); otherwise (c, j, h) = (tid & 3, (tid >> 2) & 7, tid >> 5)"""
    out = []
    for a in range(8):
        ins = []
        for tid in range(512):
            c, j, h = (tid & 3, tid >> 6, (tid >> 2) & 15) if wave else (tid & 3, (tid >> 2) & 7, tid >> 5)
            ins.append((64 * h + j + 8 * a, c))
        out.append(ins)
    return out


def round2():
    """group e = tid + 512 g: (c, j, h) = (e & 3, (e >> 2) & 63, e >> 8), positions 256h + j + 64a"""
    return [[(256 * (e >> 8) + ((e >> 2) & 63) + 64 * a, e & 3) for e in range(512 * g, 512 * g + 512)] for g in range(2) for a in range(4)]


def round3():
    """group e = tid + 512 g: (c, j) = (e & 3, e >> 2), positions j + 256a"""
    return [[((e >> 2) + 256 * a, e & 3) for e in range(512 * g, 512 * g + 512)] for g in range(2) for a in range(4)]


def accesses(wave):
    """(name, 'r' or 'w', instructions) for every LDS data access of a tile, both passes' round-0 lane maps"""
    r1 = round1(wave)
    return [("round 0 write, pass A", "w", round0(False)), ("round 0 write, pass B", "w", round0(True)), ("round 1 read", "r", r1),
            ("round 1 write", "w", r1), ("round 2 read", "r", round2()), ("round 2 write", "w", round2()), ("round 3 read", "r", round3())]


def ways(slot, kind, instructions):
    """the worst group of the worst instruction"""
    lanes = 16 if kind == "r" else 8
    worst = 0
    for ins in instructions:
        for g in range(0, 512, lanes):
            res = [slot(p, c) % lanes for p, c in ins[g:g + lanes]]
            worst = max(worst, max(res.count(r) for r in set(res)))
    return worst


# ------------------------------------------------------------------ tests of the layout
@pytest.mark.parametrize("slot", [slot_new, slot_old])
def test_layout_is_a_bijection(slot):
    assert sorted(slot(p, c) for p in range(1024) for c in range(4)) == list(range(4096))
    assert all(slot(p, c) >> 4 == p >> 2 for p in range(1024) for c in range(4))  # inside the aligned 16-slot row


def test_every_round_covers_the_tile():
    for wave in (False, True):
        for name, _, instructions in accesses(wave):
            assert sorted(pc for ins in instructions for pc in ins) == [(p, c) for p in range(1024) for c in range(4)], name


def test_new_layout_has_no_conflict():
    for name, kind, instructions in accesses(True):
        w = ways(slot_new, kind, instructions)
        print(name, w)
        assert w == 1, (name, w)


def test_model_sees_the_conflict_of_the_old_layout():
    """(4p + c) ^ (p >> 7) is free of conflicts with round 1's lanes = (c, j, h), and 4-way in round 1's reads with lanes = (c, h)"""
    for name, kind, instructions in accesses(False):
        assert ways(slot_old, kind, instructions) == 1, name
    got = {name: ways(slot_old, kind, instructions) for name, kind, instructions in accesses(True)}
    print(got)
    assert got["round 1 read"] == 4
    assert all(w == 1 for name, w in got.items() if not name.startswith("round 1"))


def test_conditions_on_l():
    """the conditions of the comment in fft.hip, which the four images of L meet"""
    l6, l7, l8, l9 = swz(64), swz(128), swz(256), swz(512)
    assert (l6, l7, l8, l9) == (4, 9, 2, 4) and all(swz(1 << b) == 0 for b in range(6))
    assert all(swz(p) == (l6 * (p >> 6 & 1)) ^ (l7 * (p >> 7 & 1)) ^ (l8 * (p >> 8 & 1)) ^ (l9 * (p >> 9 & 1)) for p in range(1024))  # linear

    def independent(vs, mask):
        sums = set()
        for m in range(1 << len(vs)):
            x = 0
            for i, v in enumerate(vs):
                if m >> i & 1:
                    x ^= v & mask
            sums.add(x)
        return len(sums) == 1 << len(vs)

    assert l9 & 4  # round-0 write, pass A
    assert independent([l7, l8, l9], 7)  # round-0 write, pass B
    assert independent([l6, l7], 12)  # round-1 read
    assert l6 & 4  # round-1 write


def test_kernel_offsets():
    """the slot expressions of the t4w_round* helpers, a base per thread and compile-time offsets, against the slot function"""
    for kb in range(128):
        for c in range(4):
            b = bitrev7(kb)
            s0 = slot_new(8 * b, c)
            for a in range(8):
                assert (s0 ^ (4 * (a & 3))) + 16 * (a >> 2) == slot_new(8 * b + a, c)
    for j in range(8):
        for h in range(16):
            for c in range(4):
                s0 = slot_new(64 * h + j, c)
                assert all(s0 + 32 * a == slot_new(64 * h + j + 8 * a, c) for a in range(8))
    for e in range(1024):
        c, h, j = e & 3, e >> 8, (e >> 2) & 63
        s0 = slot_new(256 * h + j, c)
        assert all((s0 ^ swz(64 * a)) + 256 * a == slot_new(256 * h + j + 64 * a, c) for a in range(4))
        s0 = slot_new(e >> 2, c)
        assert all((s0 ^ (2 * a)) + 1024 * a == slot_new((e >> 2) + 256 * a, c) for a in range(4))


# ------------------------------------------------------------------ the lazy rule of round 1
def _root1024():
    for g in range(2, 100):
        w = pow(g, (P - 1) // 1024, P)
        if pow(w, 512, P) == P - 1:
            return w
    raise AssertionError("no root")


W1024 = _root1024()
R1, R1_J0, R1_J0_AS_ROUND0 = "every product", "canon(v) for a skipped product", "round 0's rule: full adds, no canon"


def round1_model(x, j, mode):
    """Stages 3-5 of t4w_stages on x[a] = position 64h + j + 8a: 128-bit integers and a flag 'may be non-canonical' per value.
    A butterfly's v has to be < p (fpt_add_lazy, fpt_sub); returns (values, how often a v was not, how often a v was flagged)."""
    x = list(x)
    flag = [True] * 8  # what round 0 leaves in LDS is lazy
    bad_v = flagged_v = 0
    for t in range(3):
        half = 1 << t
        for a in range(8):
            if a & half:
                continue
            k = a & (half - 1)
            u, v, fu, fv = x[a], x[a + half], flag[a], flag[a + half]
            if mode == R1 or k != 0:
                v, fv = v * pow(W1024, (j + 8 * k) << (6 - t), P) % P, False
            elif mode == R1_J0:
                v, fv = v % P, False  # fpt_canon
            bad_v += v >= P
            flagged_v += fv
            full = mode == R1_J0_AS_ROUND0 and ((t == 0 and a != 0) or (t == 1 and a == 4))
            if full:
                x[a], flag[a] = (u + v) % P, fu or fv  # fpt_add: canonical only for canonical inputs
            else:
                x[a], flag[a] = (u + v if u + v < T128 else u + v - P), True  # fpt_add_lazy (one fold: needs v < p)
            x[a + half], flag[a + half] = (u - v if u >= v else u - v + P), fu  # fpt_sub: canonical for canonical u (needs v < p)
    return x, bad_v, flagged_v


def _lazy_inputs():
    rng = random.Random(20261020)
    edges = [0, 1, P - 1, P, P + 1, T128 - 1, T128 - 2, 2**108 - 1, 2**127]
    groups = [[e] * 8 for e in edges] + [[rng.choice(edges) for _ in range(8)] for _ in range(200)]
    groups += [[rng.randrange(P, T128) for _ in range(8)] for _ in range(200)] + [[rng.randrange(T128) for _ in range(8)] for _ in range(200)]
    return groups


def test_round1_without_its_w0_products():
    """In the j = 0 wave, seven of the twelve products are by w^0.  With canon(v) in their place no v of any butterfly is, or is
    flagged, non-canonical, the values stay below 2^128 and are congruent to those of the round with every product."""
    skipped = 0
    for x in _lazy_inputs():
        want, bad, flagged = round1_model(x, 0, R1)
        assert bad == 0 and flagged == 0
        got, bad, flagged = round1_model(x, 0, R1_J0)
        assert bad == 0 and flagged == 0, x
        assert all(0 <= v < T128 for v in got) and [v % P for v in got] == [v % P for v in want], x
    for t in range(3):
        skipped += sum(1 for a in range(8) if not a & (1 << t) and a & ((1 << t) - 1) == 0)
    assert skipped == 7


def test_round0_rule_does_not_carry_over():
    """the model can see a violation: with round 0's rule (full adds make the v of the w^0 butterflies, nothing made canonical) the
    lazy inputs of round 1 reach a butterfly as v >= p, because here stage 3's v come straight out of LDS"""
    total_bad = total_flagged = 0
    for x in _lazy_inputs():
        _, bad, flagged = round1_model(x, 0, R1_J0_AS_ROUND0)
        total_bad += bad
        total_flagged += flagged
    print(total_bad, total_flagged)
    assert total_bad >= 100 and total_flagged >= 100


@pytest.mark.parametrize("j", range(1, 8))
def test_other_waves_multiply_every_v(j):
    for x in _lazy_inputs()[:50]:
        got, bad, flagged = round1_model(x, j, R1)
        assert bad == 0 and flagged == 0 and all(0 <= v < T128 for v in got)

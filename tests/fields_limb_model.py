"""Instrumented limb models of the device's Fp128 and F64 arithmetic (csrc/fields.h, the __HIP_DEVICE_COMPILE__ path): fp_add, fp_sub,
fp_mul (the default one-step REDC), f64_sub, f64_add and f64_mul restated instruction chain by instruction chain on Python integers,
32-bit limbs that wrap as the registers do.  The models follow the assembly operands (%n), not the portable *_c code: v_sub / v_subb
take the second source from the first, v_subrev / v_subbrev the first from the second, v_cndmask reads vcc ? src1 : src0.  Each model
returns the result and the set of EVENTS the operand pair reached -- which carry and borrow links carried a one, which way each
selection went -- and takes `drop=`, the name of one link to leave out: the model of a kernel with that one link wrong.

tests/golden/fields_carry_pairs.json is a set of operand pairs per field, mined by this module's __main__ (seeded, deterministic),
that reaches every reachable event several times; tests/test_fields_limb_model.py checks that, and that every dropped link changes the
result of at least one committed pair.  tests/test_fields_arith_paths_gpu.py feeds the same pairs to the instructions themselves.

Event names (also the `drop=` names where the event is a link that carried).  Limbs are 32 bits, limb 0 the lowest.
 fp_add
  add.link.K            a carry entering limb K = 1..3 of a + b, K = 4: into the carry bit c
  add.ripple.K          K = 1..3: ... with a_K + b_K = 0xffffffff (mod 2^32): the carry goes through
  add.c.0 / .1          the carry bit
  add.subp.link.K       a borrow entering limb K = 1..3 of (c : s) - p, K = 4: into the carry bit's limb
  add.subp.ripple.K     K = 1, 2 (p's zero limbs): ... with s_K = 0, the borrow goes through
  add.sel.taken / .not  the selection of (c : s) - p
  add.sum.p / .pm1      a + b = p (result 0), a + b = p - 1
 fp_sub
  sub.link.K            a borrow entering limb K = 1..3 of a - b, K = 4: the borrow out
  sub.ripple.K          K = 1..3: ... with a_K = b_K, the borrow goes through
  sub.m.0 / .1          the borrow out (p is added back or not)
  sub.eq                a = b
  sub.addp.link.K       a carry entering limb K = 1..3 of the add-back chain
  sub.addp.ripple.K     K = 1, 2: ... with that limb 0xffffffff, the carry goes through
 fp_mul (T = a b = (t0 .. t7), T_lo = (t0 .. t3), T_hi = (t4 .. t7))
  mul.pc.I.J            the carry out of the 64-bit accumulate of a_I * b_J
  mul.u3.wrap / .not    u3 = t3 + (t0 << 12) wrapping mod 2^32 or not
  mul.tlo.zero          T_lo = 0
  mul.m.link.K          a borrow entering limb K = 1..3 of m = 0 - (t0, t1, t2, u3)
  mul.m.ripple.K        K = 1, 2: ... with that limb of the subtrahend zero
  mul.q.link.K          a borrow entering limb K = 1..3 of q = m - (m >> 20)
  mul.q.ripple.K        K = 1, 2: ... with the two limbs equal
  mul.dl.link.K         a carry entering limb K = 1..3 of T_lo + m (the delta chain; its sums are discarded)
  mul.dl.ripple.3       ... with t3 + m3 = 0xffffffff.  (Links 1 and 2 ALWAYS meet a limb sum of 0xffffffff: see DELTA_STRUCTURE.)
  mul.delta.0 / .1      delta, the carry out of T_lo + m into T_hi + q; drop name mul.delta
  mul.hi.link.K         a carry entering limb K = 1..3 of T_hi + q + delta, K = 4: into t8
  mul.hi.ripple.K       K = 1..3: ... with t_(4+K) + q_K = 0xffffffff
  mul.t8.0 / .1         t8
  mul.subp.link.K, mul.subp.ripple.K, mul.sel.taken / .not     as in fp_add, on (t8 : t7 .. t4)
  mul.v.ge_p / .lt_p    the value before the selection in [p, 2p) or in [0, p)
 f64_sub (and, as f64add.sub.*, the same chain inside f64_add)
  f64sub.link.1         a borrow entering the high limb of a - b
  f64sub.ripple.1       ... with a1 = b1
  f64sub.m.0 / .1       the borrow out, which becomes the mask; drop name f64sub.m
  f64sub.fix.0 / .1     under the mask: d0 - 0xffffffff borrowing into the high limb (.1) or, d0 = 0xffffffff, not (.0); drop name
                        f64sub.fix, and f64sub.fix.always for the link forced to one
  f64sub.eq             a = b
 f64_add
  f64add.nb.link.1 / .nolink    p - b: the borrow out of 1 - b0 (b0 > 1) or none (b0 <= 1)
  f64add.b.zero, f64add.sum.p   b = 0 (p - b = p, not reduced), a + b = p
 f64_mul (a b = (l0, l1, h0, h1))
  f64mul.e.0 / .1       the carry of x = l1 + l0; drop name f64mul.e
  f64mul.yb.0 / .1      the borrow of y = l0 - x - e, which x - borrow takes; drop name f64mul.yb
  f64mul.hb.link.1      a borrow entering the high limb of hi - (y, x)
  f64mul.hb.ripple.1    ... with h1 = x
  f64mul.neg.0 / .1     hi - (y, x) negative or not (the mask); drop name f64mul.neg
  f64mul.fix.0 / .1     as f64sub.fix; drop names f64mul.fix, f64mul.fix.always

Events that cannot occur for operands below the modulus are listed in UNREACHABLE with their bounds; the models assert that they
never fire.  EQUIVALENT lists the links whose loss no operand pair can show (none here, see there).

TEST INFRASTRUCTURE: nothing outside tests/ imports this module."""
import json
import os
import random

P = 2**128 - 2**108 + 1
P64 = 2**64 - 2**32 + 1
M32 = 2**32 - 1
M64 = 2**64 - 1
R_INV = pow(2**128, -1, P)
R64_INV = pow(2**64, -1, P64)
PW = (1, 0, 0, 0xFFFFF000)
PAIRS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fields_carry_pairs.json")

# the product scan's columns: (i, j) in the order the device issues them; FP_MAD captures no carry, FP_MADC adds it to ov
COLUMNS = tuple(tuple((i, k - i) for i in range(max(0, k - 3), min(3, k) + 1)) for k in range(7))
UNCAPTURED = ((0, 0), (0, 1), (3, 3))
_PC = {(i, j): "mul.pc.%d.%d" % (i, j) for col in COLUMNS for (i, j) in col}

# ---- what cannot happen for operands below the modulus (asserted in the models whenever no link is dropped)
UNREACHABLE = {
    # the three the device does not capture (FP_MAD)
    "mul.pc.0.0": "acc = 0 before it",
    "mul.pc.0.1": "acc <= 2^32 - 2 before it, the product <= 2^64 - 2^33 + 1",
    # the scan is exact: after the last accumulate (acc : carry) = floor(a b / 2^192) < 2^64 since a b < 2^256
    "mul.pc.3.3": "acc + a3 b3 = floor(a b / 2^192) < 2^64",
    # four that the device captures although they cannot fire.  Column 1's true sum is <= (2^32 - 2) + 2 (2^32 - 1)^2 = 2^65 - 3 2^32,
    # so column 2 comes in with acc <= 2^33 - 3 and a0 b2 <= 2^64 - 2^33 + 1 brings it to 2^64 - 2 at the most
    "mul.pc.0.2": "acc <= 2^33 - 3 before it, the product <= 2^64 - 2^33 + 1",
    # b3 <= 0xfffff000 for b < p and a column comes in with acc < 2^34 (at most three captured carries above a 32-bit half):
    # acc + a_i b3 < 2^34 + (2^32 - 1) 0xfffff000 < 2^64 (tests/test_fp_tile_mul_carries.py; first_accumulate_max() evaluates it)
    "mul.pc.0.3": "acc < 2^34 before it, a0 b3 <= (2^32 - 1) 0xfffff000",
    "mul.pc.1.3": "acc < 2^34 before it, a1 b3 <= (2^32 - 1) 0xfffff000",
    "mul.pc.2.3": "acc < 2^34 before it, a2 b3 <= (2^32 - 1) 0xfffff000",
    # q = m - (m >> 20) with 0 <= m >> 20 <= m: the difference of the 128-bit values is not negative, so the chain's last borrow is 0
    "mul.q.link.4": "m >> 20 <= m",
    # v = (a b + m p) / 2^128 < 2p, and v = p needs a b = 0 (mod p): a or b is zero, then T = 0, m = 0 and v = 0
    "mul.v.p": "v = p only if a b = 0 (mod p), and then v = 0",
    # p - b > 0 for b < p: 1 - b0 borrows only for b0 >= 2, and then 0xffffffff - b1 - 1 borrows only for b1 = 0xffffffff: b >= p + 1
    "f64add.nb.link.2": "p - b > 0",
    # x = (l0 + l1) mod 2^32 = 0 either with e = 0, then l0 = l1 = 0 and y = 0 - 0 - 0 does not borrow, or with e = 1, then l0 >= 1 and
    # y = l0 - 0 - 1 does not borrow: the borrow of y never meets x = 0.  (y borrows exactly when e = 0 and l1 > 0: then x = l0 + l1 > l0.)
    "f64mul.xb": "y borrows only with e = 0 and l1 > 0, and then x = l0 + l1 >= 1",
    # t0 = a0 b0; t1 = (t0 >> 32) + a0 b1 <= (2^32 - 2) + (2^32 - 1)^2 = 2^64 - 2^32 - 1; t2 = (u32) t1 + a1 b0 <= (2^32 - 1) + (2^32 - 1)^2 =
    # 2^64 - 2^32; t3 = (t1 >> 32) + (t2 >> 32) + a1 b1 = floor(a b / 2^64) < 2^64
    "f64mul.mad.0": "0 + a0 b0 < 2^64",
    "f64mul.mad.1": "t1 <= 2^64 - 2^32 - 1",
    "f64mul.mad.2": "t2 <= 2^64 - 2^32",
    "f64mul.mad.3": "t3 = floor(a b / 2^64) < 2^64",
}
# The delta chain adds T_lo and m = -(T_lo + (t0 << 108)) (mod 2^128), so its sum is -(t0 << 108): limbs 0..2 of the sum are zero.
# A carry enters limb 1 exactly when t0 != 0, and then the borrow entered m1 too: m1 = 2^32 - 1 - t1, the limb sum t1 + m1 is 0xffffffff
# and the carry goes on.  A carry enters limb 2 exactly when (t0, t1) != 0, and m2 = 2^32 - 1 - t2 alike.  A carry enters limb 3 exactly
# when (t0, t1, t2) != 0, m3 = 2^32 - 1 - u3, and t3 + m3 = -1 - k (mod 2^32) with k = (t0 << 12) mod 2^32: 0xffffffff exactly when k = 0.
# So delta = 1 exactly when u3 wrapped, or k = 0 and T_lo != 0.  With link 1, 2 or 3 dropped the sums 0xffffffff pass no carry on and
# delta comes out as [u3 wrapped]: wrong exactly when k = 0 and the link carried.  All three are mutants, on those pairs only
# (t0 a multiple of 2^20; mul.dl.ripple.3), and the miner keeps pairs that expose each.  The models assert the structure.
DELTA_STRUCTURE = "mul.dl.link.1 and .2 always meet a limb sum of 0xffffffff; .3 does exactly when (t0 << 12) mod 2^32 = 0"

# A link whose loss no operand pair below the modulus can show would be listed here with its proof (fp256's mul.fsub.6 was one).
# There is none: every chain here ends in the selection or in a limb of the result, and for each link there are pairs that reach it with
# the selection on the side that shows it.  The one place where that needed an argument is the delta chain (above).
EQUIVALENT = {}


def limbs4(a):
    return [(a >> (32 * i)) & M32 for i in range(4)]


def _int(w):
    return sum(x << (32 * k) for k, x in enumerate(w))


def _subp(x, hi, pre, drop, ev):
    """(hi : x) - p with v_subrev / v_subbrev / v_subb, selected (v_cndmask) when the final borrow is clear -> (limbs, taken)"""
    d, bo = [0] * 4, 0
    for i in range(4):
        if i and bo:
            ev.add("%s.link.%d" % (pre, i))
            if i < 3 and x[i] == 0:
                ev.add("%s.ripple.%d" % (pre, i))
            if drop == "%s.link.%d" % (pre, i):
                bo = 0
        t = x[i] - PW[i] - bo
        d[i], bo = t & M32, 1 if t < 0 else 0
    if bo:
        ev.add(pre + ".link.4")
        if drop == pre + ".link.4":
            bo = 0
    bo = 1 if hi - bo < 0 else 0  # v_subbrev_co_u32 c, vcc, 0, c, vcc
    return (x if bo else d), not bo


def fp_add_model(a, b, drop=None, ev=None):
    """fp_add: the 4-limb add chain with its carry bit c, then (c : s) - p and the selection on the final borrow"""
    if ev is None:
        ev = set()
    x, y = limbs4(a), limbs4(b)
    c = 0
    for i in range(4):
        if i and c:
            ev.add("add.link.%d" % i)
            if (x[i] + y[i]) & M32 == M32:
                ev.add("add.ripple.%d" % i)
            if drop == "add.link.%d" % i:
                c = 0
        t = x[i] + y[i] + c
        x[i], c = t & M32, t >> 32
    if c:
        ev.add("add.link.4")
        if drop == "add.link.4":
            c = 0
    ev.add("add.c.1" if c else "add.c.0")
    if drop is None:
        if a + b == P:
            ev.add("add.sum.p")
        elif a + b == P - 1:
            ev.add("add.sum.pm1")
    r, taken = _subp(x, c, "add.subp", drop, ev)
    ev.add("add.sel.taken" if taken else "add.sel.not")
    return _int(r)


def fp_sub_model(a, b, drop=None, ev=None):
    """fp_sub: the 4-limb subtract chain, e0 = borrow ? 1 : 0 and e3 = borrow ? 0xfffff000 : 0 added back with zeros between"""
    if ev is None:
        ev = set()
    x, y = limbs4(a), limbs4(b)
    if a == b:
        ev.add("sub.eq")
    bo = 0
    for i in range(4):
        if i and bo:
            ev.add("sub.link.%d" % i)
            if x[i] == y[i]:
                ev.add("sub.ripple.%d" % i)
            if drop == "sub.link.%d" % i:
                bo = 0
        t = x[i] - y[i] - bo
        x[i], bo = t & M32, 1 if t < 0 else 0
    if bo:
        ev.add("sub.link.4")
        if drop == "sub.link.4":
            bo = 0
    ev.add("sub.m.1" if bo else "sub.m.0")
    c = 0
    for i, add in enumerate((bo, 0, 0, PW[3] if bo else 0)):
        if i and c:
            ev.add("sub.addp.link.%d" % i)
            if i < 3 and x[i] == M32:
                ev.add("sub.addp.ripple.%d" % i)
            if drop == "sub.addp.link.%d" % i:
                c = 0
        t = x[i] + add + c
        x[i], c = t & M32, t >> 32
    return _int(x)


def fp_mul_model(a, b, drop=None, ev=None):
    """fp_mul -> a b / 2^128 mod p as the device forms it with the one-step REDC (the branch without LF_FP_REDC2)"""
    if ev is None:
        ev = set()
    strict = drop is None
    x, y = limbs4(a), limbs4(b)
    t = []
    acc = ov = 0
    for k, col in enumerate(COLUMNS):
        for ij in col:
            s = acc + x[ij[0]] * y[ij[1]]  # v_mad_u64_u32
            acc = s & M64
            if s >> 64:
                name = _PC[ij]
                assert not (strict and name in UNREACHABLE), (name, hex(a), hex(b))
                ev.add(name)
                if ij not in UNCAPTURED and name != drop:
                    ov += 1  # FP_MADC's v_addc_co_u32 ov, vcc, 0, ov, vcc
        if k < 6:
            t.append(acc & M32)  # FP_COL
            acc = (acc >> 32) | (ov << 32)
            ov = 0
        else:
            t += [acc & M32, (acc >> 32) & M32]
    if strict:
        assert _int(t) == a * b, (hex(a), hex(b))
    k12 = (t[0] << 12) & M32
    u3 = t[3] + k12
    ev.add("mul.u3.wrap" if u3 >> 32 else "mul.u3.not")
    u3 &= M32
    if not any(t[:4]):
        ev.add("mul.tlo.zero")
    # m = 0 - (t0, t1, t2, u3): v_sub_co, v_subb_co x 3
    m, bo = [0] * 4, 0
    for i, sub in enumerate((t[0], t[1], t[2], u3)):
        if i and bo:
            ev.add("mul.m.link.%d" % i)
            if i < 3 and sub == 0:
                ev.add("mul.m.ripple.%d" % i)
            if drop == "mul.m.link.%d" % i:
                bo = 0
        v = 0 - sub - bo
        m[i], bo = v & M32, 1 if v < 0 else 0
    s = limbs4(_int(m) >> 20)  # three v_alignbit_b32 and a shift
    # q = m - s
    q, bo = [0] * 4, 0
    for i in range(4):
        if i and bo:
            ev.add("mul.q.link.%d" % i)
            if i < 3 and m[i] == s[i]:
                ev.add("mul.q.ripple.%d" % i)
            if drop == "mul.q.link.%d" % i:
                bo = 0
        v = m[i] - s[i] - bo
        q[i], bo = v & M32, 1 if v < 0 else 0
    if bo:
        assert not strict, ("mul.q.link.4", hex(a), hex(b))
        ev.add("mul.q.link.4")
    # delta = the carry out of T_lo + m (t3 itself here, not u3)
    c = 0
    for i in range(4):
        if i and c:
            ev.add("mul.dl.link.%d" % i)
            full = (t[i] + m[i]) & M32 == M32
            if strict:
                assert full == (i < 3 or k12 == 0), (DELTA_STRUCTURE, hex(a), hex(b))
            if i == 3 and full:
                ev.add("mul.dl.ripple.3")
            if drop == "mul.dl.link.%d" % i:
                c = 0
        v = t[i] + m[i] + c
        c = v >> 32
    if strict:
        assert c == (1 if (t[3] + k12) >> 32 or (k12 == 0 and any(t[:4])) else 0), (DELTA_STRUCTURE, hex(a), hex(b))
    ev.add("mul.delta.1" if c else "mul.delta.0")
    if drop == "mul.delta":
        c = 0
    # (t8 : t7 .. t4) = T_hi + q + delta
    h = t[4:8]
    for i in range(4):
        if i and c:
            ev.add("mul.hi.link.%d" % i)
            if (h[i] + q[i]) & M32 == M32:
                ev.add("mul.hi.ripple.%d" % i)
            if drop == "mul.hi.link.%d" % i:
                c = 0
        v = h[i] + q[i] + c
        h[i], c = v & M32, v >> 32
    if c:
        ev.add("mul.hi.link.4")
        if drop == "mul.hi.link.4":
            c = 0
    t8 = c
    ev.add("mul.t8.1" if t8 else "mul.t8.0")
    if strict:
        v = _int(h) + (t8 << 128)
        assert v == (a * b + _int(m) * P) >> 128 and v < 2 * P, (hex(a), hex(b), hex(v))
        assert v != P, ("mul.v.p", hex(a), hex(b))
        ev.add("mul.v.ge_p" if v >= P else "mul.v.lt_p")
    r, taken = _subp(h, t8, "mul.subp", drop, ev)
    ev.add("mul.sel.taken" if taken else "mul.sel.not")
    return _int(r)


def _f64_sub_chain(a0, a1, b0, b1, pre, drop, ev):
    """f64_sub's asm statement on limbs: d = a - b, m = borrow ? -1 : 0, d0 -= m, d1 -= borrow of that"""
    bo = 1 if a0 < b0 else 0
    d0 = (a0 - b0) & M32
    if bo:
        ev.add(pre + ".link.1")
        if a1 == b1:
            ev.add(pre + ".ripple.1")
        if drop == pre + ".link.1":
            bo = 0
    v = a1 - b1 - bo
    d1, bo = v & M32, 1 if v < 0 else 0
    ev.add(pre + (".m.1" if bo else ".m.0"))
    if drop == pre + ".m":
        bo = 0
    m = M32 if bo else 0  # v_cndmask_b32 m, 0, -1, vcc
    bo = 1 if d0 < m else 0  # v_sub_co_u32 d0, vcc, d0, m
    d0 = (d0 - m) & M32
    if m:
        ev.add(pre + (".fix.1" if bo else ".fix.0"))
        if drop == pre + ".fix":
            bo = 0
        elif drop == pre + ".fix.always":
            bo = 1
    d1 = (d1 - bo) & M32  # v_subbrev_co_u32 d1, vcc, 0, d1, vcc
    return d0 | (d1 << 32)


def f64_sub_model(a, b, drop=None, ev=None):
    if ev is None:
        ev = set()
    if a == b:
        ev.add("f64sub.eq")
    return _f64_sub_chain(a & M32, a >> 32, b & M32, b >> 32, "f64sub", drop, ev)


def f64_add_model(a, b, drop=None, ev=None):
    """f64_add: n = p - b = (1 - b0, 0xffffffff - b1 - borrow), in (0, p], then f64_sub's chain on (a, n)"""
    if ev is None:
        ev = set()
    b0, b1 = b & M32, b >> 32
    bo = 1 if b0 > 1 else 0
    n0 = (1 - b0) & M32
    if bo:
        ev.add("f64add.nb.link.1")
        if drop == "f64add.nb.link.1":
            bo = 0
    else:
        ev.add("f64add.nb.nolink")
    v = M32 - b1 - bo
    if v < 0:
        assert drop is not None, ("f64add.nb.link.2", hex(b))
        ev.add("f64add.nb.link.2")
    n1 = v & M32
    if drop is None:
        if b == 0:
            ev.add("f64add.b.zero")
        if a + b == P64:
            ev.add("f64add.sum.p")
    return _f64_sub_chain(a & M32, a >> 32, n0, n1, "f64add.sub", drop, ev)


def f64_mul_model(a, b, drop=None, ev=None):
    """f64_mul: four v_mad_u64_u32 re-combined into (l0, l1, h0, h1), then the shift-only reduction and f64_sub's fix-up"""
    if ev is None:
        ev = set()
    strict = drop is None
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32

    def mad(k, acc, x, y):
        s = acc + x * y
        if s >> 64:
            assert not strict, ("f64mul.mad.%d" % k, hex(a), hex(b))
            ev.add("f64mul.mad.%d" % k)
        return s & M64

    t0 = mad(0, 0, a0, b0)
    t1 = mad(1, t0 >> 32, a0, b1)
    t2 = mad(2, t1 & M32, a1, b0)
    t3 = mad(3, (t1 >> 32) + (t2 >> 32), a1, b1)
    l0, l1, h0, h1 = t0 & M32, t2 & M32, t3 & M32, t3 >> 32
    if strict:
        assert l0 | (l1 << 32) | (t3 << 64) == a * b
    x = l1 + l0  # v_add_co_u32 x, vcc, l1, l0
    e, x = x >> 32, x & M32
    ev.add("f64mul.e.1" if e else "f64mul.e.0")
    if drop == "f64mul.e":
        e = 0
    v = l0 - x - e  # v_subb_co_u32 y, vcc, l0, x, vcc
    y, bo = v & M32, 1 if v < 0 else 0
    ev.add("f64mul.yb.1" if bo else "f64mul.yb.0")
    if drop == "f64mul.yb":
        bo = 0
    v = x - bo  # v_subbrev_co_u32 x, vcc, 0, x, vcc
    if v < 0:
        assert not strict, ("f64mul.xb", hex(a), hex(b))
        ev.add("f64mul.xb")
    x = v & M32
    bo = 1 if h0 < y else 0  # r = hi - (y, x)
    r0 = (h0 - y) & M32
    if bo:
        ev.add("f64mul.hb.link.1")
        if h1 == x:
            ev.add("f64mul.hb.ripple.1")
        if drop == "f64mul.hb.link.1":
            bo = 0
    v = h1 - x - bo
    r1, bo = v & M32, 1 if v < 0 else 0
    ev.add("f64mul.neg.1" if bo else "f64mul.neg.0")
    if drop == "f64mul.neg":
        bo = 0
    z = M32 if bo else 0
    bo = 1 if r0 < z else 0
    r0 = (r0 - z) & M32
    if z:
        ev.add("f64mul.fix.1" if bo else "f64mul.fix.0")
        if drop == "f64mul.fix":
            bo = 0
        elif drop == "f64mul.fix.always":
            bo = 1
    r1 = (r1 - bo) & M32
    return r0 | (r1 << 32)


def f64x2_mul_events(a, b, ev=None):
    """f64x2_mul is three base-field products, two adds and three subs (fields.h): -> ((re, im), the base-field events they reach)"""
    if ev is None:
        ev = set()
    p0, p1 = f64_mul_model(a[0], b[0], ev=ev), f64_mul_model(a[1], b[1], ev=ev)
    x = f64_mul_model(f64_add_model(a[0], a[1], ev=ev), f64_add_model(b[0], b[1], ev=ev), ev=ev)
    return (f64_sub_model(p0, p1, ev=ev), f64_sub_model(f64_sub_model(x, p0, ev=ev), p1, ev=ev)), ev


def f64x2_mul_real_events(a, y, ev=None):
    if ev is None:
        ev = set()
    return (f64_mul_model(a[0], y, ev=ev), f64_mul_model(a[1], y, ev=ev)), ev


FIELDS = {"fp128": ("add", "sub", "mul"), "f64": ("f64add", "f64sub", "f64mul")}
MODULUS = {"fp128": P, "f64": P64}
MODELS = {"add": fp_add_model, "sub": fp_sub_model, "mul": fp_mul_model, "f64add": f64_add_model, "f64sub": f64_sub_model, "f64mul": f64_mul_model}
EXACT = {"add": lambda a, b: (a + b) % P, "sub": lambda a, b: (a - b) % P, "mul": lambda a, b: a * b * R_INV % P,
         "f64add": lambda a, b: (a + b) % P64, "f64sub": lambda a, b: (a - b) % P64, "f64mul": lambda a, b: a * b * R64_INV % P64}


def _names(fmt, ks):
    return [fmt % k for k in ks]


def _f64chain(pre):
    return [pre + s for s in (".link.1", ".ripple.1", ".m.0", ".m.1", ".fix.0", ".fix.1")]


# ---- the events a committed set has to reach, and the links whose loss it has to notice
EVENTS = {
    "add": sorted(_names("add.link.%d", (1, 2, 3, 4)) + _names("add.ripple.%d", (1, 2, 3)) + _names("add.subp.link.%d", (1, 2, 3, 4))
                  + _names("add.subp.ripple.%d", (1, 2)) + ["add.c.0", "add.c.1", "add.sel.taken", "add.sel.not", "add.sum.p", "add.sum.pm1"]),
    "sub": sorted(_names("sub.link.%d", (1, 2, 3, 4)) + _names("sub.ripple.%d", (1, 2, 3)) + _names("sub.addp.link.%d", (1, 2, 3))
                  + _names("sub.addp.ripple.%d", (1, 2)) + ["sub.m.0", "sub.m.1", "sub.eq"]),
    "mul": sorted([n for n in _PC.values() if n not in UNREACHABLE] + ["mul.u3.wrap", "mul.u3.not", "mul.tlo.zero"]
                  + _names("mul.m.link.%d", (1, 2, 3)) + _names("mul.m.ripple.%d", (1, 2)) + _names("mul.q.link.%d", (1, 2, 3))
                  + _names("mul.q.ripple.%d", (1, 2)) + _names("mul.dl.link.%d", (1, 2, 3)) + ["mul.dl.ripple.3", "mul.delta.0", "mul.delta.1"]
                  + _names("mul.hi.link.%d", (1, 2, 3, 4)) + _names("mul.hi.ripple.%d", (1, 2, 3)) + ["mul.t8.0", "mul.t8.1"]
                  + _names("mul.subp.link.%d", (1, 2, 3, 4)) + _names("mul.subp.ripple.%d", (1, 2))
                  + ["mul.sel.taken", "mul.sel.not", "mul.v.ge_p", "mul.v.lt_p"]),
    "f64sub": sorted(_f64chain("f64sub") + ["f64sub.eq"]),
    "f64add": sorted(_f64chain("f64add.sub") + ["f64add.nb.link.1", "f64add.nb.nolink", "f64add.b.zero", "f64add.sum.p"]),
    "f64mul": sorted(["f64mul.e.0", "f64mul.e.1", "f64mul.yb.0", "f64mul.yb.1", "f64mul.hb.link.1", "f64mul.hb.ripple.1", "f64mul.neg.0",
                      "f64mul.neg.1", "f64mul.fix.0", "f64mul.fix.1"]),
}
DROPS = {
    "add": sorted(_names("add.link.%d", (1, 2, 3, 4)) + _names("add.subp.link.%d", (1, 2, 3, 4))),
    "sub": sorted(_names("sub.link.%d", (1, 2, 3, 4)) + _names("sub.addp.link.%d", (1, 2, 3))),
    "mul": sorted([n for n in _PC.values() if n not in UNREACHABLE] + _names("mul.m.link.%d", (1, 2, 3)) + _names("mul.q.link.%d", (1, 2, 3))
                  + _names("mul.dl.link.%d", (1, 2, 3)) + ["mul.delta"] + _names("mul.hi.link.%d", (1, 2, 3, 4))
                  + _names("mul.subp.link.%d", (1, 2, 3, 4))),
    "f64sub": ["f64sub.fix", "f64sub.fix.always", "f64sub.link.1", "f64sub.m"],
    "f64add": ["f64add.nb.link.1", "f64add.sub.fix", "f64add.sub.fix.always", "f64add.sub.link.1", "f64add.sub.m"],
    "f64mul": ["f64mul.e", "f64mul.fix", "f64mul.fix.always", "f64mul.hb.link.1", "f64mul.neg", "f64mul.yb"],
}
# drop name -> the event whose pairs can show it (a dropped link changes nothing for a pair that does not reach it)
EVENT_OF = {d: d for op in DROPS for d in DROPS[op]}
EVENT_OF.update({"mul.delta": "mul.delta.1", "f64mul.e": "f64mul.e.1", "f64mul.yb": "f64mul.yb.1", "f64mul.neg": "f64mul.neg.1"})
for _pre in ("f64sub", "f64add.sub", "f64mul"):
    EVENT_OF.update({_pre + ".fix": _pre + ".fix.1", _pre + ".fix.always": _pre + ".fix.0"})
    if _pre != "f64mul":
        EVENT_OF[_pre + ".m"] = _pre + ".m.1"
DROPS_AT = {}
for _d, _e in EVENT_OF.items():
    DROPS_AT.setdefault(_e, []).append(_d)
OP_OF = {d: op for op in DROPS for d in DROPS[op]}


def first_accumulate_max(k):
    """The largest true value of column k's first accumulate, acc + a_i b_j with acc = floor(sum of the columns below / 2^(32 k)), over
    a, b < p.  It does not decrease when a limb grows, and [0, p) is two boxes of limb ranges, p = {1, 0, 0, 0xfffff000}: a3 < 0xfffff000,
    or a3 = 0xfffff000 and a2 = a1 = a0 = 0.  So it is largest at a top corner: 4 evaluations.  That accumulate carries for some
    a, b < p exactly when this reaches 2^64.  (Only a column's first accumulate is monotone like this.)"""
    i, j = COLUMNS[k][0]
    corners = ((M32, M32, M32, 0xFFFFEFFF), (0, 0, 0, 0xFFFFF000))
    best = 0
    for x in corners:
        for y in corners:
            below = sum(x[u] * y[v] << (32 * (u + v)) for u in range(4) for v in range(4) if u + v < k)
            best = max(best, (below >> (32 * k)) + x[i] * y[j])
    return best


# ---- the edge lists of the tests that were there before (test_gpu_parity.py::test_field_binops, test_device_arith_on_host.py)
def _e(lo, hi):
    return lo | (hi << 64)


FP_EDGES = [_e(*v) for v in ([0, 0], [1, 0], [0, 0xFFFFF00000000000], [0xFFFFFFFFFFFFFFFF, 0xFFFFEFFFFFFFFFFF], [0xFFFFFFFFFFFFFFFF, 0], [0, 1],
                             [0, 0xFFFFF00000000000 - 1], [0xFFFFFFFF, 0], [0x100000000, 0], [0, 0xFFFFEFFF00000000], [1 << 20, 0], [(1 << 20) - 1, 0],
                             [0xFFFFF, 0xFFFFFFFF00000000], [0, 1 << 44], [0xFFF00000, 0xFFF0000000000000])]
GF_EDGES = FP_EDGES + [_e(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF), _e(0, 0x8000000000000000)]
F64_EDGES = [0, 1, 2, 0xFFFFFFFF, 1 << 32, (1 << 32) + 1, P64 - 1, P64 - 2, (P64 - 1) // 2, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001,
             0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0x00000000FFFFFFFE]
# (one of the Fp128 list, hi = 0xffffffff00000000, is no field element: the models and the device tests here take canonical operands only)
EDGES = {"fp128": [v for v in FP_EDGES if v < P], "f64": F64_EDGES}

# ---- GF(2^128): no carries, so no model; a plain reference, the records and what they have to meet
GF_WORDS = (0, 0xFFFFFFFF, 0x11111111, 0x22222222, 0x44444444, 0x88888888, 0x55555555, 0xAAAAAAAA, 1, 0x80000000, None)  # None: a random word
CLMUL_MASKS = (0x11111111, 0x22222222, 0x44444444, 0x88888888)


def clmul(x, y):
    """the carry-less product of two non-negative integers"""
    r = 0
    while y:
        low = y & -y
        r ^= x * low
        y ^= low
    return r


def gf_fold(t):
    """a carry-less product below 2^256 modulo x^128 + x^7 + x^2 + x + 1"""
    for _ in range(2):
        h = t >> 128
        t = (t & (2**128 - 1)) ^ h ^ (h << 1) ^ (h << 2) ^ (h << 7)
    assert t >> 128 == 0
    return t


def gf_mul_exact(a, b):
    return gf_fold(clmul(a, b))


def gf_records(seed=20261021):
    """-> [(a, b)]: every word of GF_WORDS in each of the four 32-bit positions of a against every word in that position of b (the other
    positions random); all words 0 or 0xffffffff, a against b; the squared edge list; every word from GF_WORDS"""
    rng = random.Random(seed)

    def word(w):
        return rng.getrandbits(32) if w is None else w

    def put(v, pos, w):
        return (v & ~(M32 << (32 * pos))) | (word(w) << (32 * pos))

    rec = [(put(rng.getrandbits(128), pos, wa), put(rng.getrandbits(128), pos, wb)) for pos in range(4) for wa in GF_WORDS for wb in GF_WORDS]
    ones = [sum(M32 << (32 * k) for k in range(4) if (i >> k) & 1) for i in range(16)]
    rec += [(a, b) for a in ones for b in ones]
    rec += [(a, b) for a in GF_EDGES for b in GF_EDGES]
    rec += [(sum(word(rng.choice(GF_WORDS)) << (32 * k) for k in range(4)), sum(word(rng.choice(GF_WORDS)) << (32 * k) for k in range(4))) for _ in range(500)]
    return rec


def gf_clmul32_calls(a, b):
    """the nine (x, y) that gf_mul hands to clmul32, as (clmul64 call, clmul32 call within it, x, y): Karatsuba over 64-bit halves, then
    over 32-bit halves, the middle terms on the XORs of the halves"""
    out = []
    for i, (x, y) in enumerate(((a & M64, b & M64), (a >> 64, b >> 64), ((a & M64) ^ (a >> 64), (b & M64) ^ (b >> 64)))):
        xl, xh, yl, yh = x & M32, x >> 32, y & M32, y >> 32
        out += [(i, 0, xl, yl), (i, 1, xh, yh), (i, 2, xl ^ xh, yl ^ yh)]
    return out


def gf_fold_words(a, b):
    """-> (t3, t2) as gf_reduce256 shifts them: t3 the top word of the 256-bit product, t2 the word below after t3's fold into it"""
    t = clmul(a, b)
    t3 = t >> 192
    t2 = ((t >> 128) & M64) ^ (t3 >> 63) ^ (t3 >> 62) ^ (t3 >> 57)
    return t3, t2


# ---- the committed pairs: mined, seeded and deterministic
SPECIAL = (0, 1, 2, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF, 0xFFFFF000, 0xFFFFEFFF, 0xFFF, 0x1000, 0xFFFFF, 0x100000)
SPARSE = (0, 0, 1, M32 - 1, M32, M32)
KEEP = {"fp128": 16, "f64": 40}  # a pair is kept when it is among the first KEEP to reach an event (or to expose a dropped link)


def structured(rng, nl, bound, special=SPECIAL, p_special=0.85):
    """each 32-bit limb one of `special` with probability p_special, otherwise uniform; redrawn until below `bound`"""
    while True:
        v = 0
        for i in range(nl):
            v |= (rng.choice(special) if rng.random() < p_special else rng.getrandbits(32)) << (32 * i)
        if v < bound:
            return v


def events_of(field, a, b):
    ev = set()
    for op in FIELDS[field]:
        got = MODELS[op](a, b, ev=ev)
        assert got == EXACT[op](a, b), (op, hex(a), hex(b), hex(got))
    return ev


def related(rng, a, p, nl):
    """b next to a, -a and the limb boundaries: b = a, p - a, p - a +- 1, p - a +- 2^(32 k), a +- 1, a +- 2^(32 k)"""
    steps = [0, 1, -1] + [s << (32 * k) for k in range(1, nl) for s in (1, -1)]
    base = a if rng.random() < 0.4 else p - a
    return (base + rng.choice(steps)) % p


def hand_pairs(field):
    """what no draw finds by itself: the edge values against each other, a + b = p and p - 1, a = b"""
    p = MODULUS[field]
    e = EDGES[field]
    mid = [1, 2, p - 1, (p - 1) // 2, M32, 1 << 32, p >> 1] + ([1 << 96, (1 << 96) - 1, 1 << 64, M64, 0x7FFFFFFF_80000000_FFFFFFFE_00000001] if field == "fp128" else [])
    pairs = [(a, p - a) for a in mid] + [(a, p - 1 - a) for a in mid + [0]] + [(a, a) for a in mid + [0]]
    return pairs + [(a, b) for a in e for b in e]


def draw(field, rng, n):
    """The kinds of draw, taking turns:
      0  a and b both structured;
      1  a structured and b related to it (related());
      2  a structured and b chosen so that the Montgomery product is a structured r, or r = v mod p for a structured v below 2^128
         (2^64): the structure is on the value before the selection, which is r or r + p.  A zero limb of v is where a ripple of
         T_hi + q + delta (hi - (y, x) for F64) ends, and v with limbs 0..2 zero is where the subtract-p borrows run;
      3  the same with the limbs of r from {0, 1, 2^32 - 2, 2^32 - 1} only;
      4  sums and differences built directly: a + b = s (mod 2^128 or 2^64) for a sparse s, a - b = d for a sparse d;
      5  Fp128 only, on the REDC intermediate: q = m - (m >> 20) structured, m solved from it, T_lo = -m p (mod 2^128), b = 1 or an odd
         structured b, and a = T_lo / b (mod 2^128): m and q depend on T_lo alone."""
    p = MODULUS[field]
    nl = 4 if field == "fp128" else 2
    top = 1 << (32 * nl)
    r_one = top % p
    kind = n % (6 if field == "fp128" else 5)
    a = structured(rng, nl, p)
    if kind == 0:
        return a, structured(rng, nl, p)
    if kind == 1:
        return a, related(rng, a, p, nl)
    if kind in (2, 3):
        if a == 0:
            return a, structured(rng, nl, p)
        if kind == 3:
            r = structured(rng, nl, top, SPARSE, 1.0) % p
        else:
            r = structured(rng, nl, p) if rng.random() < 0.5 else structured(rng, nl, top) % p
        return a, r * r_one * pow(a, -1, p) % p
    if kind == 4:
        s = structured(rng, nl, top, SPARSE, 0.9)
        if rng.random() < 0.5:
            b = (s - a) % top if rng.random() < 0.5 else (s + top - a) % (2 * top)  # a + b = s or 2^128 + s
        else:
            b = (a - s) % top  # a - b = s (mod 2^128)
        return (a, b) if b < p else (a, structured(rng, nl, p))
    q = structured(rng, nl, top - (top >> 19))
    m = q
    for _ in range(8):
        m = q + (m >> 20)
    tlo = -m * P % top
    b = 1 if rng.random() < 0.3 else structured(rng, nl, p) | 1  # odd: a = T_lo / b (mod 2^128) exists
    a2 = tlo * pow(b, -1, top) % top
    return (a2, b) if a2 < p and b < p else (a, structured(rng, nl, p))


def mine(field, seed=20261021, draws=200000):
    """-> the kept pairs in the order found, and the counts per event and per exposed drop ("kill <drop>")"""
    rng = random.Random(seed)
    keep = KEEP[field]
    count, kept, seen = {}, [], set()

    def offer(a, b):
        if (a, b) in seen:
            return
        ev = events_of(field, a, b)
        for e in sorted(ev):
            for d in DROPS_AT.get(e, ()):
                if count.get("kill " + d, 0) < keep:
                    op = OP_OF[d]
                    if MODELS[op](a, b, drop=d) != EXACT[op](a, b):
                        ev.add("kill " + d)
        if any(count.get(e, 0) < keep for e in ev):
            kept.append((a, b))
            seen.add((a, b))
            for e in ev:
                count[e] = count.get(e, 0) + 1

    for a, b in hand_pairs(field):
        offer(a, b)
    for n in range(draws):
        offer(*draw(field, rng, n))
    return kept, count


def load_pairs(field):
    with open(PAIRS) as f:
        return [(int(a, 16), int(b, 16)) for a, b in json.load(f)[field]]


if __name__ == "__main__":
    out, counts = {}, {}
    for field in FIELDS:
        kept, counts[field] = mine(field)
        out[field] = sorted(kept)
    with open(PAIRS, "w") as f:
        f.write('{"what": "operand pairs (hex, both below the modulus) that reach the carry paths of the device Fp128 and F64 arithmetic; written by tests/fields_limb_model.py"')
        for field, width in (("fp128", 32), ("f64", 16)):
            f.write(',\n "%s": [\n' % field)
            f.write(",\n".join('  ["%0*x", "%0*x"]' % (width, a, width, b) for a, b in out[field]))
            f.write("\n ]")
        f.write("}\n")
    for field in FIELDS:
        print(field, len(out[field]), "pairs")
        for op in FIELDS[field]:
            for e in EVENTS[op]:
                print("%-22s %d" % (e, counts[field].get(e, 0)))
            for d in DROPS[op]:
                if counts[field].get("kill " + d, 0) < 4:
                    print("NOT EXPOSED", d, counts[field].get("kill " + d, 0))

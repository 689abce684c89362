"""Instrumented limb models of the device's Fp256Base arithmetic (csrc/fp256.h, the __HIP_DEVICE_COMPILE__ path): fp256_mul,
fp256_add and fp256_sub restated instruction chain by instruction chain on Python integers, 32-bit limbs that wrap as the
registers do.  Each model returns the result and the set of EVENTS the operand pair reached -- which carry and borrow links of
the chains carried a one, which way each selection went -- and takes `drop=`, the name of one link to leave out: the model of a
kernel with that one link wrong (a wrong vcc operand, a swapped %n, a carry read before it was written).

tests/golden/p256_carry_pairs.json is a set of operand pairs, mined by this module's __main__ (seeded, deterministic), that
reaches every reachable event several times; tests/test_p256_limb_model.py checks that, and that every dropped link changes the
result of at least one committed pair.  tests/test_p256_arith_paths_gpu.py feeds the same pairs to the instructions themselves.

Event names (also the `drop=` names where the event is a link that carried):
  mul.pc.I.J          the carry out of the 64-bit accumulate of x_I * y_J (the bit its SGPR pair captures)
  mul.sadd.S.K        a carry entering link K = 1..6 of step S's add chain (limb 2S+3+K); K = 2 is the `+0` link, limb 2S+5
  mul.ssub.S.K        a borrow entering link K = 1..2 of step S's subtract chain (limb 2S+7+K)
  mul.cc.S.0 / .1     the carry out of step S's add chain; drop name mul.cc.S
  mul.bb.S.0 / .1     the borrow out of step S's subtract chain; drop name mul.bb.S
  mul.fadd.K          a carry entering position K = 1..6 of the final add chain over T[10..16]
  mul.fsub.K          a borrow entering position K = 1..6 of the final subtract chain
  mul.t16.0 / .1      T[16] before p256_cond_sub
  mul.csub.taken / .not   the conditional subtraction with T[16] = 0
  add.link.K          a carry entering limb K = 1..7 of the add chain, K = 8: into the carry bit c
  add.ripple.K        ... with that limb's sum x_K + y_K = 0xffffffff (mod 2^32): the carry goes through
  add.c.0 / .1        the carry bit
  add.subp.link.K     a borrow entering limb K = 1..8 of the subtract-p chain (8: the carry bit's limb)
  add.subp.ripple.K   K = 3, 4, 5 (p's zero limbs): ... with that limb zero, the borrow goes through
  add.sel.taken / .not    the selection of (c : x) - p
  add.sum.p / .pm1    a + b = p (result 0), a + b = p - 1
  sub.link.K          a borrow entering limb K = 1..7 of the subtract chain, K = 8: into the mask m
  sub.ripple.K        ... with x_K = y_K: the borrow goes through
  sub.m.0 / .1        the borrow out
  sub.eq              a = b
  sub.addp.link.K     a carry entering limb K = 1..7 of the add-back chain
  sub.addp.ripple.K   K = 3, 4, 5: ... with that limb 0xffffffff, the carry goes through

Events that cannot occur for a, b < p are listed in UNREACHABLE with their bounds; the models assert that they never fire.

TEST INFRASTRUCTURE: nothing outside tests/ imports this module."""
import json
import os
import random

P = 2**256 - 2**224 + 2**192 + 2**96 - 1
M32 = 2**32 - 1
M64 = 2**64 - 1
R_INV = pow(2**256, -1, P)
PW = tuple((P >> (32 * i)) & M32 for i in range(8))  # {-1, -1, -1, 0, 0, 0, 1, -1}
PAIRS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p256_carry_pairs.json")

# the product scan's columns: (i, j) in the order the device issues them
COLUMNS = tuple(tuple((i, k - i) for i in range(max(0, k - 7), min(7, k) + 1)) for k in range(15))
_PC = {(i, j): "mul.pc.%d.%d" % (i, j) for col in COLUMNS for (i, j) in col}
_SADD = [[None] + ["mul.sadd.%d.%d" % (s, k) for k in range(1, 7)] for s in range(4)]
_SSUB = [[None] + ["mul.ssub.%d.%d" % (s, k) for k in range(1, 3)] for s in range(4)]
_CC = [("mul.cc.%d.0" % s, "mul.cc.%d.1" % s, "mul.cc.%d" % s) for s in range(4)]
_BB = [("mul.bb.%d.0" % s, "mul.bb.%d.1" % s, "mul.bb.%d" % s) for s in range(4)]
_FADD = [None] + ["mul.fadd.%d" % k for k in range(1, 7)]
_FSUB = [None] + ["mul.fsub.%d" % k for k in range(1, 7)]

# ---- what cannot happen for a, b < p (asserted in the models whenever no link is dropped)
UNREACHABLE = {
    # x0 y0 is the first accumulate: 0 + x0 y0 < 2^64.  The device does not capture it either (FP_MAD).
    "mul.pc.0.0": "acc = 0 before it",
    # column 1 comes in with acc = (x0 y0) >> 32 <= 2^32 - 2, and x0 y1 <= (2^32 - 1)^2: the sum is <= 2^64 - 2^32 - 1
    "mul.pc.0.1": "acc <= 2^32 - 2 before it, the product <= 2^64 - 2^33 + 1",
    # column 1's true sum is <= (2^32 - 2) + 2 (2^32 - 1)^2 = 2^65 - 3 2^32, so column 2 comes in with acc <= 2^33 - 3 and
    # x0 y2 <= 2^64 - 2^33 + 1 brings it to 2^64 - 2 at the most (tests/test_fp_tile_mul_carries.py has the same bound for Fp128)
    "mul.pc.0.2": "acc <= 2^33 - 3 before it, the product <= 2^64 - 2^33 + 1",
    # column 13's first accumulate: first_accumulate_max(13) = 2^64 - 2 (x7 = 2^32 - 1 forces x6 <= 1, and so for y)
    "mul.pc.6.7": "acc + x6 y7 <= 2^64 - 2 over the five boxes of [0, p): first_accumulate_max(13)",
    # the scan is exact: after the last accumulate (acc : carry) = floor(a b / 2^448) < 2^64 since a b < 2^512
    "mul.pc.7.7": "acc + x7 y7 = floor(a b / 2^448) < 2^64",
    # the value before p256_cond_sub is v = (a b + q p) / 2^256 < 2p, and v = p needs a b = 0 (mod p): a or b is zero, then T = 0, q = 0
    # and v = 0.  So the subtraction never yields zero from v = p; a zero result is always v = 0, not taken
    "mul.v.p": "v = p only if a b = 0 (mod p), and then v = 0",
}


def limbs(a):
    return [(a >> (32 * i)) & M32 for i in range(8)]


def _cond_sub(x, hi):
    """p256_cond_sub / the second half of fp256_add: (hi : x) - p, selected when the final borrow is clear"""
    d, bo = [0] * 8, 0
    for i in range(8):
        t = x[i] - PW[i] - bo
        d[i], bo = t & M32, 1 if t < 0 else 0
    bo = 1 if hi - bo < 0 else 0
    return x if bo else d, not bo


def mul_model(a, b, drop=None, ev=None):
    """fp256_mul -> a b / 2^256 mod p as the device forms it; ev (a set) collects the events"""
    if ev is None:
        ev = set()
    strict = drop is None
    x, y = limbs(a), limbs(b)
    T = [0] * 17
    acc = ov = 0
    for k, col in enumerate(COLUMNS):
        for ij in col:
            s = acc + x[ij[0]] * y[ij[1]]  # v_mad_u64_u32
            acc = s & M64
            if s >> 64:
                name = _PC[ij]
                assert not (strict and name in UNREACHABLE), (name, hex(a), hex(b))
                ev.add(name)
                if name != drop:
                    ov += 1  # v_addc_co_u32 ov, vcc, 0, ov, s[..]
        T[k] = acc & M32  # FP_COL
        acc = (acc >> 32) | (ov << 32)
        ov = 0
    T[15] = acc & M32
    assert not strict or acc >> 32 == 0
    cs, bs = [0] * 4, [0] * 4
    for s in range(4):
        i = 2 * s
        m0, m1 = T[i], T[i + 1]
        c = 0
        for k, add in enumerate((m0, m1, 0, m0, m1, m0, m1)):
            if k and c:
                ev.add(_SADD[s][k])
                if _SADD[s][k] == drop:
                    c = 0
            t = T[i + 3 + k] + add + c
            T[i + 3 + k], c = t & M32, t >> 32
        ev.add(_CC[s][c])
        cs[s] = 0 if _CC[s][2] == drop else c
        bo = 0
        for k, sub in enumerate((m0, m1, 0)):
            if k and bo:
                ev.add(_SSUB[s][k])
                if _SSUB[s][k] == drop:
                    bo = 0
            t = T[i + 7 + k] - sub - bo
            T[i + 7 + k], bo = t & M32, 1 if t < 0 else 0
        ev.add(_BB[s][bo])
        bs[s] = 0 if _BB[s][2] == drop else bo
    c = 0
    for k, add in enumerate((cs[0], 0, cs[1], 0, cs[2], 0, cs[3])):
        if k and c:
            ev.add(_FADD[k])
            if _FADD[k] == drop:
                c = 0
        t = T[10 + k] + add + c
        T[10 + k], c = t & M32, t >> 32
    bo = 0
    for k, sub in enumerate((bs[0], 0, bs[1], 0, bs[2], 0, bs[3])):
        if k and bo:
            ev.add(_FSUB[k])
            if _FSUB[k] == drop:
                bo = 0
        t = T[10 + k] - sub - bo
        T[10 + k], bo = t & M32, 1 if t < 0 else 0
    if strict:
        # the value is v = (T[16] : T[8..15]) = (a b + q p) / 2^256 with q < 2^256: 0 <= v < 2p, so T[16] is a bit and nothing
        # leaves the top of either final chain; v = p would need a b = 0 (mod p), and then T = 0 and v = 0
        v = sum(T[8 + k] << (32 * k) for k in range(9))
        assert c == 0 and bo == 0 and T[16] in (0, 1) and v < 2 * P, (hex(a), hex(b), hex(v))
        assert v != P, ("mul.v.p", hex(a), hex(b))
    ev.add("mul.t16.1" if T[16] else "mul.t16.0")
    r, taken = _cond_sub(T[8:16], T[16])
    if T[16] == 0:
        ev.add("mul.csub.taken" if taken else "mul.csub.not")
    elif strict:
        assert taken
    return sum(w << (32 * k) for k, w in enumerate(r))


_ADD_LINK = [None] + ["add.link.%d" % k for k in range(1, 9)]
_ADD_RIP = [None] + ["add.ripple.%d" % k for k in range(1, 8)]
_SUBP_LINK = [None] + ["add.subp.link.%d" % k for k in range(1, 9)]
_SUBP_RIP = {k: "add.subp.ripple.%d" % k for k in (3, 4, 5)}


def add_model(a, b, drop=None, ev=None):
    """fp256_add: the 8-limb add chain with its carry bit c, then (c : x) - p and the selection on the final borrow"""
    if ev is None:
        ev = set()
    x, y = limbs(a), limbs(b)
    c = 0
    for i in range(8):
        if i and c:
            ev.add(_ADD_LINK[i])
            if (x[i] + y[i]) & M32 == M32:
                ev.add(_ADD_RIP[i])
            if _ADD_LINK[i] == drop:
                c = 0
        t = x[i] + y[i] + c
        x[i], c = t & M32, t >> 32
    if c:
        ev.add(_ADD_LINK[8])
        if _ADD_LINK[8] == drop:
            c = 0
    ev.add("add.c.1" if c else "add.c.0")
    if drop is None:
        s = a + b
        if s == P:
            ev.add("add.sum.p")
        elif s == P - 1:
            ev.add("add.sum.pm1")
    d, bo = [0] * 8, 0
    for i in range(8):
        if i and bo:
            ev.add(_SUBP_LINK[i])
            if i in _SUBP_RIP and x[i] == 0:
                ev.add(_SUBP_RIP[i])
            if _SUBP_LINK[i] == drop:
                bo = 0
        t = x[i] - PW[i] - bo
        d[i], bo = t & M32, 1 if t < 0 else 0
    if bo:
        ev.add(_SUBP_LINK[8])
        if _SUBP_LINK[8] == drop:
            bo = 0
    bo = 1 if c - bo < 0 else 0  # v_subbrev_co_u32 c, vcc, 0, c, vcc
    ev.add("add.sel.not" if bo else "add.sel.taken")
    r = x if bo else d
    return sum(w << (32 * k) for k, w in enumerate(r))


_SUB_LINK = [None] + ["sub.link.%d" % k for k in range(1, 9)]
_SUB_RIP = [None] + ["sub.ripple.%d" % k for k in range(1, 8)]
_ADDP_LINK = [None] + ["sub.addp.link.%d" % k for k in range(1, 8)]
_ADDP_RIP = {k: "sub.addp.ripple.%d" % k for k in (3, 4, 5)}


def sub_model(a, b, drop=None, ev=None):
    """fp256_sub: the 8-limb subtract chain, the mask m of its borrow, then p & m added back"""
    if ev is None:
        ev = set()
    x, y = limbs(a), limbs(b)
    if a == b:
        ev.add("sub.eq")
    bo = 0
    for i in range(8):
        if i and bo:
            ev.add(_SUB_LINK[i])
            if x[i] == y[i]:
                ev.add(_SUB_RIP[i])
            if _SUB_LINK[i] == drop:
                bo = 0
        t = x[i] - y[i] - bo
        x[i], bo = t & M32, 1 if t < 0 else 0
    if bo:
        ev.add(_SUB_LINK[8])
        if _SUB_LINK[8] == drop:
            bo = 0
    ev.add("sub.m.1" if bo else "sub.m.0")
    m = M32 if bo else 0
    c = 0
    for i, add in enumerate((m, m, m, 0, 0, 0, m & 1, m)):
        if i and c:
            ev.add(_ADDP_LINK[i])
            if i in _ADDP_RIP and x[i] == M32:
                ev.add(_ADDP_RIP[i])
            if _ADDP_LINK[i] == drop:
                c = 0
        t = x[i] + add + c
        x[i], c = t & M32, t >> 32
    return sum(w << (32 * k) for k, w in enumerate(x))


MODELS = {"mul": mul_model, "add": add_model, "sub": sub_model}
EXACT = {"mul": lambda a, b: a * b * R_INV % P, "add": lambda a, b: (a + b) % P, "sub": lambda a, b: (a - b) % P}

# ---- the events a committed set has to reach, and the links whose loss it has to notice
EVENTS = {
    "mul": sorted(
        [n for n in _PC.values() if n not in UNREACHABLE] + [n for s in range(4) for n in _SADD[s][1:] + _SSUB[s][1:] + list(_CC[s][:2]) + list(_BB[s][:2])]
        + _FADD[1:] + _FSUB[1:] + ["mul.t16.0", "mul.t16.1", "mul.csub.taken", "mul.csub.not"]),
    "add": sorted(_ADD_LINK[1:] + _ADD_RIP[1:] + _SUBP_LINK[1:] + list(_SUBP_RIP.values())
                  + ["add.c.0", "add.c.1", "add.sel.taken", "add.sel.not", "add.sum.p", "add.sum.pm1"]),
    "sub": sorted(_SUB_LINK[1:] + _SUB_RIP[1:] + _ADDP_LINK[1:] + list(_ADDP_RIP.values()) + ["sub.m.0", "sub.m.1", "sub.eq"]),
}
DROPS = {
    "mul": sorted([n for n in _PC.values() if n not in UNREACHABLE] + [n for s in range(4) for n in _SADD[s][1:] + _SSUB[s][1:] + [_CC[s][2], _BB[s][2]]]
                  + _FADD[1:] + _FSUB[1:6]),
    "add": sorted(_ADD_LINK[1:] + _SUBP_LINK[1:]),
    "sub": sorted(_SUB_LINK[1:] + _ADDP_LINK[1:]),
}
# A link whose loss no a, b < p can show.  A borrow enters position 6 of the final subtract chain (T[16]) only out of T[15], which
# it entered too (nothing else is subtracted there) and left at 2^32 - 1, and it entered T[15] out of T[14], left at 2^32 - 2 or more:
# v >= 2^256 - 2^193 > p whether T[16] ends as 0 or, the borrow lost, as 1, and p256_cond_sub subtracts p from the same eight limbs
# either way.  The event is reachable and the committed set reaches it.
EQUIVALENT = {"mul.fsub.6": "the borrow into T[16] leaves (T[15] : T[14]) >= 2^64 - 2, so p is subtracted with T[16] = 0 or 1 alike"}


def _box_corners():
    """[0, p) is the union of five boxes of limb ranges, p = {M, M, M, 0, 0, 0, 1, M} (M = 2^32 - 1, low limb first): x7 < M;
    x7 = M and x6 = 0; x7 = M, x6 = 1, x5 = x4 = x3 = 0 and x2 < M, or x2 = M and x1 < M, or x2 = x1 = M and x0 < M.  -> the top
    corner of each"""
    M = M32
    return [sum(w << (32 * i) for i, w in enumerate(c)) for c in (
        (M, M, M, M, M, M, M, M - 1), (M, M, M, M, M, M, 0, M), (M, M, M - 1, 0, 0, 0, 1, M), (M, M - 1, M, 0, 0, 0, 1, M), (M - 1, M, M, 0, 0, 0, 1, M))]


def first_accumulate_max(k):
    """The largest true value of column k's first accumulate, acc + x_i y_j with acc = floor(sum of the columns below / 2^(32 k)),
    over a, b < p.  It does not decrease when a limb grows, so over a box of limb ranges it is largest at the top corner, and [0, p)
    is five boxes: 25 evaluations.  That accumulate carries for some a, b < p exactly when this reaches 2^64.  (Only a column's first
    accumulate is monotone like this: the later ones start from an accumulator that has wrapped.)"""
    i, j = COLUMNS[k][0]
    best = 0
    for a in _box_corners():
        x = limbs(a)
        for b in _box_corners():
            y = limbs(b)
            below = sum(x[u] * y[v] << (32 * (u + v)) for u in range(8) for v in range(8) if u + v < k)
            best = max(best, (below >> (32 * k)) + x[i] * y[j])
    return best


# ---- the committed pairs: mined, seeded and deterministic
SPECIAL = (0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
KEEP = 8  # a pair is kept when it is among the first KEEP to reach an event (or to expose a dropped link)
DROP_OF = {n: n for op in DROPS for n in DROPS[op] if not n.startswith(("mul.cc", "mul.bb"))}  # event -> the link to drop
DROP_OF.update({"mul.cc.%d.1" % s: "mul.cc.%d" % s for s in range(4)})
DROP_OF.update({"mul.bb.%d.1" % s: "mul.bb.%d" % s for s in range(4)})


def structured(rng, bound=P):
    """each 32-bit limb one of SPECIAL with probability 0.9, otherwise uniform; redrawn until below `bound`"""
    while True:
        v = 0
        for i in range(8):
            v |= (rng.choice(SPECIAL) if rng.random() < 0.9 else rng.getrandbits(32)) << (32 * i)
        if v < bound:
            return v


def sparse(rng):
    while True:
        a = sum(rng.choice((0, 1, M32 - 1, M32)) << (32 * i) for i in range(8))
        b = (rng.choice((0, 1, 0x80000000, M32 - 1, M32)) << 224) + (rng.choice((1, M32 - 1, M32)) << (32 * rng.randrange(7)))
        if a < P and b < P:
            return a, b


def events_of(a, b):
    ev = set()
    for op, model in MODELS.items():
        got = model(a, b, ev=ev)
        assert got == EXACT[op](a, b), (op, hex(a), hex(b), hex(got))
    return ev


def hand_pairs():
    """what no draw finds: a + b = p, a + b = p - 1, a = b, and the edge values against each other"""
    edge = [0, 1, 2, P - 1, P - 2, 2**255, 2**224, 2**192 - 1, 2**96, 2**96 - 1, (P - 1) // 2, M32, 2**64 - 1, 2**256 - 2**224]
    mid = [1, 2**96, 2**96 - 1, 2**224, (P - 1) // 2, 2**255, 2**192 - 1, 0x7FFFFFFF_80000000_FFFFFFFE_00000001_00000002_FFFFFFFF_00000000_7FFFFFFF]
    pairs = [(a, P - a) for a in mid] + [(a, P - 1 - a) for a in mid + [0]] + [(a, a) for a in mid + [0, P - 1]]
    return pairs + [(a, b) for a in edge for b in edge]


def mine(seed=20261021, draws=240000):
    """-> the kept pairs, in the order found.  Four kinds of draw take turns:
      0  a and b both structured;
      1  a structured and b chosen so that the product a b / 2^256 mod p is a structured r;
      2  the same with r = v mod p for a structured v < 2^256, which puts the structure on the value before p256_cond_sub;
      3  sparse(): every limb of a from {0, 1, 2^32 - 2, 2^32 - 1} and a b of at most two non-zero limbs.  Only this kind reaches the
         even positions of the final chains in useful numbers: a deferred bit bb[s] or cc[s] has to meet limbs of T that the steps
         left at exactly 0 or 2^32 - 1, which a b that mixes every limb of a into every column does not leave."""
    rng = random.Random(seed)
    count, kept = {}, []
    R = 2**256 % P

    def offer(a, b):
        if (a, b) in kept:
            return
        ev = events_of(a, b)
        for e in sorted(ev):
            d = DROP_OF.get(e)
            if d is not None and count.get("kill " + d, 0) < KEEP:
                op = d[:3]
                if MODELS[op](a, b, drop=d) != EXACT[op](a, b):
                    ev.add("kill " + d)
        if any(count.get(e, 0) < KEEP for e in ev):
            kept.append((a, b))
            for e in ev:
                count[e] = count.get(e, 0) + 1

    for a, b in hand_pairs():
        offer(a, b)
    for n in range(draws):
        if n % 4 == 3:
            a, b = sparse(rng)
        else:
            a = structured(rng)
            if n % 4 == 0 or a == 0:
                b = structured(rng)
            else:
                r = structured(rng) if n % 4 == 1 else structured(rng, 2**256) % P
                b = r * R * pow(a, -1, P) % P
        offer(a, b)
    return kept, count


def load_pairs():
    with open(PAIRS) as f:
        return [(int(a, 16), int(b, 16)) for a, b in json.load(f)["pairs"]]


if __name__ == "__main__":
    kept, count = mine()
    with open(PAIRS, "w") as f:
        f.write('{"what": "operand pairs (hex, both below p) that reach the carry paths of the device Fp256Base arithmetic; written by tests/p256_limb_model.py",\n "pairs": [\n')
        f.write(",\n".join('  ["%064x", "%064x"]' % ab for ab in kept))
        f.write("\n ]}\n")
    print(len(kept), "pairs")
    for op in EVENTS:
        for e in EVENTS[op]:
            print("%-22s %d" % (e, count.get(e, 0)))
    for op in DROPS:
        for d in DROPS[op]:
            if count.get("kill " + d, 0) < 4:
                print("NOT EXPOSED", d, count.get("kill " + d, 0))

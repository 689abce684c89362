"""The instrumented limb models of the device's Fp128 and F64 arithmetic (tests/fields_limb_model.py) over the committed operand pairs
(tests/golden/fields_carry_pairs.json): every model result equals Python-integer arithmetic, every reachable event of the carry and
borrow chains is reached by at least four distinct pairs, and every model with one link dropped gets at least one pair wrong -- so
a kernel with that link wrong would fail tests/test_fields_arith_paths_gpu.py, which runs the same pairs on the device.  The portable
*_c code of fields.h sees the same pairs through libhostfields.so, and the GF(2^128) records of the device test, where nothing carries,
are held to the conditions that make them worth running."""
import ctypes as C

import numpy as np
import pytest

import fields_limb_model as L
from oracle_lib import P as PTR

MIN_PAIRS = 4
FIELDS = list(L.FIELDS)


@pytest.fixture(scope="module")
def pairs():
    return {f: L.load_pairs(f) for f in FIELDS}


@pytest.fixture(scope="module")
def reached(pairs):
    """field -> event -> the distinct pairs that reach it; the models' results are compared on the way"""
    out = {}
    for f in FIELDS:
        out[f] = {}
        for ab in set(pairs[f]):
            for e in L.events_of(f, *ab):  # asserts model == exact for the three operations
                out[f].setdefault(e, []).append(ab)
    return out


@pytest.mark.parametrize("field", FIELDS)
def test_pairs_are_canonical_sorted_and_few(pairs, field):
    ps = pairs[field]
    assert 100 <= len(ps) <= 1000 and ps == sorted(set(ps))
    assert all(0 <= a < L.MODULUS[field] and 0 <= b < L.MODULUS[field] for a, b in ps)


@pytest.mark.parametrize("field", FIELDS)
def test_every_reachable_event_is_reached_four_times(reached, field):
    counts = {e: len(reached[field].get(e, ())) for op in L.FIELDS[field] for e in L.EVENTS[op]}
    for e in sorted(counts):
        print("%-22s %d" % (e, counts[e]))
    thin = {e: n for e, n in counts.items() if n < MIN_PAIRS}
    assert not thin, thin
    assert not set(reached[field]) - set(counts), "an event the lists do not name"
    assert not set(L.UNREACHABLE) & set(reached[field])


def test_models_equal_big_integers_on_edges_and_random_pairs():
    """the squared edge lists and 10^5 seeded uniform pairs per field; the UNREACHABLE assertions of the models hold on the way"""
    rng = np.random.default_rng(20261021)
    for f in FIELDS:
        p, nb = L.MODULUS[f], 16 if f == "fp128" else 8
        for a in L.EDGES[f]:
            for b in L.EDGES[f]:
                L.events_of(f, a, b)
        raw = rng.bytes(200000 * nb)
        for i in range(100000):
            L.events_of(f, int.from_bytes(raw[2 * i * nb:(2 * i + 1) * nb], "little") % p, int.from_bytes(raw[(2 * i + 1) * nb:(2 * i + 2) * nb], "little") % p)


def test_unreachable_product_carries_are_exactly_the_column_firsts():
    """a column's first accumulate carries for some a, b < p exactly when its largest true value reaches 2^64: none of the seven does
    (b3 <= 0xfffff000).  Every other product carry is reached by the committed pairs (above)."""
    firsts = {"mul.pc.%d.%d" % L.COLUMNS[k][0]: L.first_accumulate_max(k) for k in range(7)}
    assert {e for e, m in firsts.items() if m < 2**64} == {e for e in L.UNREACHABLE if e.startswith("mul.pc.")} == set(firsts)
    assert firsts["mul.pc.0.2"] == 2**64 - 2
    assert all(L._PC[ij] in L.UNREACHABLE for ij in L.UNCAPTURED)


def test_unreachable_events_fire_outside_the_field():
    """the bounds need operands below the modulus: with all limbs 2^32 - 1 column 3's first accumulate carries, p - b is negative for
    b = 2^64 - 1, and the models say so"""
    with pytest.raises(AssertionError, match="mul.pc.0.3"):
        L.fp_mul_model(2**128 - 1, 2**128 - 1)
    with pytest.raises(AssertionError, match="f64add.nb.link.2"):
        L.f64_add_model(0, 2**64 - 1)


@pytest.mark.parametrize("op", list(L.DROPS))
def test_every_dropped_link_is_noticed(op, reached):
    """the model with one link left out (or, .always, forced) must get a committed pair wrong; only pairs that reach the link can differ"""
    field = "fp128" if op in L.FIELDS["fp128"] else "f64"
    missed, noticed = [], []
    for d in L.DROPS[op]:
        if d in L.EQUIVALENT:
            continue
        n = sum(L.MODELS[op](a, b, drop=d) != L.EXACT[op](a, b) for a, b in reached[field].get(L.EVENT_OF[d], ()))
        (noticed if n else missed).append((d, n))
    print("noticed:", noticed, "proven non-mutants:", sorted(L.EQUIVALENT))
    assert not missed, missed


def test_equivalent_links_change_no_result(reached):
    """none is known for these chains (fields_limb_model.EQUIVALENT says why); one that is added has to hold here"""
    for d in L.EQUIVALENT:
        op = L.OP_OF[d]
        hit = reached["fp128" if op in L.FIELDS["fp128"] else "f64"][L.EVENT_OF[d]]
        assert len(hit) >= MIN_PAIRS and all(L.MODELS[op](a, b, drop=d) == L.EXACT[op](a, b) for a, b in hit)


def test_delta_links_show_exactly_where_t0_is_a_multiple_of_2_20(reached):
    """DELTA_STRUCTURE: a dropped link of the delta chain changes the product exactly on the pairs that reach it with
    (t0 << 12) mod 2^32 = 0, which is mul.dl.ripple.3 -- and the committed pairs hold such a pair for every link"""
    for k in (1, 2, 3):
        d = "mul.dl.link.%d" % k
        shown = 0
        for a, b in reached["fp128"][d]:
            k12 = ((a * b) << 12) & L.M32
            wrong = L.fp_mul_model(a, b, drop=d) != L.EXACT["mul"](a, b)
            assert wrong == (k12 == 0), (d, hex(a), hex(b))
            assert wrong == ((a, b) in reached["fp128"]["mul.dl.ripple.3"])
            shown += wrong
        assert shown >= MIN_PAIRS, (d, shown)


@pytest.mark.parametrize("field", FIELDS)
def test_generator_reproduces_the_committed_pairs(pairs, field):
    """seeded and deterministic: what the first draws of the generator keep is in the committed (sorted) list"""
    kept, _ = L.mine(field, draws=3000)
    assert len(kept) > 100 and set(kept) <= set(pairs[field])


# ---- the same pairs through the portable *_c code (the host compilation of fields.h)
def _words(v, n):
    return np.array([(v >> (64 * k)) & L.M64 for k in range(n)], dtype=np.uint64)


@pytest.fixture(scope="module")
def host():
    from test_device_arith_on_host import _lib
    return _lib()


def test_host_fp128_on_the_carry_pairs(host, pairs):
    out = np.zeros(2, dtype=np.uint64)
    for a, b in pairs["fp128"] + [(b, a) for a, b in pairs["fp128"]]:
        xa, xb = _words(a, 2), _words(b, 2)
        for op in L.FIELDS["fp128"]:
            getattr(host, "hf_fp_" + op)(PTR(xa), PTR(xb), PTR(out))
            assert int(out[0]) | (int(out[1]) << 64) == L.EXACT[op](a, b), (op, hex(a), hex(b))


def f64x2_records(ps):
    """neighbouring F64 pairs as (re, im): -> [((a_re, a_im), (b_re, b_im))]"""
    return [((ps[i][0], ps[i + 1][0]), (ps[i][1], ps[i + 1][1])) for i in range(len(ps) - 1)]


def f64x2_mul_exact(a, b):
    return (a[0] * b[0] - a[1] * b[1]) * L.R64_INV % L.P64, (a[0] * b[1] + a[1] * b[0]) * L.R64_INV % L.P64


def test_host_f64_and_f64x2_on_the_carry_pairs(host, pairs):
    ps = pairs["f64"] + [(b, a) for a, b in pairs["f64"]]
    A, B = np.array([a for a, _ in ps], dtype=np.uint64), np.array([b for _, b in ps], dtype=np.uint64)
    out = np.zeros_like(A)
    for op, fn in (("f64add", host.hf_f64_add_many), ("f64sub", host.hf_f64_sub_many), ("f64mul", host.hf_f64_mul_many)):
        fn(C.c_size_t(len(A)), PTR(A), PTR(B), PTR(out))
        assert [int(x) for x in out] == [L.EXACT[op](a, b) for a, b in ps], op
    o2 = np.zeros(2, dtype=np.uint64)
    ev, ev_real = set(), set()
    for a, b in f64x2_records(ps):
        want, _ = L.f64x2_mul_events(a, b, ev)
        assert want == f64x2_mul_exact(a, b)
        host.hf_f64x2_mul(PTR(_words(a[0] | (a[1] << 64), 2)), PTR(_words(b[0] | (b[1] << 64), 2)), PTR(o2))
        assert (int(o2[0]), int(o2[1])) == want, (a, b)
        want, _ = L.f64x2_mul_real_events(a, b[0], ev_real)
        assert want == (L.EXACT["f64mul"](a[0], b[0]), L.EXACT["f64mul"](a[1], b[0]))
        host.hf_f64x2_mul_real(PTR(_words(a[0] | (a[1] << 64), 2)), PTR(_words(b[0], 2)), PTR(o2))
        assert (int(o2[0]), int(o2[1])) == want, (a, b)
    # f64x2_mul and f64x2_mul_real are compositions: which base-field events their products, adds and subs reach on these records
    every = {e for op in L.FIELDS["f64"] for e in L.EVENTS[op]}
    print("f64x2_mul reaches %d of %d base-field events; not: %s" % (len(ev & every), len(every), sorted(every - ev)))
    print("f64x2_mul_real reaches", sorted(ev_real))
    assert {e for e in every if e.startswith("f64mul.")} <= ev and {e for e in every if e.startswith("f64mul.")} <= ev_real


def test_host_gf_mul_on_the_records(host):
    out = np.zeros(2, dtype=np.uint64)
    for a, b in L.gf_records():
        host.hf_gf_mul(PTR(_words(a, 2)), PTR(_words(b, 2)), PTR(out))
        assert int(out[0]) | (int(out[1]) << 64) == L.gf_mul_exact(a, b), (hex(a), hex(b))


# ---- GF(2^128): what the records have to meet, as predicates on the inputs
def test_gf_reference_is_the_field():
    one, x = 1, 2
    assert L.gf_mul_exact(1 << 127, x) == 0x87 and L.gf_mul_exact(one, 0x1234) == 0x1234
    rng = np.random.default_rng(1)
    a, b, c = (int.from_bytes(rng.bytes(16), "little") for _ in range(3))
    assert L.gf_mul_exact(a, b) == L.gf_mul_exact(b, a)
    assert L.gf_mul_exact(L.gf_mul_exact(a, b), c) == L.gf_mul_exact(a, L.gf_mul_exact(b, c))
    assert L.gf_mul_exact(a, b ^ c) == L.gf_mul_exact(a, b) ^ L.gf_mul_exact(a, c)


def test_gf_records_put_every_word_in_every_position():
    rec = L.gf_records()
    assert rec == L.gf_records() and len(rec) < 2000
    fixed = [w for w in L.GF_WORDS if w is not None]
    assert set(fixed) == {0, 0xFFFFFFFF, 1, 0x80000000, 0x55555555, 0xAAAAAAAA} | {0x11111111 << k for k in range(4)}
    for side in (0, 1):
        for pos in range(4):
            seen = {(r[side] >> (32 * pos)) & L.M32 for r in rec}
            assert set(fixed) <= seen and len(seen - set(fixed)) > 100, (side, pos)  # and random words


def test_gf_records_fill_the_holes_of_every_clmul32():
    """clmul32 multiplies x & m_i by y & m_j as integers: 8 bits a side at the most, so at most 8 partial products meet in a 4-bit hole.
    Each of the nine clmul32 calls of gf_mul (three per clmul64, the Karatsuba middle terms xl ^ xh included) meets every (i, j) with 8
    set bits on both sides, and the product 0x11111111^2 has the digit 8 in the middle: the hole count the 4 bits have to hold."""
    full = set()
    for a, b in L.gf_records():
        for c64, c32, x, y in L.gf_clmul32_calls(a, b):
            for i, mi in enumerate(L.CLMUL_MASKS):
                for j, mj in enumerate(L.CLMUL_MASKS):
                    if x & mi == mi and y & mj == mj:
                        full.add((c64, c32, i, j))
    assert len(full) == 9 * 16
    assert max((0x11111111 * 0x11111111 >> (4 * k)) & 15 for k in range(16)) == 8


def test_gf_records_reach_every_fold_shift():
    """gf_reduce256 folds t3 and then t2 with the shifts >> 57, >> 62, >> 63.  t3 >> 63 is zero for EVERY input: the product of two
    polynomials of degree <= 127 has degree <= 254, bit 62 of t3.  The other five meet non-zero values."""
    met = set()
    for a, b in L.gf_records():
        t3, t2 = L.gf_fold_words(a, b)
        assert t3 >> 63 == 0
        met |= {("t3", s) for s in (57, 62) if t3 >> s} | {("t2", s) for s in (57, 62, 63) if t2 >> s}
    assert met == {("t3", 57), ("t3", 62), ("t2", 57), ("t2", 62), ("t2", 63)}
    assert L.clmul(2**128 - 1, 2**128 - 1) >> 255 == 0

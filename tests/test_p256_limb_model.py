"""The instrumented limb models of the device's Fp256Base arithmetic (tests/p256_limb_model.py) over the committed operand pairs
(tests/golden/p256_carry_pairs.json): every model result equals Python-integer arithmetic, every reachable event of the carry and
borrow chains is reached by at least four distinct pairs, and every model with one link dropped gets at least one pair wrong -- so
a kernel with that link wrong would fail tests/test_p256_arith_paths_gpu.py, which runs the same pairs on the device."""
import pytest

import p256_limb_model as L

MIN_PAIRS = 4


@pytest.fixture(scope="module")
def pairs():
    return L.load_pairs()


@pytest.fixture(scope="module")
def reached(pairs):
    """event -> the distinct pairs that reach it; the models' results are compared on the way"""
    out = {}
    for ab in set(pairs):
        for e in L.events_of(*ab):  # asserts model == exact for the three operations
            out.setdefault(e, []).append(ab)
    return out


def test_pairs_are_canonical_and_few(pairs):
    assert 100 <= len(pairs) <= 1000 and len(set(pairs)) == len(pairs)
    assert all(0 <= a < L.P and 0 <= b < L.P for a, b in pairs)


def test_every_reachable_event_is_reached_four_times(reached):
    counts = {e: len(reached.get(e, ())) for op in L.EVENTS for e in L.EVENTS[op]}
    for e in sorted(counts):
        print("%-22s %d" % (e, counts[e]))
    thin = {e: n for e, n in counts.items() if n < MIN_PAIRS}
    assert not thin, thin
    assert not set(reached) - set(counts), "an event the lists do not name"
    assert not set(L.UNREACHABLE) & set(reached)


def test_unreachable_product_carries_are_exactly_the_bounded_ones():
    """a column's first accumulate carries for some a, b < p exactly when its largest true value reaches 2^64; every other product
    carry is reached by the committed pairs (above)"""
    firsts = {"mul.pc.%d.%d" % L.COLUMNS[k][0]: L.first_accumulate_max(k) for k in range(15)}
    assert {e for e, m in firsts.items() if m < 2**64} == {e for e in L.UNREACHABLE if e.startswith("mul.pc.")}
    assert firsts["mul.pc.6.7"] == 2**64 - 2 and firsts["mul.pc.0.2"] == 2**64 - 2


def test_unreachable_events_fire_outside_the_field():
    """the bounds need a, b < p: with all limbs 2^32 - 1 column 13's first accumulate carries and the model says so"""
    with pytest.raises(AssertionError, match="mul.pc.6.7"):
        L.mul_model(2**256 - 1, 2**256 - 1)


@pytest.mark.parametrize("op", list(L.DROPS))
def test_every_dropped_link_is_noticed(op, reached):
    """the model with one link left out must get a committed pair wrong; only pairs that reach the link can differ"""
    missed = []
    for d in L.DROPS[op]:
        ev = d + ".1" if d.startswith(("mul.cc", "mul.bb")) else d
        if not any(L.MODELS[op](a, b, drop=d) != L.EXACT[op](a, b) for a, b in reached.get(ev, ())):
            missed.append(d)
    assert not missed, missed


def test_the_equivalent_link_changes_no_result(reached):
    for d in L.EQUIVALENT:
        assert len(reached[d]) >= MIN_PAIRS
        assert all(L.mul_model(a, b, drop=d) == L.EXACT["mul"](a, b) for a, b in reached[d])


def test_generator_reproduces_the_committed_pairs(pairs):
    """seeded and deterministic: the first draws of the generator give the first committed pairs"""
    kept, _ = L.mine(draws=2000)
    assert len(kept) > 100 and kept == pairs[:len(kept)]

"""The integer model of the product's even/odd accumulation (carry_patterns.py) and the fixed operand list that the device test of
the bit-sliced three-event carry counter runs (test_gpu_carry_counters.py)."""
import random

import pytest

import carry_patterns as cp
import field_cases as fc

P = cp.P


def test_the_fixed_pairs_are_canonical_and_reach_all_eight_patterns():
    assert sorted(cp.PAIRS) == sorted(cp.PATTERNS) and len(cp.PATTERNS) == 8
    for want, pairs in cp.PAIRS.items():
        assert len(pairs) == 2 and pairs[0] != pairs[1]
        for a, b in pairs:
            assert 0 <= a < P and 0 <= b < P
            assert cp.pattern(a, b) == want, (want, hex(a), hex(b))
    assert [p for p, _, _ in cp.all_pairs()] == cp.PATTERNS * 2


def test_the_fixed_pairs_raise_no_top_limb_flag():
    """so the flag forms (sc_field_selftest2 ops 4 and 5) return the exact product on every one of them"""
    for _, a, b in cp.all_pairs():
        assert fc.model("mul", a, b)[0] == 0


def test_counter_is_the_sum_of_its_bit_planes():
    for c1, c2, c3 in cp.PATTERNS:
        ones, twos = c1 ^ c2 ^ c3, (c1 & c2) | ((c1 ^ c2) & c3)
        assert 2 * twos + ones == c1 + c2 + c3


def _operands():
    rng = random.Random(77)
    pairs = [(a, b) for _, a, b in cp.all_pairs()]
    pairs += [(rng.randrange(1 << 128), rng.randrange(P)) for _ in range(2000)]       # first operands may be lazy: anything below 2^128
    A, B = fc.crossed_lists("mul")
    pairs += [(a, b) for a in A[::7] for b in B[::11]]
    return pairs


def test_accumulators_rebuild_the_product():
    """the model's accumulators and counters, merged as the device merges them, are the 256-bit product; counters stay in range"""
    for a, b in _operands():
        r = cp.accumulate(a, b)
        assert cp.merged(r) == a * b, (hex(a), hex(b))
        assert r["nO1"] == sum(r["pattern"]) <= 3 and r["nO0"] <= 1 and r["nE1"] <= 2 and r["nE2"] <= 2 and r["nO2"] <= 1


def test_a_seeded_search_finds_every_pattern():
    found = cp.search(per_pattern=1)
    assert all(len(found[p]) == 1 for p in cp.PATTERNS), {p: len(v) for p, v in found.items()}
    for want, pairs in found.items():
        for a, b in pairs:
            assert a < P and b < P and cp.pattern(a, b) == want

"""An integer model of the product's even/odd accumulation (csrc/field_asm.cuh, mont_mul_core / mont_mul2_core) and a fixed list of
canonical operand pairs that reaches every overflow pattern of the four-product accumulator O1, shared by
test_carry_patterns_model.py (CPU) and test_gpu_carry_counters.py (device).

The 128-bit operands are four 32-bit limbs a0..a3, b0..b3.  The 64-bit accumulators cover two columns each: E_k the columns
(2k, 2k+1), O_k the columns (2k+1, 2k+2).  Every v_mad_u64_u32 after an accumulator's first can overflow 64 bits; the overflows are
counted per accumulator and the counts enter the next accumulator of the same parity as the addend of its first v_mad:

    O0 = a0 b1 + a1 b0                         -> nO0 (1 event)
    E1 = a0 b2 + a1 b1 + a2 b0                 -> nE1 (2 events)
    O1 = (nO0 | nE1 << 32) + a0 b3, then + a1 b2 (c1), + a2 b1 (c2), + a3 b0 (c3)   -> nO1 = c1 + c2 + c3

The carry-outs are wave-wide masks in SGPR pairs and nO1 is the only counter of three events, so all eight patterns (c1, c2, c3)
matter, per lane and in every mixture within a wave -- whichever way the count is formed (three v_addc_co_u32 today; a form that
bit-slices the masks on the SALU, ones = c1 ^ c2 ^ c3 and twos = maj(c1, c2, c3), was measured and lost:
profiles/salu_counters)."""
import random

import field_cases as fc

P = fc.P
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
PATTERNS = [(c1, c2, c3) for c1 in (0, 1) for c2 in (0, 1) for c3 in (0, 1)]


def limbs(v):
    return [(v >> (32 * k)) & M32 for k in range(4)]


def _acc(start, products):
    """(value mod 2^64, carry-out of every product added to `start`)"""
    acc, carries = start, []
    for x, y in products:
        acc += x * y
        carries.append(acc >> 64)
        acc &= M64
    return acc, carries


def accumulate(a, b):
    """every accumulator and counter of the product a * b as the device computes them: a dict with E0..E3, O0..O2 (values mod 2^64),
    the counters nO0, nE1, nO1, nE2, nO2 and `pattern` = (c1, c2, c3) of O1"""
    A, B = limbs(a), limbs(b)
    r = {}
    r["E0"] = A[0] * B[0]
    r["O0"], c = _acc(A[0] * B[1], [(A[1], B[0])])
    r["nO0"] = sum(c)
    r["E1"], c = _acc(A[0] * B[2], [(A[1], B[1]), (A[2], B[0])])
    r["nE1"] = sum(c)
    first = A[0] * B[3] + (r["nO0"] | (r["nE1"] << 32))
    assert first <= M64, "the first v_mad of O1 cannot overflow (b3 <= PH3)"
    r["O1"], c = _acc(first, [(A[1], B[2]), (A[2], B[1]), (A[3], B[0])])
    r["pattern"], r["nO1"] = tuple(c), sum(c)
    r["E2"], c = _acc(A[1] * B[3], [(A[2], B[2]), (A[3], B[1])])
    r["nE2"] = sum(c)
    first = A[2] * B[3] + (r["nO1"] | (r["nE2"] << 32))
    assert first <= M64, "the first v_mad of O2 cannot overflow (b3 <= PH3)"
    r["O2"], c = _acc(first, [(A[3], B[2])])
    r["nO2"] = sum(c)
    r["E3"] = A[3] * B[3]
    return r


def merged(r):
    """T = E + (O << 32) as the merge chain forms it: E3's high word takes nO2 (the carries out of O2 have the weight of column 7)"""
    even = r["E0"] | (r["E1"] << 64) | (r["E2"] << 128) | (r["E3"] << 192)
    odd = r["O0"] | (r["O1"] << 64) | (r["O2"] << 128) | (r["nO2"] << 192)
    return even + (odd << 32)


def pattern(a, b):
    return accumulate(a, b)["pattern"]


def search(seed=20250611, draws=20000, per_pattern=2):
    """seeded search over limbs from a few extreme values and random ones, reduced mod p: {pattern: [pairs]}.  Three overflows need
    all four products near their maximum -- top limbs just below p's (a value with a larger one is reduced to a small one)."""
    rng = random.Random(seed)
    pick = lambda: rng.choice([0, 1, (1 << 31) - 1, 1 << 31, fc.PH3 - 1, M32 - 1, M32, rng.randrange(1 << 32)])
    value = lambda: sum(pick() << (32 * k) for k in range(4)) % P
    found = {p: [] for p in PATTERNS}
    for _ in range(draws):
        a, b = value(), value()
        hit = found[pattern(a, b)]
        if len(hit) < per_pattern:
            hit.append((a, b))
        if all(len(v) == per_pattern for v in found.values()):
            break
    return found


# Two canonical pairs per pattern, found once by search() and fixed here: the tests must not depend on a search succeeding.
PAIRS = {
    (0, 0, 0): [(0x7fffffff4fc4c9b580000000ce8ab0e7, 0x1800000000000000000000001), (0x22940c9f8fbaec3e7fffffff91b7143b, 0x347fffff8000000000000000fffffffd)],
    (0, 0, 1): [(0x347fffff7fffffff7fffffff00000000, 0x80000000ffffffffbe534abcffffffff), (0x7fffffffd469eb4fffffffff00000001, 0x110258a2afffffffffffffffe)],
    (0, 1, 0): [(0x347fffffebbc1d6380000000fffffffe, 0xa7ed2f09fffffffe00000001), (0x347ffffefffffffe000000014ad3af71, 0x256a59bafffffffffffffffdffffffff)],
    (0, 1, 1): [(0x7fffffffffffffff80000000fffffffe, 0x7fffffff80000000fbaa3234fffffffe), (0x80000000fffffffffffffffe7fffffff, 0xffffffffffffffff7fffffff)],
    (1, 0, 0): [(0x347ffffe80000000fffffffffffffffe, 0xbfb3ccd18000000080000000ffffffff), (0x7fffffff00000000ffffffffd678f5c8, 0x347ffffefffffffe7fffffff7fffffff)],
    (1, 0, 1): [(0x7fffffff80000000fffffffffffffffe, 0x7ffffffffffffffefffffffeffffffff), (0x7fffffff7fffffffffffffff80000000, 0x347ffffefffffffefffffffdffffffff)],
    (1, 1, 0): [(0x80000000fffffffffffffffeffffffff, 0x7fffffffee4aad75ffffffff7fffffff), (0xa3021817fffffffefffffffffffffffe, 0x347ffffffffffffefffffffffffffffe)],
    (1, 1, 1): [(0xcb7fffffffffffffcb7fffffd4129584, 0xcb7fffffcb7fffffffffffffffffffff), (0x99ee3fdefffffffecb7fffffcb7fffff, 0xcb7fffffffffffffffffffffffffffff)],
}


def all_pairs():
    """[(pattern, a, b)] in pattern order, the first pair of every pattern before the second ones"""
    return [(p, *PAIRS[p][k]) for k in range(2) for p in PATTERNS]

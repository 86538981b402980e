"""Operands for the field routines and a model of them in Python integers, shared by the CPU tests of the portable top-limb
corrections (test_fast_fixups_emu.py, test_field_model.py) and the device test of the hand-written forms (test_gpu_field_pairs.py).

model(op, a, b) gives, for op in ("add", "sub", "mul"), the flag a top-limb correction raises on (a, b) and the exact result
((a +- b) mod p, a * b * 2^-128 mod p); what a flagged correction returns is undefined and is not modelled."""
import functools
import random

from oracle import py_oracle as po

P = po.P
M32, M96, M128 = (1 << 32) - 1, (1 << 96) - 1, (1 << 128) - 1
PH3 = P >> 96
R = 1 << 128
R_M = R % P                               # the Montgomery form of 1
RINV = pow(R, -1, P)
PINV = pow(P, -1, R)
OPS = ("add", "sub", "mul")


def values():
    """canonical values: 25 edge values, 300 random ones, 120 that are small, near p or multiples of 2^96"""
    edge = [0, 1, 2, P - 1, P - 2, P - 3, PH3 << 96, (PH3 << 96) - 1, (PH3 - 1) << 96, ((PH3 - 1) << 96) + M96, 1 << 32, M32, 1 << 64, (1 << 64) - 1,
            1 << 96, M96, P - (1 << 32), P - (1 << 96), 1 << 127, (1 << 127) - 1, (P + 1) // 2, (P - 1) // 2, (1 << 32) + 1, P - (1 << 64), (1 << 127) + 1]
    assert len(edge) == 25 and all(0 <= v < P for v in edge)
    rng = random.Random(20240611)
    rand = [rng.randrange(P) for _ in range(300)]
    special = [rng.randrange(1 << 33) for _ in range(40)] + [P - 1 - rng.randrange(1 << 33) for _ in range(40)] + \
              [rng.randrange(PH3 + 1) << 96 for _ in range(40)]
    special = [v % P for v in special]
    return edge, rand, special


def lazy_values():
    """first operands of a product only: anything below 2^128 (the butterflies hand the product unreduced differences)"""
    rng = random.Random(7)
    return [M128, M128 - 1, 1 << 127, R - (1 << 32), R - (1 << 96), P, P + 1] + [rng.randrange(R) for _ in range(150)]


@functools.lru_cache(maxsize=None)
def crossed_lists(op):
    """(A, B): every a of A meets every b of B.  Sums and differences: all canonical values; products: 200 canonical and the lazy
    first operands against 240 canonical second operands (a second operand of a product is always below p)."""
    edge, rand, special = values()
    canon = edge + rand + special
    if op == "mul":
        return canon[:200] + lazy_values(), canon[:240]
    return canon, canon


def crossed_pairs(op):
    """the crossed lists as two flat lists: element i * len(B) + j is (A[i], B[j])"""
    A, B = crossed_lists(op)
    return [a for a in A for _ in B], [b for _ in A for b in B]


def random_pairs(n=1 << 16, seed=20250117):
    """seeded pairs of uniform canonical values: no correction flags any of them (asserted in test_field_model.py)"""
    rng = random.Random(seed)
    return [rng.randrange(P) for _ in range(n)], [rng.randrange(P) for _ in range(n)]


def model(op, a, b):
    """(flag, exact) of one top-limb correction.  The flag is the wrap of limb 0 when p is added or taken away on the limbs 0 and 3
    alone (fe_fixup_fast_c / fe_add_fast_c of csrc/field.cuh): the carry that the limbs 1 and 2 would have passed on."""
    if op == "add":
        r = a + b
        sel = r >= R or ((r & M128) >> 96) >= PH3
        return int(sel and (r & M32) == 0), r % P
    if op == "sub":
        d = (a - b) & M128
        return int(a < b and (d & M32) == M32), (a - b) % P
    if op == "mul":
        t = a * b
        m = (t & M128) * PINV & M128
        assert (t - m * P) & M128 == 0
        r = (t - m * P) >> 128
        assert -P < r < P
        return int(r < 0 and (r & M32) == M32), t * RINV % P
    raise ValueError(op)


def flagged_products(count=5):
    """products whose pre-correction difference (T - m' p) / 2^128 is negative with low limb 0xFFFFFFFF (the correction carries out of
    limb 0): searched among the products a * R~ = a with a = k * 2^32"""
    found = []
    for k in range(1, 4000):
        a = (k * 0x9E3779B97F4A7C15 % (1 << 96)) << 32
        if a < P and model("mul", a, R_M)[0]:
            found.append((a, R_M))
            if len(found) == count:
                break
    return found


def known_flagged(op):
    """operands known to raise the flag of `op`"""
    return {"sub": [(0, 1)], "add": [(P - 1, 1 << 32)], "mul": flagged_products()}[op]

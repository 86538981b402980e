"""The two-slot and the top-limb-correction forms of the device field routines (csrc/field_asm.cuh), as the kernels call them, against
Python integers, lane by lane, through sc_field_selftest2.

sc_field_selftest (test_gpu_cabi.py::test_device_field_ops) reaches the interleaved pair of products only with the same operands in
both slots, where a carry, borrow mask or select wired from one slot into the other changes nothing; here the slots hold different
operands.  The top-limb forms are held to field_cases.model: the flag of every lane equals the model's, every unflagged lane holds the
exact value (the value of a flagged lane is undefined by contract and is not asserted), and the wave-wide answer of rare_any is the OR
of the flags of that wave's own lanes.  test_field_model.py holds the portable twins to the same model and caps the flagged share.

The launch puts element i on thread i of 256-thread workgroups (include/starkcore.h), so wave w is the elements 64w .. 64w+63."""
import ctypes
import functools
import random

import pytest

import field_cases as fc
import synth
from test_gpu_fuzz import rand_vals

pytestmark = pytest.mark.gpu
P, R, RINV = fc.P, fc.R, fc.RINV
MUL2, ADDSUB2, ADD_FAST, SUB_FAST, MUL_FAST, MUL2_FAST, ADDSUB2_FAST, NEG = range(8)
ONE_SLOT = {"add": ADD_FAST, "sub": SUB_FAST, "mul": MUL_FAST}


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


def run(sc, op, a, b, c=None, d=None):
    """one launch: ([r0, r1, r2, r3] as lists of integers, own-lane flags, wave flags)"""
    n = len(a)
    c, d = (a if c is None else c), (b if d is None else d)
    assert len(b) == len(c) == len(d) == n
    out = ctypes.create_string_buffer(64 * n)
    word = (ctypes.c_uint32 * n)()
    sc._check(sc.lib().sc_field_selftest2(op, synth.pack_ints(a), synth.pack_ints(b), synth.pack_ints(c), synth.pack_ints(d), out, word, n))
    words = list(word)
    assert all(w < 4 for w in words)
    return [synth.unpack_ints(out.raw[16 * n * k:16 * n * (k + 1)]) for k in range(4)], [w & 1 for w in words], [w >> 1 for w in words]


def rot(xs, r):
    """element i gets what element (i + r) mod n has"""
    r %= len(xs)
    return xs[r:] + xs[:r]


@functools.lru_cache(maxsize=None)
def dataset(op, which):
    """(a, b, [(flag, exact)]) -- "crossed": the crossed lists of field_cases; "random": 2^16 seeded pairs with the edge residues of
    the fuzz tests mixed in (for products every other first operand lifted by p where that stays below 2^128: the lazy inputs), then
    the 2^16 uniform pairs on which the model flags nothing"""
    if which == "crossed":
        a, b = fc.crossed_pairs(op)
    else:
        rng = random.Random(4242)
        a, b = rand_vals(rng, 1 << 16), rand_vals(rng, 1 << 16)
        if op == "mul":
            a = [v + P if i & 1 and v + P < R else v for i, v in enumerate(a)]
        ua, ub = fc.random_pairs()
        a, b = a + ua, b + ub
    assert len(a) <= 200000
    return a, b, [fc.model(op, x, y) for x, y in zip(a, b)]


def rotations(op):
    """slot 1 takes the pair of the neighbouring lane, or one with both operands different (usually from another wave)"""
    return (1, len(fc.crossed_lists(op)[1]) + 1)


def check_exact(got, want, what):
    if got != want:
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        raise AssertionError("%s: %d of %d wrong, first at element %d (lane %d): got %#x, want %#x" % (what, len(bad), len(want), bad[0], bad[0] % 64, got[bad[0]], want[bad[0]]))


def check_fast(planes, own, wave, want_flags, want_values, what):
    """the flag of every lane is the model's, every unflagged lane is exact in every output, and every lane's wave flag is the OR of
    the own flags of its wave"""
    n = len(own)
    bad = [i for i in range(n) if own[i] != want_flags[i]]
    assert not bad, "%s: flag differs from the model at %d lanes, first element %d (lane %d): device %d, model %d" % (what, len(bad), bad[0], bad[0] % 64, own[bad[0]], want_flags[bad[0]])
    for k, want in enumerate(want_values):
        bad = [i for i in range(n) if not own[i] and planes[k][i] != want[i]]
        assert not bad, "%s: output %d of an unflagged lane is wrong at %d lanes, first element %d: got %#x, want %#x" % (what, k, len(bad), bad[0], planes[k][bad[0]], want[bad[0]])
    for w0 in range(0, n, 64):
        any_flag = int(any(own[w0:w0 + 64]))
        assert all(v == any_flag for v in wave[w0:w0 + 64]), "%s: wave %d: rare_any = %s, own flags %s" % (what, w0 // 64, wave[w0:w0 + 64], own[w0:w0 + 64])


# ---- the exact two-slot forms, different operands in the two slots

@pytest.mark.parametrize("which", ["crossed", "random"])
@pytest.mark.parametrize("rsel", [0, 1])
def test_mont_mul2_distinct_slots(sc, which, rsel):
    a, b, m = dataset("mul", which)
    r = rotations("mul")[rsel]
    exact = [e for _, e in m]
    planes, own, wave = run(sc, MUL2, a, b, rot(a, r), rot(b, r))
    check_exact(planes[0], exact, "mont_mul2 slot 0")
    check_exact(planes[1], rot(exact, r), "mont_mul2 slot 1")
    assert not any(own) and not any(wave)


def test_mont_mul2_worst_case_operands_differ_per_slot(sc):
    """the operands that drive the paired carry counters to their largest values (test_device_field_ops), a different one of the four
    patterns in each slot"""
    pats = [((1 << 128) - 1, P - 1), ((1 << 128) - 1, P - (1 << 32)), (0xFFFFFFFF, P - 1), ((1 << 128) - (1 << 96) + 0xFFFFFFFF, P - 2)]
    n = 64 * 5 + 13
    s0 = [i % 4 for i in range(n)]
    s1 = [(k + 1 + (i // 4) % 3) % 4 for i, k in enumerate(s0)]
    assert all(x != y for x, y in zip(s0, s1)) and {(x, y) for x, y in zip(s0, s1)} == {(x, y) for x in range(4) for y in range(4) if x != y}
    ops = [[pats[k][j] for k in s] for s in (s0, s1) for j in (0, 1)]
    planes, _, _ = run(sc, MUL2, *ops)
    check_exact(planes[0], [pats[k][0] * pats[k][1] * RINV % P for k in s0], "mont_mul2 slot 0")
    check_exact(planes[1], [pats[k][0] * pats[k][1] * RINV % P for k in s1], "mont_mul2 slot 1")


@pytest.mark.parametrize("which", ["crossed", "random"])
@pytest.mark.parametrize("rsel", [0, 1])
def test_fe_addsub2_distinct_slots(sc, which, rsel):
    a, b, m = dataset("add", which)
    r = rotations("add")[rsel]
    sums, diffs = [e for _, e in m], [(x - y) % P for x, y in zip(a, b)]
    planes, own, wave = run(sc, ADDSUB2, a, b, rot(a, r), rot(b, r))
    check_exact(planes[0], sums, "fe_addsub2 s0")
    check_exact(planes[1], diffs, "fe_addsub2 d0")
    check_exact(planes[2], rot(sums, r), "fe_addsub2 s1")
    check_exact(planes[3], rot(diffs, r), "fe_addsub2 d1")
    assert not any(own) and not any(wave)


# ---- the top-limb forms

@pytest.mark.parametrize("which", ["crossed", "random"])
@pytest.mark.parametrize("op", fc.OPS)
def test_fast_forms_one_slot(sc, op, which):
    a, b, m = dataset(op, which)
    planes, own, wave = run(sc, ONE_SLOT[op], a, b)
    check_fast(planes, own, wave, [f for f, _ in m], [[e for _, e in m]], op + "_fast")
    if which == "crossed":
        assert any(own), "the crossed lists reach the flag"


@pytest.mark.parametrize("which", ["crossed", "random"])
@pytest.mark.parametrize("rsel", [0, 1])
def test_mont_mul2_fast(sc, which, rsel):
    a, b, m = dataset("mul", which)
    r = rotations("mul")[rsel]
    flags, exact = [f for f, _ in m], [e for _, e in m]
    planes, own, wave = run(sc, MUL2_FAST, a, b, rot(a, r), rot(b, r))
    check_fast(planes, own, wave, [x | y for x, y in zip(flags, rot(flags, r))], [exact, rot(exact, r)], "mont_mul2_fast")


@pytest.mark.parametrize("which", ["crossed", "random"])
@pytest.mark.parametrize("rsel", [0, 1])
def test_fe_addsub2_fast(sc, which, rsel):
    a, b, ma = dataset("add", which)
    ms = dataset("sub", which)[2]
    assert dataset("sub", which)[:2] == (a, b)
    r = rotations("add")[rsel]
    flags = [x | y for (x, _), (y, _) in zip(ma, ms)]
    sums, diffs = [e for _, e in ma], [e for _, e in ms]
    planes, own, wave = run(sc, ADDSUB2_FAST, a, b, rot(a, r), rot(b, r))
    check_fast(planes, own, wave, [x | y for x, y in zip(flags, rot(flags, r))], [sums, diffs, rot(sums, r), rot(diffs, r)], "fe_addsub2_fast")


# ---- one lane's flag stays that lane's, one wave's stays that wave's

N_ISO = 64 * 8 + 17
# waves 0..4: one planted lane each; wave 5 and 7: none; wave 6: every lane; wave 8 (17 lanes): its last lane, the last element
PLANTED = [0 * 64 + 0, 1 * 64 + 1, 2 * 64 + 31, 3 * 64 + 32, 4 * 64 + 63] + list(range(6 * 64, 7 * 64)) + [N_ISO - 1]


def isolation_operands(op, slot):
    """seeded uniform operands that flag nowhere, with known flagged pairs of `op` planted in `slot` at PLANTED"""
    kinds = {"add": ["add"], "sub": ["sub"], "mul": ["mul"], "mul2": ["mul"], "addsub2": ["add", "sub"]}[op]
    rng = random.Random(777 + slot)
    ops = [[rng.randrange(P) for _ in range(N_ISO)] for _ in range(4)]
    for x, y in ((0, 1), (2, 3)):
        for kind in {"add", "sub", "mul"}:
            assert not any(fc.model(kind, u, v)[0] for u, v in zip(ops[x], ops[y])), "the base operands must not flag"
    known = [pair for kind in kinds for pair in fc.known_flagged(kind)]
    for j, i in enumerate(PLANTED):
        ops[2 * slot][i], ops[2 * slot + 1][i] = known[j % len(known)]
    return ops


@pytest.mark.parametrize("op,slot", [("add", 0), ("sub", 0), ("mul", 0), ("mul2", 0), ("mul2", 1), ("addsub2", 0), ("addsub2", 1)])
def test_lane_isolation(sc, op, slot):
    a, b, c, d = isolation_operands(op, slot)
    want_flags = [int(i in set(PLANTED)) for i in range(N_ISO)]
    if op in ONE_SLOT:
        planes, own, wave = run(sc, ONE_SLOT[op], a, b, c, d)
        want = [[fc.model(op, x, y)[1] for x, y in zip(a, b)]]
        model_flags = [fc.model(op, x, y)[0] for x, y in zip(a, b)]
    elif op == "mul2":
        planes, own, wave = run(sc, MUL2_FAST, a, b, c, d)
        want = [[fc.model("mul", x, y)[1] for x, y in zip(a, b)], [fc.model("mul", x, y)[1] for x, y in zip(c, d)]]
        model_flags = [fc.model("mul", x, y)[0] | fc.model("mul", z, w)[0] for x, y, z, w in zip(a, b, c, d)]
    else:
        planes, own, wave = run(sc, ADDSUB2_FAST, a, b, c, d)
        want = [[fc.model(k, x, y)[1] for x, y in zip(u, v)] for u, v in ((a, b), (c, d)) for k in ("add", "sub")]
        model_flags = [fc.model("add", x, y)[0] | fc.model("sub", x, y)[0] | fc.model("add", z, w)[0] | fc.model("sub", z, w)[0] for x, y, z, w in zip(a, b, c, d)]
    assert model_flags == want_flags                       # the model flags the planted lanes and nothing else
    assert [i for i in range(N_ISO) if own[i]] == sorted(PLANTED), (op, slot)
    check_fast(planes, own, wave, want_flags, want, "%s slot %d" % (op, slot))
    waves = [wave[w0] for w0 in range(0, N_ISO, 64)]
    assert waves == [1, 1, 1, 1, 1, 0, 1, 0, 1]


def test_fe_neg_and_empty_launch(sc):
    edge = fc.values()[0]
    planes, own, wave = run(sc, NEG, edge, edge)
    assert edge[0] == 0 and planes[0][0] == 0
    check_exact(planes[0], [(-v) % P for v in edge], "fe_neg")
    assert not any(own) and not any(wave)
    assert sc.lib().sc_field_selftest2(MUL2_FAST, None, None, None, None, None, None, 0) == 0
    assert sc.lib().sc_field_selftest2(8, None, None, None, None, None, None, 0) != 0

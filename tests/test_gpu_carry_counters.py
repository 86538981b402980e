"""The three-event carry counter of the device products (csrc/field_asm.cuh): the count of the overflows of the accumulator O1 comes
from three wave-wide carry masks in SGPR pairs, so a form that combines the masks (the bit-sliced SALU form of
profiles/salu_counters, or any later one) can go wrong in one lane because of what its neighbours hold.  The products' constants
(PH3 as an SGPR operand, inline zeros: SC_SGPR_CONST) ride through the same launches.

  * the fixed operand pairs of carry_patterns.py -- two per overflow pattern (c1, c2, c3), all eight patterns -- through
    sc_field_selftest op 0 (mont_mul) and sc_field_selftest2 ops 0, 4, 5, 18, 19 (the pair, the flag forms, the self-repairing forms):
    every lane of a wave on one pattern, the eight patterns interleaved lane by lane within a wave, and different patterns in the
    two slots of a pair.  Every lane must hold a * b * 2^-128 mod p; the flags of ops 4 and 5 must be field_cases.model's.
  * whole transforms through the three eight-element kernel shapes, on the smallest batches whose default plan takes them (the
    planner says which: tests/emu/kernel_cover.cpp), forward and inverse, on random data and on the 0 | 1 halves, bit for bit
    against sc_set_tuning("fast_fixups", 0) and against the C oracle.

The launches of the selftests put element i on thread i of 256-thread workgroups, so wave w is the elements 64w .. 64w+63."""
import ctypes
import functools

import numpy as np
import pytest

import carry_patterns as cp
import field_cases as fc
import ntt_grid
import synth
from oracle import py_oracle as po

pytestmark = pytest.mark.gpu
P, RINV = fc.P, fc.RINV
C = po.C
MUL1 = 0                                            # sc_field_selftest
MUL2, MUL_FAST, MUL2_FAST, MUL_FIX, MUL2_FIX = 0, 4, 5, 18, 19      # sc_field_selftest2
SINGLE, PAIR = (MUL_FAST, MUL_FIX), (MUL2, MUL2_FAST, MUL2_FIX)
DEFAULTS = dict(fast_fixups=1)


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    for key, value in DEFAULTS.items():
        starkcore.set_tuning(key, value)


# ---- the operand layouts: lists of (pattern, a, b), one entry per lane

PAIRS = cp.all_pairs()                               # 16 entries: the eight patterns, then their second pairs
N_WAVES = len(PAIRS)


@functools.lru_cache(maxsize=None)
def layout(name):
    """"uniform": wave w holds PAIRS[w] in every lane, and a last, partial wave of 17 lanes holds the three-overflow pattern;
    "interleaved": lane l of wave w holds PAIRS[(l + w) % 16], so every wave mixes all eight patterns, each wave shifted by a lane;
    "blocks": wave w holds the patterns in runs of 8 lanes, rotated by w runs (masks with long equal stretches)"""
    if name == "uniform":
        lanes = [PAIRS[w] for w in range(N_WAVES) for _ in range(64)] + [PAIRS[7]] * 17
    elif name == "interleaved":
        lanes = [PAIRS[(l + w) % 16] for w in range(N_WAVES) for l in range(64)]
    else:
        assert name == "blocks"
        lanes = [PAIRS[(l // 8 + w) % 16] for w in range(N_WAVES) for l in range(64)]
    assert {p for p, _, _ in lanes} == set(cp.PATTERNS)
    return tuple(lanes)


LAYOUTS = ("uniform", "interleaved", "blocks")


def exact(lanes):
    return [a * b * RINV % P for _, a, b in lanes]


def flags(lanes):
    return [fc.model("mul", a, b)[0] for _, a, b in lanes]


def run2(sc, op, la, lb):
    """sc_field_selftest2 with the lanes `la` in slot 0 and `lb` in slot 1: (plane 0, plane 1, own flags, wave flags)"""
    n = len(la)
    assert len(lb) == n
    out = ctypes.create_string_buffer(64 * n)
    word = (ctypes.c_uint32 * n)()
    a, b, c, d = ([v[k] for v in l] for l in (la, lb) for k in (1, 2))
    sc._check(sc.lib().sc_field_selftest2(op, synth.pack_ints(a), synth.pack_ints(b), synth.pack_ints(c), synth.pack_ints(d), out, word, n))
    words = list(word)
    assert all(w < 4 for w in words)
    planes = [synth.unpack_ints(out.raw[16 * n * k:16 * n * (k + 1)]) for k in range(2)]
    return planes[0], planes[1], [w & 1 for w in words], [w >> 1 for w in words]


def check_lanes(got, lanes, what):
    want = exact(lanes)
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, "%s: %d of %d lanes wrong, first at element %d (lane %d, pattern %s): got %#x, want %#x" % (
        what, len(bad), len(want), bad[0], bad[0] % 64, lanes[bad[0]][0], got[bad[0]], want[bad[0]])


def check_flags(op, own, wave, want):
    """ops 4 and 5 report the model's flag per lane and its OR over the lane's wave; the other forms have no flag"""
    if op not in (MUL_FAST, MUL2_FAST):
        assert not any(own) and not any(wave)
        return
    assert own == want
    for w0 in range(0, len(own), 64):
        assert all(v == int(any(want[w0:w0 + 64])) for v in wave[w0:w0 + 64]), "wave %d" % (w0 // 64)


# ---- the device forms

@pytest.mark.parametrize("name", LAYOUTS)
def test_mont_mul_single_form(sc, name):
    lanes = layout(name)
    n = len(lanes)
    out = ctypes.create_string_buffer(16 * n)
    sc._check(sc.lib().sc_field_selftest(MUL1, synth.pack_ints([a for _, a, _ in lanes]), synth.pack_ints([b for _, _, b in lanes]), out, n))
    check_lanes(synth.unpack_ints(out.raw), lanes, "mont_mul, %s" % name)


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("op", SINGLE)
def test_single_forms_of_selftest2(sc, op, name):
    lanes = layout(name)
    r0, _, own, wave = run2(sc, op, lanes, lanes)
    check_lanes(r0, lanes, "op %d, %s" % (op, name))
    check_flags(op, own, wave, flags(lanes))


# slot 1 against slot 0: the same lanes; the neighbouring pattern (rotated by one lane / one wave: another pattern in every lane);
# the complementary pattern (PAIRS[k] and PAIRS[7 - k] have complementary carries); one slot on a single pattern throughout
def _slot1(lanes, how):
    n = len(lanes)
    if how == "same":
        return lanes
    if how == "next lane":
        return lanes[1:] + lanes[:1]
    if how == "next wave":
        return lanes[64 % n:] + lanes[:64 % n]
    if how == "complement":
        return tuple(PAIRS[7 - cp.PATTERNS.index(p)] for p, _, _ in lanes)
    assert how in ("none", "all three")
    return (PAIRS[0] if how == "none" else PAIRS[7],) * n


SLOT1 = ("same", "next lane", "next wave", "complement", "none", "all three")


@pytest.mark.parametrize("how", SLOT1)
@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("op", PAIR)
def test_pair_forms(sc, op, name, how):
    la = layout(name)
    lb = _slot1(la, how)
    if how == "complement":
        assert all(tuple(1 - c for c in x[0]) == y[0] for x, y in zip(la, lb))
    for s0, s1 in ((la, lb), (lb, la)):
        r0, r1, own, wave = run2(sc, op, s0, s1)
        check_lanes(r0, s0, "op %d slot 0, %s / %s" % (op, name, how))
        check_lanes(r1, s1, "op %d slot 1, %s / %s" % (op, name, how))
        check_flags(op, own, wave, [x | y for x, y in zip(flags(s0), flags(s1))])


# ---- whole transforms through the eight-element shapes

SHAPES = ("fixed8<8,4>", "fixed8<9,3>", "fixed8<10,2>")
CANDIDATES = [(lg, cols) for cols in (2, 3, 4, 5, 6, 7, 8) for lg in range(12, 21)]       # two columns first, short before long


@functools.lru_cache(maxsize=None)
def _plans():
    """{(logn, cols): kernels of the default plan's passes, forward} from the planner (tests/emu/kernel_cover.cpp)"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = ntt_grid.build_helper(tmp)
        lines = ["tune default"] + ["ntt %d:%d %d %d %d 0 0 0" % (lg, c, lg, c, ntt_grid.NOLIMIT) for lg, c in CANDIDATES]
        out = ntt_grid.run_helper(exe, lines)
    plans = {}
    for line in out.splitlines():
        cid, *ks = line.split()
        lg, c = map(int, cid.split(":"))
        plans[(lg, c)] = tuple(k.split("@")[0] for k in ks)
    return plans


def batch_of(shape):
    """(logn, cols) of the first candidate whose default plan takes `shape` -- two columns where such a plan exists (no two-column
    plan takes fixed8<8,4>: its smallest batch has more columns) -- and that plan"""
    plans = _plans()
    hit = next(k for k in CANDIDATES if shape in plans[k])
    return hit, plans[hit]


def test_the_planner_reaches_every_shape_with_small_batches():
    chosen = [batch_of(shape)[0] for shape in SHAPES]
    assert all(lg <= 19 and cols <= 8 for lg, cols in chosen), chosen
    assert any(cols == 2 for _, cols in chosen)


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.int64).copy()).to(torch.device("cuda", 0))


def _transform(sc, x, n, cols, root, inverse, **tuning):
    import torch
    y = torch.empty_like(x)
    try:
        for key, value in tuning.items():
            sc.set_tuning(key, value)
        sc._check(sc.lib().sc_ntt_columns_dev(x.data_ptr(), y.data_ptr(), n, cols, sc.fe_bytes(root), inverse, None))
        sc.synchronize()
    finally:
        for key in tuning:
            sc.set_tuning(key, DEFAULTS[key])
    return y


def _halves(n):
    a = np.zeros((n, 2), dtype=np.uint64)
    a[n // 2:, 0] = 1
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def _column(logn, name, k):
    """column k of the data set `name` (bytes) and its forward and inverse transforms by the C oracle, computed once"""
    n = 1 << logn
    col = _halves(n) if name == "halves 0|1" else synth.synth_packed(4100 + 37 * logn + k, n).tobytes()
    root = po.primitive_nth_root(n)
    return col, C.ntt(root, col, n), C.intt(root, col, n)


@pytest.mark.parametrize("name", ["random", "halves 0|1"])
@pytest.mark.parametrize("shape", SHAPES)
def test_transforms_through_the_eight_element_shapes(sc, shape, name):
    import torch
    (logn, cols), plan = batch_of(shape)
    n = 1 << logn
    root = po.primitive_nth_root(n)
    # the halves are one column repeated; random columns differ (two distinct ones, cycled, keep the oracle's share small)
    columns = [_column(logn, name, 0 if name == "halves 0|1" else k % 2) for k in range(cols)]
    x = _dev(b"".join(c[0] for c in columns))
    for inverse in (0, 1):
        want = b"".join(c[1 + inverse] for c in columns)
        exact_run = _transform(sc, x, n, cols, root, inverse, fast_fixups=0)
        assert exact_run.cpu().numpy().tobytes() == want, (logn, cols, plan, name, inverse, "fast_fixups=0")
        y = _transform(sc, x, n, cols, root, inverse)
        assert torch.equal(y, exact_run), (logn, cols, plan, name, inverse)

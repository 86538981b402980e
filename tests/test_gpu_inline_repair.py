"""The self-repairing eight-element batch kernel (ntt_pass_kernel_fixed8: top-limb corrections repaired where a carry is dropped, one
launch per pass, csrc/field_asm.cuh) on the device.

  * the device forms lane by lane through the op codes 16..20 of sc_field_selftest2, against Python integers: waves with no repaired
    lane, exactly one and all 64, planted pairs in slot 0 only, slot 1 only and both; every lane of every output is asserted;
  * whole transforms through sc_ntt_columns_dev on the planted inputs of fast_fixups_cases.py (the one whose carry sits in the
    store-side product included) and on dense inputs where nearly every wave repairs, forward and inverse, under xcd_remap and
    wave_local 0 / 1, against the C oracle and against sc_set_tuning("fast_fixups", 0) bit for bit;
  * a three-pass transform whose in-place middle pass has an eight-element shape, and so takes the self-repairing kernel, on dense
    and random inputs against "fast_fixups" = 0.

The launch of sc_field_selftest2 puts element i on thread i of 256-thread workgroups, so wave w is the elements 64w .. 64w+63."""
import ctypes
import functools
import random

import numpy as np
import pytest

import fast_fixups_cases as fxc
import field_cases as fc
import synth
from oracle import py_oracle as po

pytestmark = pytest.mark.gpu
P, RINV = fc.P, fc.RINV
C = po.C
ADD_FIX, SUB_FIX, MUL_FIX, MUL2_FIX, ADDSUB2_FIX = 16, 17, 18, 19, 20
ONE_SLOT = {"add": ADD_FIX, "sub": SUB_FIX, "mul": MUL_FIX}
DEFAULTS = dict(fast_fixups=1, xcd_remap=1, wave_local=1, max_tile_log=-1)
EXACT = {"add": lambda a, b: (a + b) % P, "sub": lambda a, b: (a - b) % P, "mul": lambda a, b: a * b * RINV % P}


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    for key, value in DEFAULTS.items():
        starkcore.set_tuning(key, value)


# ---- the device forms

def run_forms(sc, op, a, b, c, d):
    n = len(a)
    out = ctypes.create_string_buffer(64 * n)
    word = (ctypes.c_uint32 * n)()
    sc._check(sc.lib().sc_field_selftest2(op, synth.pack_ints(a), synth.pack_ints(b), synth.pack_ints(c), synth.pack_ints(d), out, word, n))
    assert not any(word)                             # these forms have no flag
    return [synth.unpack_ints(out.raw[16 * n * k:16 * n * (k + 1)]) for k in range(4)]


def check_lanes(got, want, what):
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, "%s: %d of %d lanes wrong, first at element %d (lane %d): got %#x, want %#x" % (what, len(bad), len(want), bad[0], bad[0] % 64, got[bad[0]], want[bad[0]])


N_ISO = 64 * 8 + 17
# waves 0..4: one planted lane each; waves 5 and 7: none; wave 6: every lane; wave 8 (17 lanes): its last lane, the last element
PLANTED = [0 * 64 + 0, 1 * 64 + 1, 2 * 64 + 31, 3 * 64 + 32, 4 * 64 + 63] + list(range(6 * 64, 7 * 64)) + [N_ISO - 1]


def _repaired(kinds):
    """operands on which a form of `kinds` drops a carry: the known ones, and for sums those with r = p - 1, whose repair is undone"""
    known = [pair for kind in kinds for pair in fc.known_flagged(kind)]
    if "add" in kinds:
        known += [(P - 1, 0), ((P - 1) // 2, (P - 1) // 2), (P - 1, 1 << 64)]
    for kind in kinds:
        assert any(fc.model(kind, a, b)[0] for a, b in known)
    return known


@functools.lru_cache(maxsize=None)
def planted_operands(kinds, slots):
    """seeded uniform operands on which no form repairs, with repaired pairs planted at PLANTED in the given slots"""
    rng = random.Random(991 + 7 * len(kinds) + sum(slots))
    ops = [[rng.randrange(P) for _ in range(N_ISO)] for _ in range(4)]
    for x, y in ((0, 1), (2, 3)):
        for kind in fc.OPS:
            assert not any(fc.model(kind, u, v)[0] for u, v in zip(ops[x], ops[y])), "the base operands must not flag"
    known = _repaired(kinds)
    for slot in slots:
        for j, i in enumerate(PLANTED):
            ops[2 * slot][i], ops[2 * slot + 1][i] = known[(j + slot) % len(known)]
    flagged = [int(any(fc.model(kind, ops[2 * s][i], ops[2 * s + 1][i])[0] for kind in kinds for s in (0, 1))) for i in range(N_ISO)]
    assert [i for i, f in enumerate(flagged) if f] == sorted(PLANTED)
    return tuple(tuple(o) for o in ops)


@pytest.mark.parametrize("op", fc.OPS)
def test_one_slot_forms_lane_by_lane(sc, op):
    a, b, c, d = (list(o) for o in planted_operands((op,), (0,)))
    planes = run_forms(sc, ONE_SLOT[op], a, b, c, d)
    check_lanes(planes[0], [EXACT[op](x, y) for x, y in zip(a, b)], op + "_fix")
    # the structured operands, every pair
    A, B = fc.crossed_pairs(op)
    planes = run_forms(sc, ONE_SLOT[op], A, B, A, B)
    check_lanes(planes[0], [EXACT[op](x, y) for x, y in zip(A, B)], op + "_fix crossed")


@pytest.mark.parametrize("slots", [(0,), (1,), (0, 1)])
def test_mont_mul2_fix_lane_by_lane(sc, slots):
    a, b, c, d = (list(o) for o in planted_operands(("mul",), slots))
    planes = run_forms(sc, MUL2_FIX, a, b, c, d)
    check_lanes(planes[0], [EXACT["mul"](x, y) for x, y in zip(a, b)], "mont_mul2_fix slot 0")
    check_lanes(planes[1], [EXACT["mul"](x, y) for x, y in zip(c, d)], "mont_mul2_fix slot 1")


@pytest.mark.parametrize("kinds", [("add",), ("sub",), ("add", "sub")])
@pytest.mark.parametrize("slots", [(0,), (1,), (0, 1)])
def test_fe_addsub2_fix_lane_by_lane(sc, slots, kinds):
    a, b, c, d = (list(o) for o in planted_operands(kinds, slots))
    planes = run_forms(sc, ADDSUB2_FIX, a, b, c, d)
    for k, (u, v, kind) in enumerate(((a, b, "add"), (a, b, "sub"), (c, d, "add"), (c, d, "sub"))):
        check_lanes(planes[k], [EXACT[kind](x, y) for x, y in zip(u, v)], "fe_addsub2_fix output %d" % k)


def test_paired_forms_on_the_structured_operands(sc):
    """every structured pair in slot 0 against a rotated copy in slot 1"""
    A, B = fc.crossed_pairs("mul")
    r = len(fc.crossed_lists("mul")[1]) + 1
    A1, B1 = A[r:] + A[:r], B[r:] + B[:r]
    planes = run_forms(sc, MUL2_FIX, A, B, A1, B1)
    check_lanes(planes[0], [EXACT["mul"](x, y) for x, y in zip(A, B)], "mont_mul2_fix slot 0")
    check_lanes(planes[1], [EXACT["mul"](x, y) for x, y in zip(A1, B1)], "mont_mul2_fix slot 1")
    A, B = fc.crossed_pairs("add")
    r = len(fc.crossed_lists("add")[1]) + 1
    A1, B1 = A[r:] + A[:r], B[r:] + B[:r]
    planes = run_forms(sc, ADDSUB2_FIX, A, B, A1, B1)
    for k, (u, v, kind) in enumerate(((A, B, "add"), (A, B, "sub"), (A1, B1, "add"), (A1, B1, "sub"))):
        check_lanes(planes[k], [EXACT[kind](x, y) for x, y in zip(u, v)], "fe_addsub2_fix output %d" % k)


def test_new_codes_leave_the_gap_unknown(sc):
    for op in (8, 15, 21):
        assert sc.lib().sc_field_selftest2(op, None, None, None, None, None, None, 0) != 0
    assert sc.lib().sc_field_selftest2(ADDSUB2_FIX, None, None, None, None, None, None, 0) == 0


# ---- whole transforms

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


@pytest.mark.parametrize("shape,inverse,name", fxc.case_ids())
def test_planted_inputs_one_launch_per_pass(sc, shape, inverse, name):
    import torch
    case = fxc.build(shape, inverse, name)
    plan = case.plan
    want = plan.oracle(case.data)
    x = _dev(case.data)
    exact = _transform(sc, x, plan.n, plan.cols, plan.root, inverse, fast_fixups=0)
    assert exact.cpu().numpy().tobytes() == want, (shape, inverse, name, "fast_fixups=0")
    for remap in (0, 1):
        for wave_local in (0, 1):
            y = _transform(sc, x, plan.n, plan.cols, plan.root, inverse, xcd_remap=remap, wave_local=wave_local)
            assert torch.equal(y, exact), (shape, inverse, name, remap, wave_local)


def _fe(v, count):
    a = np.empty((count, 2), dtype=np.uint64)
    a[:, 0] = v & ((1 << 64) - 1)
    a[:, 1] = v >> 64
    return a


def _dense_column(n, name):
    if name == "p-1":
        return _fe(P - 1, n).tobytes()
    if name == "alternating":
        a = _fe(0, n)
        a[1::2, 0] = 1
        return a.tobytes()
    assert name == "halves 0|1"
    return _fe(0, n // 2).tobytes() + _fe(1, n // 2).tobytes()


DENSE = ["halves 0|1", "p-1", "alternating"]


@functools.lru_cache(maxsize=None)
def _dense_want(logn, name, inverse):
    n = 1 << logn
    return (C.intt if inverse else C.ntt)(po.primitive_nth_root(n), _dense_column(n, name), n)


# passes: 2^17 x 8 (9,3) (8,4) | 2^19 x 2 (10,2) (9,3) | 2^20 x 2 (10,2) (10,2): the lengths of fast_fixups_cases.py and the benchmark's
@pytest.mark.parametrize("name", DENSE)
@pytest.mark.parametrize("logn,cols", [(17, 8), (19, 2), (20, 2)])
def test_dense_inputs_nearly_every_wave_repairs(sc, logn, cols, name):
    import torch
    n = 1 << logn
    root = po.primitive_nth_root(n)
    x = _dev(_dense_column(n, name) * cols)
    for inverse in (0, 1):
        want = _dense_want(logn, name, inverse) * cols
        exact = _transform(sc, x, n, cols, root, inverse, fast_fixups=0)
        assert exact.cpu().numpy().tobytes() == want, (logn, cols, name, inverse, "fast_fixups=0")
        for remap in (0, 1):
            for wave_local in (0, 1):
                y = _transform(sc, x, n, cols, root, inverse, xcd_remap=remap, wave_local=wave_local)
                assert torch.equal(y, exact), (logn, cols, name, inverse, remap, wave_local)


def _device_random(count, seed):
    """canonical values made on the device: limbs below 2^62 (p's top 64-bit limb is above 2^63)"""
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    x = torch.randint(0, 1 << 62, (2 * count,), dtype=torch.int64, device=torch.device("cuda", 0), generator=g)
    torch.cuda.synchronize()                         # the library runs on a stream of its own
    return x


@pytest.mark.parametrize("name", DENSE + ["random"])
def test_in_place_pass_takes_the_repairing_kernel(sc, name):
    """2^23 x 2 columns under max_tile_log = 12: the smallest batch whose plan has an in-place pass (the middle one of three) on an
    eight-element shape -- fixed8<8,4>, fixed8<8,4>, generic by tests/emu/kernel_cover; the default plans of three passes use
    2^11-element tiles and four elements a thread.  Compared with "fast_fixups" = 0, which takes the exact kernel there."""
    import torch
    logn, cols = 23, 2
    n = 1 << logn
    root = po.primitive_nth_root(n)
    if name == "random":
        x = _device_random(n * cols, 3123)
    else:
        col = _dev(_dense_column(n, name))
        x = torch.cat([col] * cols)
        torch.cuda.synchronize()                     # made by a kernel on torch's stream; the library runs on a stream of its own
    knobs = dict(max_tile_log=12)
    assert sc.lib().sc_ntt_num_passes(n) == 3
    for inverse in (0, 1):
        exact = _transform(sc, x, n, cols, root, inverse, fast_fixups=0, **knobs)
        y = _transform(sc, x, n, cols, root, inverse, **knobs)
        assert torch.equal(y, exact), (name, inverse)
        if inverse == 0:
            # the pair of transforms is the identity: ties the exact mode itself to the input
            assert torch.equal(_transform(sc, y, n, cols, root, 1, **knobs), x), name

"""The integer model of the top-limb corrections (field_cases.model) against their portable twins (fe_add_fast_c, fe_sub_fast_c,
mont_mul_fast_c of csrc/field.cuh, through tests/emu/ntt_fast_emu.cpp): the same flag and the same exact value on every pair of the
shared operand lists.  test_gpu_field_pairs.py holds the device forms to the same model, so the two together say that the twins and the
device forms flag the same operands -- what the CPU emulation of the tiles assumes.  The caps on the flagged share are asserted on the
model alone: the device test asserts no value of a flagged lane, so a model that flagged much would hide a wrong routine."""
import ctypes

import pytest

import field_cases as fc
from test_fast_fixups_emu import emu      # noqa: F401  (the build fixture of the emulation library)

EMU_OP = {"add": 0, "sub": 1, "mul": 2}


def _pack(vals):
    return b"".join(int(v).to_bytes(16, "little") for v in vals)


def _emu_pairs(emu, op, a, b):
    """[(flag, exact)] of fast_field_one over the pairs (a[i], b[i])"""
    n = len(a)
    pa, pb = ctypes.create_string_buffer(_pack(a), 16 * n), ctypes.create_string_buffer(_pack(b), 16 * n)
    base_a, base_b = ctypes.addressof(pa), ctypes.addressof(pb)
    out = (ctypes.c_uint64 * 4)()
    res = []
    for i in range(n):
        flag = emu.fast_field_one(EMU_OP[op], base_a + 16 * i, base_b + 16 * i, out)
        res.append((flag, out[2] | (out[3] << 64)))
    return res


@pytest.fixture(scope="module")
def modelled():
    """op -> [(flag, exact)] of the model over the crossed lists (computed once)"""
    return {op: [fc.model(op, x, y) for x, y in zip(*fc.crossed_pairs(op))] for op in fc.OPS}


@pytest.mark.parametrize("op", fc.OPS)
def test_model_agrees_with_portable_twins(emu, modelled, op):  # noqa: F811
    a, b = fc.crossed_pairs(op)
    assert len(a) == {"add": 198025, "sub": 198025, "mul": 85680}[op]
    got = _emu_pairs(emu, op, a, b)
    bad = [(hex(x), hex(y), g, m) for x, y, g, m in zip(a, b, got, modelled[op]) if g != m]
    assert not bad, (op, len(bad), bad[:3])


@pytest.mark.parametrize("op", fc.OPS)
def test_model_agrees_on_random_and_known_pairs(emu, op):  # noqa: F811
    a, b = fc.random_pairs(1 << 12)
    known = fc.known_flagged(op)
    a, b = a + [x for x, _ in known], b + [y for _, y in known]
    assert _emu_pairs(emu, op, a, b) == [fc.model(op, x, y) for x, y in zip(a, b)]
    assert all(fc.model(op, x, y)[0] == 1 for x, y in known)
    assert len(fc.known_flagged("mul")) == 5


def test_flagged_share_stays_under_the_caps(modelled):
    """<= 2 % per one-slot routine over the crossed lists (0.44 %, 0.19 %, 0.14 % when this was written), <= 4 % for the two-slot
    routines, whose flag is the OR of two or four of those; none at all on 2^16 uniform pairs"""
    share = {}
    for op in fc.OPS:
        flags = [f for f, _ in modelled[op]]
        share[op] = sum(flags) / len(flags)
        print(op, "flagged share %.4f %%" % (100 * share[op]))
        assert 0 < share[op] <= 0.02, (op, share[op])
    # two-slot forms with slot 1 = the pair r elements further on (the rotations of the device test)
    addsub = [x[0] | y[0] for x, y in zip(modelled["add"], modelled["sub"])]
    for name, op, flags in (("mont_mul2_fast", "mul", [f for f, _ in modelled["mul"]]), ("fe_addsub2_fast", "add", addsub)):
        n = len(flags)
        for r in (1, len(fc.crossed_lists(op)[1]) + 1):
            both = sum(flags[i] | flags[(i + r) % n] for i in range(n)) / n
            print(name, "r =", r, "flagged share %.4f %%" % (100 * both))
            assert both <= 0.04, (name, r, both)
    a, b = fc.random_pairs()
    assert len(a) == 1 << 16
    for op in fc.OPS:
        assert sum(fc.model(op, x, y)[0] for x, y in zip(a, b)) == 0, op

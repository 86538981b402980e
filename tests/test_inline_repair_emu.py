"""The self-repairing top-limb field corrections of the eight-element batch kernel on the CPU (tests/emu/ntt_fix_emu.cpp): the portable
twins (csrc/field.cuh: fe_add_fix_c / fe_sub_fix_c / mont_mul_fix_c, limb for limb what csrc/field_asm.cuh does) equal the exact forms
on every pair -- none is excluded, there is no flag -- and the structured operands do take the repair; and single tiles of each kernel
shape through the ARITH_FIX rounds are bit-equal to the exact rounds on the planted inputs of fast_fixups_cases.py and on a tile that
holds p - 1 everywhere."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
import fast_fixups_cases as fxc
import field_cases as fc

P = fc.P
EMU_DIR = os.path.join(REPO, "tests", "emu")
OPCODE = {"add": 0, "sub": 1, "mul": 2}


@functools.lru_cache(maxsize=None)
def load_fix_emu():
    """tests/emu/libntt_fix_emu.so, built on demand the way test_fast_fixups_emu.py builds its library"""
    so = os.path.join(EMU_DIR, "libntt_fix_emu.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("ntt_fix_emu.cpp", "ntt_fast_emu.cpp", "ntt_emu.cpp")] + \
           [os.path.join(REPO, "stark-anatomy_amd", "csrc", f) for f in ("field.cuh", "ntt_tile.cuh", "ntt_plan.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    vp, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
    lib.fix_field_one.restype = i32
    lib.fix_field_one.argtypes = [i32, vp, vp, vp]
    lib.fix_field_pairs.restype = None
    lib.fix_field_pairs.argtypes = [i32, i32, vp, u64, vp, u64, vp]
    lib.fix_field_two.restype = None
    lib.fix_field_two.argtypes = [i32, vp, vp, vp, vp, vp]
    lib.fx_open.restype = vp
    lib.fx_open.argtypes = [i32, i32, vp, i32]
    lib.fx_close.restype = None
    lib.fx_close.argtypes = [vp]
    lib.fix_tile.restype = i32
    lib.fix_tile.argtypes = [vp, i32, u32, vp, vp, vp, vp, vp, vp]
    return lib


@pytest.fixture(scope="module")
def emu():
    return load_fix_emu()


def _pack(vals):
    return b"".join(int(v).to_bytes(16, "little") for v in vals)


def _one(emu, op, a, b):
    out = ctypes.create_string_buffer(32)
    flag = emu.fix_field_one(OPCODE[op], _pack([a]), _pack([b]), out)
    return flag, int.from_bytes(out.raw[:16], "little"), int.from_bytes(out.raw[16:], "little")


def _pairs(emu, op, crossed, a, b):
    counts = (ctypes.c_uint64 * 3)()
    emu.fix_field_pairs(OPCODE[op], int(crossed), _pack(a), len(a), _pack(b), len(b), counts)
    return list(counts)


@pytest.mark.parametrize("op", fc.OPS)
def test_twins_equal_the_exact_forms_on_every_pair(emu, op):
    # the structured operand set, all pairs: nothing differs, and the repair is taken (the fast twin flags there)
    A, B = fc.crossed_lists(op)
    total, differ, repaired = _pairs(emu, op, True, A, B)
    assert total == len(A) * len(B)
    assert differ == 0, (op, differ)
    assert repaired > 0, op
    # the known flagged operands of this operation
    known = fc.known_flagged(op)
    total, differ, repaired = _pairs(emu, op, False, [a for a, _ in known], [b for _, b in known])
    assert (total, differ, repaired) == (len(known), 0, len(known)), op
    for a, b in known:
        flag, fix, exact = _one(emu, op, a, b)
        assert flag == 1 and fix == exact == fc.model(op, a, b)[1], (op, hex(a), hex(b))
    # 400 000 seeded random pairs
    a, b = fc.random_pairs(400000, seed=20260401 + OPCODE[op])
    total, differ, _ = _pairs(emu, op, False, a, b)
    assert (total, differ) == (400000, 0), op


def test_the_sum_that_equals_p_minus_1_is_among_the_repairs(emu):
    """r = p - 1 = [0, 0, 0, PH3]: the top limb says r >= p, limb 0 borrows, the borrow runs out of the top: the result is r itself"""
    edge = fc.values()[0]
    A, B = fc.crossed_lists("add")
    hits = [(a, b) for a in edge for b in edge if a + b == P - 1]
    assert hits and all(a in A and b in B for a, b in hits)
    for a, b in hits + [(P - 1 - (1 << 96), 1 << 96), ((P - 1) // 2, (P - 1) // 2)]:
        flag, fix, exact = _one(emu, "add", a, b)
        assert a + b == P - 1 and flag == 1 and fix == exact == P - 1, (hex(a), hex(b))
    # its neighbours: r = p (-> 0) and r = p - 1 + 2^32 (a borrow that stops in limb 1)
    for a, b in ((P - 1, 1), (P - 1, 1 << 32), (P - 1, 1 << 64), (P - 1, 1 << 96), (P - 1, P - 1)):
        _, fix, exact = _one(emu, "add", a, b)
        assert fix == exact == (a + b) % P, (hex(a), hex(b))


def test_paired_dispatchers_keep_the_slots_apart(emu):
    """mont_mul2_fix / fe_addsub2_fix with a repaired pair in slot 0 only, slot 1 only and both"""
    plain = (0x1234567890ABCDEF1122334455667788 % P, 0x0FEDCBA987654321AABBCCDDEEFF0011 % P)
    assert not any(fc.model(op, *plain)[0] for op in fc.OPS)
    for kind, ops in ((0, ("mul",)), (1, ("add", "sub"))):
        for op in ops:
            bad = fc.known_flagged(op)[0]
            for s0, s1 in ((bad, plain), (plain, bad), (bad, bad)):
                out = ctypes.create_string_buffer(64)
                emu.fix_field_two(kind, _pack([s0[0]]), _pack([s0[1]]), _pack([s1[0]]), _pack([s1[1]]), out)
                got = [int.from_bytes(out.raw[16 * k:16 * k + 16], "little") for k in range(4)]
                if kind == 0:
                    want = [fc.model("mul", *s0)[1], fc.model("mul", *s1)[1], 0, 0]
                else:
                    want = [fc.model("add", *s0)[1], fc.model("sub", *s0)[1], fc.model("add", *s1)[1], fc.model("sub", *s1)[1]]
                assert got == want, (op, s0 is bad, s1 is bad)


# ---- single tiles

def _tile(emu, plan, k, tile, buf):
    """(ARITH_FIX output, exact output, flag of the ARITH_FAST rounds) of one tile of pass k on the pass's input `buf`"""
    of, oe, scratch = plan.empty(), plan.empty(), plan.empty()
    flag, rare = ctypes.c_uint64(0), ctypes.c_uint64(0)
    shape = emu.fix_tile(plan.h, k, tile, buf.ctypes.data, of.ctypes.data, oe.ctypes.data, scratch.ctypes.data, ctypes.byref(flag), ctypes.byref(rare))
    assert shape == plan.passes[k].logR * 100 + plan.passes[k].logC, shape
    assert rare.value == 0                       # the mode has no accumulator
    return of, oe, flag.value


@pytest.mark.parametrize("shape,inverse,name", fxc.case_ids())
def test_planted_tiles_fix_rounds_equal_exact_rounds(emu, shape, inverse, name):
    case = fxc.build(shape, inverse, name)
    plan = case.plan
    bufs = {0: np.frombuffer(case.data, dtype=np.uint64).reshape(-1, 2).copy()}
    for f in case.flagged:
        for k in range(f.k):
            if k + 1 not in bufs:
                bufs[k + 1] = plan.run_pass(k, bufs[k], fast=False)[1]
        of, oe, flag = _tile(emu, plan, f.k, f.tile, bufs[f.k])
        assert flag != 0, f                      # the tile does take a repair
        assert oe.any() and np.array_equal(of, oe), f


@pytest.mark.parametrize("shape,k,want", [("A", 0, 903), ("A", 1, 804), ("B", 0, 1002)])
def test_a_tile_of_p_minus_1_fix_rounds_equal_exact_rounds(emu, shape, k, want):
    logn, cols = fxc.SHAPES[shape]
    for inverse in (0, 1):
        plan = fxc.Plan(logn, cols, inverse)
        assert plan.passes[k].logR * 100 + plan.passes[k].logC == want and plan.passes[k].fixed8
        buf = plan.empty()
        buf[:, 0] = (P - 1) & ((1 << 64) - 1)
        buf[:, 1] = (P - 1) >> 64
        for tile in (0, plan.nwg(k) - 1):
            of, oe, flag = _tile(emu, plan, k, tile, buf)
            assert flag != 0, (shape, k, inverse, tile)
            assert oe.any() and np.array_equal(of, oe), (shape, k, inverse, tile)

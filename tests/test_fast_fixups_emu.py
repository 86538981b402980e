"""The top-limb field corrections of the eight-element batch kernels on the CPU (tests/emu/ntt_fast_emu.cpp): the portable twins of the
device forms against the exact forms over edge, structured and random values -- every unflagged result equal, the known bad cases
flagged -- and one tile of each kernel shape through the FAST and the exact rounds."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import REPO
import field_cases
from oracle import py_oracle as po

P = po.P
EMU_DIR = os.path.join(REPO, "tests", "emu")
M32, M96, M128 = (1 << 32) - 1, (1 << 96) - 1, (1 << 128) - 1
PH3 = P >> 96


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libntt_fast_emu.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("ntt_fast_emu.cpp", "ntt_emu.cpp")] + \
           [os.path.join(REPO, "stark-anatomy_amd", "csrc", f) for f in ("field.cuh", "ntt_tile.cuh", "ntt_plan.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    lib.fast_field_one.restype = ctypes.c_int
    lib.fast_field_one.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.fast_field_pairs.restype = None
    lib.fast_field_pairs.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.fast_tile.restype = ctypes.c_int
    lib.fast_tile.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


_values = field_cases.values      # the operand lists live in field_cases.py, shared with the model and the device test


def _pack(vals):
    return b"".join(int(v).to_bytes(16, "little") for v in vals)


def _one(emu, op, a, b):
    out = ctypes.create_string_buffer(32)
    flag = emu.fast_field_one(op, _pack([a]), _pack([b]), out)
    return flag, int.from_bytes(out.raw[:16], "little"), int.from_bytes(out.raw[16:], "little")


def _pairs(emu, op, a, b):
    counts = (ctypes.c_uint64 * 4)()
    emu.fast_field_pairs(op, _pack(a), len(a), _pack(b), len(b), counts)
    return list(counts)


def test_fast_forms_equal_exact_where_unflagged(emu):
    edge, rand, special = _values()
    canon = edge + rand + special
    rng = random.Random(7)
    left = canon[:200] + [rng.randrange(1 << 128) for _ in range(150)] + [M128, M128 - 1, 1 << 127, (1 << 128) - (1 << 32), (1 << 128) - (1 << 96)]
    for op, a, b in ((0, canon, canon), (1, canon, canon), (2, left, canon[:240])):
        total, flagged, bad, wrong = _pairs(emu, op, a, b)
        assert total == len(a) * len(b)
        assert bad == 0, (op, bad)
        assert 0 < flagged < total // 50, (op, flagged, total)          # the structured values do reach the flag, and it stays rare
        if op < 2:
            assert wrong > 0, op                                            # ... and some flagged results are indeed wrong without the redo
    # random data does not flag
    rng = random.Random(11)
    a, b = [rng.randrange(P) for _ in range(2000)], [rng.randrange(P) for _ in range(200)]
    for op in (0, 1, 2):
        total, flagged, bad, _ = _pairs(emu, op, a, b)
        assert (total, flagged, bad) == (400000, 0, 0), op


def test_exact_reference_is_the_field(emu):
    """the comparison's reference (fe_add_c / fe_sub_c / mont_mul_c) against Python integers on the edge values"""
    edge, rand, _ = _values()
    rinv = pow(1 << 128, P - 2, P)
    for a in edge + rand[:20]:
        for b in edge:
            assert _one(emu, 0, a, b)[2] == (a + b) % P
            assert _one(emu, 1, a, b)[2] == (a - b) % P
            assert _one(emu, 2, a, b)[2] == a * b * rinv % P


def test_known_cases_are_flagged(emu):
    flag, fast, exact = _one(emu, 1, 0, 1)
    assert flag == 1 and exact == P - 1 and fast != exact
    flag, fast, exact = _one(emu, 0, P - 1, 1 << 32)
    assert flag == 1 and exact == (1 << 32) - 1 and fast != exact
    # a product whose pre-correction difference R = (T - m' p) / 2^128 is negative with low limb 0xFFFFFFFF (its correction carries
    # out of limb 0): searched among the products a * R~ = a with a = k * 2^32, modelled with Python integers (field_cases.flagged_products)
    found = 0
    for a, r_m in field_cases.flagged_products(5):
        assert r_m == (1 << 128) % P and a < P and a % (1 << 32) == 0
        flag, fast, exact = _one(emu, 2, a, r_m)
        assert exact == a and flag == 1, hex(a)
        found += 1
    assert found == 5


def _tile(emu, logn, cols, npass, data, root):
    n = 1 << logn
    fast, exact = ctypes.create_string_buffer(16 * cols * n), ctypes.create_string_buffer(16 * cols * n)
    rare = ctypes.c_uint64(0)
    shape = emu.fast_tile(logn, cols, npass, data, fast, exact, int(root).to_bytes(16, "little"), ctypes.byref(rare))
    return shape, rare.value, fast.raw, exact.raw


# (logn, columns, pass) -> tile shape: 2^17 x 8 = (9,3) then (8,4); 2^19 x 2 = (10,2) then (9,3)   (fewer columns of 2^17 get smaller tiles)
@pytest.mark.parametrize("logn,cols,npass,shape", [(17, 8, 1, 804), (17, 8, 0, 903), (19, 2, 0, 1002)])
def test_one_tile_fast_against_exact(emu, logn, cols, npass, shape):
    import numpy as np
    import synth
    n = 1 << logn
    root = po.primitive_nth_root(n)
    got, rare, fast, exact = _tile(emu, logn, cols, npass, synth.synth_packed(4100 + logn, cols * n).tobytes(), root)
    assert got == shape
    assert rare == 0 and fast == exact and any(exact)
    # the first butterflies of the tile pair the halves of its rows' axis: the first half of a column for the column pass (pass 0),
    # the halves of every contiguous run of R elements for the transposing pass
    R = 1 << (shape // 100)
    j = np.arange(cols * n, dtype=np.uint64)
    upper = ((j % np.uint64(n)) >= np.uint64(n // 2)) if npass == 0 else ((j % np.uint64(R)) >= np.uint64(R // 2))

    def halves(lo, hi):
        a = np.zeros((cols * n, 2), dtype=np.uint64)
        for val, sel in ((lo, ~upper), (hi, upper)):
            a[sel, 0] = val & ((1 << 64) - 1)
            a[sel, 1] = val >> 64
        return a.tobytes()
    for lo, hi in ((0, 1), (P - 1, 1 << 32)):          # u - v = -1 flags through sub; (p-1) + 2^32 flags through add
        got, rare, fast, exact = _tile(emu, logn, cols, npass, halves(lo, hi), root)
        assert got == shape and rare != 0, (lo, hi)

"""CPU build of the batched verifier's row checks (csrc/merkle_verify.cuh, compiled for the host by tests/emu/merkle_verify_emu.cpp)
against the host functions they replace: Merkle.verify_ / hashlib paths and test_colinearity.  The device BLAKE2b of merkle.cuh
does not compile for the host, so the emulation hashes with the host compression of csrc/transcript.h; the row layout, the
indexing, the position bits and the field arithmetic are the kernels' own."""
import ctypes
import os
import random
import subprocess
from hashlib import blake2b

import numpy as np
import pytest

from conftest import REPO
import starkcore as sc
from algebra import Field, FieldElement
from merkle import Merkle
from univariate import test_colinearity

EMU_DIR = os.path.join(REPO, "tests", "emu")
P = Field.P_MAIN


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libmerkle_verify_emu.so")
    srcs = [os.path.join(EMU_DIR, "merkle_verify_emu.cpp")] + [os.path.join(REPO, "stark-anatomy_amd", "csrc", f)
                                                               for f in ("merkle_verify.cuh", "field.cuh", "transcript.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    lib.emu_merkle_verify.restype = None
    lib.emu_merkle_verify.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p]
    lib.emu_colinearity.restype = None
    lib.emu_colinearity.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def run_merkle(lib, rows, digests, roots):
    rows = sc.merkle_rows(*[[r[k] for r in rows] for k in range(5)], b"".join(r[5] for r in rows))
    out = np.zeros(len(rows), dtype=np.uint8)
    lib.emu_merkle_verify(rows.ctypes.data, len(rows), b"".join(digests) or b"\0" * 64, b"".join(roots), out.ctypes.data)
    return out


def run_colinearity(lib, rows, rounds):
    rows = sc.colinearity_rows([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], b"".join(r[3] for r in rows))
    rounds = np.frombuffer(b"".join(rounds), dtype=sc.COLINEARITY_ROUND)
    out = np.zeros(len(rows), dtype=np.uint8)
    lib.emu_colinearity(rows.ctypes.data, len(rows), rounds.ctypes.data, out.ctypes.data)
    return out


def test_row_layouts(emu):
    sizes = (ctypes.c_uint64 * 3)()
    emu.emu_row_sizes(sizes)
    assert list(sizes) == [sc.MERKLE_ROW.itemsize, sc.COLINEARITY_ROW.itemsize, sc.COLINEARITY_ROUND.itemsize]


def tree_levels(leaf_digests):
    levels = [list(leaf_digests)]
    while len(levels[-1]) > 1:
        lv = levels[-1]
        levels.append([blake2b(lv[i] + lv[i + 1]).digest() for i in range(0, len(lv), 2)])
    return levels


def path_of(levels, index):
    return [levels[l][(index >> l) ^ 1] for l in range(len(levels) - 1)]


def fe16(v):
    return v.to_bytes(16, "little")


@pytest.mark.parametrize("logn", [1, 2, 5, 8])
def test_merkle_rows_match_host(emu, logn):
    rng = random.Random(700 + logn)
    n = 1 << logn
    values = [rng.randrange(P) for _ in range(n)]
    values[0], values[-1] = 0, P - 1
    if n >= 4:
        values[1] = (1 << 128) - 1         # a leaf value >= p: the tree hashes its decimal digits all the same
    levels = tree_levels([blake2b(b"%d" % v).digest() for v in values])
    root = levels[-1][0]
    roots = [root, blake2b(b"another root").digest()]
    cases = []          # (root index, position, path, leaf value or digest)
    for _ in range(24):
        i = rng.randrange(n)
        path = path_of(levels, i)
        cases.append((0, i, path, values[i]))                                        # honest
        cases.append((0, i, path, (values[i] + 1) % P))                              # altered leaf
        cases.append((1, i, path, values[i]))                                        # wrong root
        cases.append((0, i ^ 1, path, values[i]))                                    # wrong index
        for d in range(logn):                                                        # each digest of the path altered
            bad = list(path)
            bad[d] = bytes([bad[d][0] ^ 1]) + bad[d][1:]
            cases.append((0, i, bad, values[i]))
        cases.append((0, i, path, (values[i] + P) % (1 << 128)))                     # a value >= p (still below 2^128)
        cases.append((0, i, path, blake2b(b"%d" % values[i]).digest()))              # the leaf given as its digest (Merkle.verify_)
        cases.append((0, i, path, blake2b(b"%d" % (values[i] + 3)).digest()))
    cases.append((0, n, path_of(levels, 0), values[0]))                              # position >= 2^depth: the host's assertion
    rows, digests, nd = [], [], 0
    for r, i, path, leaf in cases:
        if isinstance(leaf, bytes):
            digests.append(leaf)
            rows.append((i, nd + 1, r, len(path), sc.LEAF_DIGEST, fe16(nd)))
            nd += 1
        else:
            rows.append((i, nd, r, len(path), sc.LEAF_RESIDUE, fe16(leaf)))
        digests += path
        nd += len(path)
    got = run_merkle(emu, rows, digests, roots)
    for (r, i, path, leaf), v in zip(cases, got):
        try:
            want = Merkle.verify_(roots[r], i, path, leaf if isinstance(leaf, bytes) else blake2b(b"%d" % leaf).digest())
        except AssertionError:
            want = False
        assert bool(v) == want, (r, i, leaf)
    assert got.sum() >= 24 * 2


def test_colinearity_rows_match_host(emu):
    field = Field.main()
    rng = random.Random(71)
    rows, rounds, expect = [], [], []
    for n_log in (4, 8, 12):
        omega = field.primitive_nth_root(1 << n_log)
        offset = field.generator()
        alpha = FieldElement(rng.randrange(P), field)
        rounds.append(b"".join(fe16(e.value) for e in (offset, omega, alpha)))
        ridx = len(rounds) - 1
        half = 1 << (n_log - 1)
        for t in range(40):
            a = rng.randrange(half)
            b = a + half
            xa, xb = offset * (omega ^ a), offset * (omega ^ b)
            ya, yb = FieldElement(rng.randrange(P), field), FieldElement(rng.randrange(P), field)
            kind = t % 5
            if kind == 0:          # honest: y_c on the line through (x_a, y_a), (x_b, y_b) -- what the fold computes
                yc = ya + (yb - ya) / (xb - xa) * (alpha - xa)
            elif kind == 1:
                yc = FieldElement(rng.randrange(P), field)
            elif kind == 2:        # y_a == y_b: a constant, degree 0
                yb = ya
                yc = ya
            elif kind == 3:        # coinciding abscissas: undecided on the device
                b = a
                xb = xa
                yc = FieldElement(rng.randrange(P), field)
            else:                  # off by one
                yc = ya + (yb - ya) / (xb - xa) * (alpha - xa) + field.one()
            rows.append((a, b, ridx, fe16(ya.value) + fe16(yb.value) + fe16(yc.value)))
            expect.append((kind, test_colinearity([(xa, ya), (xb, yb), (alpha, yc)])))
    # a value that is not a canonical residue: undecided
    rows.append((1, 2, 0, fe16(P + 5) + fe16(3) + fe16(4)))
    expect.append((5, None))
    got = run_colinearity(emu, rows, rounds)
    for (kind, want), v in zip(expect, got):
        if kind in (3, 5):
            assert v == sc.UNDECIDED
        else:
            assert v in (0, 1) and bool(v) == want, kind
    assert sum(1 for (k, w) in expect if k == 0 and w) == sum(1 for (k, _), v in zip(expect, got) if k == 0 and v == 1) > 0


def test_colinearity_alpha_on_domain_is_undecided(emu):
    field = Field.main()
    omega, offset = field.primitive_nth_root(16), field.generator()
    xa = offset * (omega ^ 3)
    rounds = [b"".join(fe16(e.value) for e in (offset, omega, xa))]
    rows = [(3, 11, 0, fe16(1) + fe16(2) + fe16(1))]
    assert list(run_colinearity(emu, rows, rounds)) == [sc.UNDECIDED]

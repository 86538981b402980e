"""CPU walk of the Merkle forest (csrc/merkle_forest.cuh, compiled for the host by tests/emu/merkle_forest_emu.cpp) against hashlib
trees: the flat numbering of the forest's nodes, where each workgroup stores each level of each tree, the launch plan, the packing
of small trees into shared workgroups, and the query kernel's routing and path gather.  The device BLAKE2b does not compile for the
host, so the emulation hashes with the host compression of csrc/transcript.h; the indexing is the kernels' own."""
import ctypes
import os
import random
import subprocess
from hashlib import blake2b

import numpy as np
import pytest

from conftest import REPO
from algebra import Field

EMU_DIR = os.path.join(REPO, "tests", "emu")
P = Field.P_MAIN

# (leaves per tree, trees): N below, at and above 256 with count below and above 256
SHAPES = [(2, 1), (2, 257), (4, 3), (4, 64), (128, 3), (128, 257), (256, 1), (256, 64), (256, 257), (512, 3), (512, 257), (1 << 12, 1), (1 << 12, 64),
          (1 << 15, 3)]


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libmerkle_forest_emu.so")
    srcs = [os.path.join(EMU_DIR, "merkle_forest_emu.cpp")] + [os.path.join(REPO, "stark-anatomy_amd", "csrc", f)
                                                               for f in ("merkle_forest.cuh", "field.cuh", "transcript.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    lib.emu_forest_build.restype = ctypes.c_int
    lib.emu_forest_build.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_forest_query.restype = ctypes.c_int
    lib.emu_forest_query.argtypes = [ctypes.c_uint64] + [ctypes.c_void_p] * 8
    return lib


def values_of(n, count, seed):
    rng = random.Random(seed)
    rows = [[rng.randrange(P) for _ in range(n)] for _ in range(count)]
    rows[0][0], rows[-1][-1] = 0, P - 1
    return rows


def tree_levels(values):
    levels = [[blake2b(b"%d" % v).digest() for v in values]]
    while len(levels[-1]) > 1:
        lv = levels[-1]
        levels.append([blake2b(lv[i] + lv[i + 1]).digest() for i in range(0, len(lv), 2)])
    return levels


def build(emu, rows):
    count, n = len(rows), len(rows[0])
    elems = b"".join(v.to_bytes(16, "little") for row in rows for v in row)
    levels = np.zeros(count * 2 * n * 64, dtype=np.uint8)
    roots = np.zeros(count * 64, dtype=np.uint8)
    stats = (ctypes.c_uint64 * 3)()
    assert emu.emu_forest_build(elems, n, count, levels.ctypes.data, roots.ctypes.data, stats) == 0      # no store outside the forest, none twice
    return elems, levels, roots.tobytes(), list(stats)


@pytest.mark.parametrize("n,count", SHAPES)
def test_forest_levels_match_hashlib(emu, n, count):
    rows = values_of(n, count, 17 * n + count)
    _, levels, roots, stats = build(emu, rows)
    logn = n.bit_length() - 1
    raw = levels.tobytes()
    for t in (range(count) if n * count <= 1 << 16 else sorted({0, 1 % count, count // 2, count - 1})):
        want = tree_levels(rows[t])
        base = t * 2 * n
        for l, level in enumerate(want):
            off = base + (0 if l == 0 else 2 * n - (n >> (l - 1)))
            assert raw[64 * off:64 * (off + len(level))] == b"".join(level), (t, l)
        assert roots[64 * t:64 * t + 64] == want[-1][0]
    # the launch plan: eight levels per launch, 256 flat nodes per workgroup -- trees narrower than that share workgroups
    assert stats[0] == max(1, -(-logn // 8))
    assert stats[2] == -(-count * n // 256)
    if n < 256:
        assert stats[1] == stats[2]                    # small trees: one launch, 256 // n trees per workgroup from the leaves on


def test_forest_query_matches_hashlib(emu):
    rng = random.Random(5)
    shapes = [(2, 5), (128, 3), (256, 4), (1 << 12, 3)]
    forests, requests = [], []
    for n, count in shapes:
        rows = values_of(n, count, n + count)
        elems, levels, _, _ = build(emu, rows)
        positions = [(0, 0), (count - 1, n - 1), (count - 1, n - 1), (0, n - 1)] + [(rng.randrange(count), rng.randrange(n)) for _ in range(20)]
        forests.append((rows, elems, levels, n))
        requests.append(positions)
    requests[1] = []                                   # a pair nobody opens
    total = sum(map(len, requests))
    trees = (ctypes.c_uint64 * total)(*[t for req in requests for t, _ in req])
    indices = (ctypes.c_uint64 * total)(*[i for req in requests for _, i in req])
    path_digests = sum(len(req) * (f[3].bit_length() - 1) for f, req in zip(forests, requests))
    elems_out = np.zeros(16 * total, dtype=np.uint8)
    paths_out = np.zeros(64 * path_digests, dtype=np.uint8)
    k = len(forests)
    keep = [ctypes.create_string_buffer(f[1], len(f[1])) for f in forests]
    assert emu.emu_forest_query(k, (ctypes.c_void_p * k)(*[f[2].ctypes.data for f in forests]), (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in keep]),
                                (ctypes.c_uint64 * k)(*[f[3] for f in forests]), (ctypes.c_uint64 * k)(*map(len, requests)), trees, indices,
                                elems_out.ctypes.data, paths_out.ctypes.data) == 0
    got_e, got_p, eo, po = elems_out.tobytes(), paths_out.tobytes(), 0, 0
    for (rows, _, _, n), req in zip(forests, requests):
        depth = n.bit_length() - 1
        for t, i in req:
            want = tree_levels(rows[t])
            assert got_e[16 * eo:16 * eo + 16] == rows[t][i].to_bytes(16, "little")
            assert got_p[64 * po:64 * (po + depth)] == b"".join(want[l][(i >> l) ^ 1] for l in range(depth)), (n, t, i)
            eo += 1
            po += depth

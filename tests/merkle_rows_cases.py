"""Row commitments (csrc/merkle_rows.cuh): the hashlib model and the value matrices shared by
tests/test_merkle_rows_cpu.py and tests/test_gpu_merkle_rows.py.  Everything here is plain Python over hashlib: the row leaf is

    blake2b(b"".join(v.to_bytes(16, "little") for v in row), person=b"sc-merkle-row").digest()

and a node is blake2b(left + right).digest(), as in merkle.py."""
import functools
import random
from hashlib import blake2b

PERSON = b"sc-merkle-row"
P = 1 + 407 * (1 << 119)
SPECIAL = (0, 1, P - 1, 1 << 64, (1 << 64) - 1)
CPU_WIDTHS = tuple(range(1, 41)) + (128, 256)


def leaf(values):
    return blake2b(b"".join(v.to_bytes(16, "little") for v in values), person=PERSON).digest()


def pack(values):
    return b"".join(v.to_bytes(16, "little") for v in values)


def unpack(raw):
    return [int.from_bytes(raw[i:i + 16], "little") for i in range(0, len(raw), 16)]


def matrix(w, n, seed=0):
    """w columns of n residues: the first five rows hold the special values (0, 1, p - 1, 2^64, 2^64 - 1), displaced by one from
    column to column so that neighbouring columns never agree there and every column sees every one (from five rows up); the
    rest is random, different per column"""
    rng = random.Random(1000003 * w + 31 * n + seed)
    return [[SPECIAL[(r + c) % len(SPECIAL)] if r < len(SPECIAL) else rng.randrange(P) for r in range(n)] for c in range(w)]


def extremes(w, n):
    """columns that hold 0 throughout and columns that hold p - 1 throughout, alternating"""
    return [[0 if c % 2 == 0 else P - 1] * n for c in range(w)]


def levels(columns):
    """every level of the tree over the rows, leaves first, the root's level (one digest) last"""
    level = [leaf(row) for row in zip(*columns)]
    assert len(level) & (len(level) - 1) == 0 and level
    out = [level]
    while len(level) > 1:
        level = [blake2b(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
        out.append(level)
    return out


def path(tree_levels, index):
    return [level[(index >> l) ^ 1] for l, level in enumerate(tree_levels[:-1])]


def verify(root, index, auth_path, values):
    node = leaf(values)
    for sibling in auth_path:
        node = blake2b(node + sibling).digest() if index % 2 == 0 else blake2b(sibling + node).digest()
        index >>= 1
    return index == 0 and node == root


def packed_matrix(w, n, seed=0):
    """matrix(w, n) as packed columns (16 little-endian bytes per value); above 4096 rows the random part is drawn as bytes, the top
    bit of every value cleared (below 2^127 < p), which keeps a 2^18-row case at a second"""
    if n <= 4096:
        return [pack(column) for column in matrix(w, n, seed)]
    rng = random.Random(1000003 * w + 31 * n + seed)
    mask = (b"\xff" * 15 + b"\x7f") * n
    columns = []
    for c in range(w):
        body = (int.from_bytes(rng.randbytes(16 * n), "little") & int.from_bytes(mask, "little")).to_bytes(16 * n, "little")
        columns.append(pack([SPECIAL[(r + c) % len(SPECIAL)] for r in range(len(SPECIAL))]) + body[16 * len(SPECIAL):])
    return columns


def levels_packed(packed_columns):
    """levels() over packed columns"""
    n = len(packed_columns[0]) // 16
    level = [blake2b(b"".join(column[16 * i:16 * i + 16] for column in packed_columns), person=PERSON).digest() for i in range(n)]
    out = [level]
    while len(level) > 1:
        level = [blake2b(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
        out.append(level)
    return out


def row_of(packed_columns, index):
    return b"".join(column[16 * index:16 * index + 16] for column in packed_columns)


@functools.lru_cache(maxsize=None)
def reference(w, n, kind="matrix"):
    """(packed columns, levels) of a case, computed once and shared (callers leave both unchanged)"""
    columns = packed_matrix(w, n) if kind == "matrix" else [pack(column) for column in extremes(w, n)]
    return columns, levels_packed(columns)

"""Row forests (csrc/merkle_forest.cuh + csrc/merkle_rows.cuh): case builders shared by tests/test_row_forest_cpu.py,
tests/test_gpu_row_forest.py and tests/test_gpu_row_forest_proofs.py.  The model is tests/merkle_rows_cases.py's (hashlib); what is
added here is the layout a row forest reads its values from: up to eight segments, segment s a matrix of count * per_tree[s] columns
`pitch` elements apart, tree t's columns being columns t * per_tree[s] ... of every segment in turn.  Values differ per (tree, column):
a lane that reads a neighbour tree's column, a wrong segment or the padding between two columns changes a root."""
import functools
import random

import merkle_rows_cases as cases

LAYOUTS = ((1,), (3, 1), (7, 3), (5, 6), (8,), (8, 1), (16, 1), (1,) * 8)
FILLER = b"\xA5" * 16                # what lies between two columns when pitch > N (never read)


def tree_columns(w, n, tree, kind="matrix"):
    """the w packed columns of tree `tree`"""
    if kind == "extremes":
        return [cases.pack(column) for column in cases.extremes(w, n)]
    if kind == "bytes":                  # (forests of hundreds of trees: random bytes below 2^127 < p, no special values)
        raw = random.Random(1000 * tree + 7).randbytes(16 * n * w)
        raw = (int.from_bytes(raw, "little") & int.from_bytes((b"\xff" * 15 + b"\x7f") * (n * w), "little")).to_bytes(16 * n * w, "little")
        return [raw[16 * n * c:16 * n * (c + 1)] for c in range(w)]
    return cases.packed_matrix(w, n, seed=1000 * tree + 7)


@functools.lru_cache(maxsize=None)
def forest(layout, n, count, pad=0, kind="matrix"):
    """(segment buffers, per_tree, pitch, columns per tree, levels per tree) of a forest of `count` trees of n rows whose columns lie in
    len(layout) segments, segment s holding layout[s] columns per tree, every column followed by `pad` filler elements.  Computed
    once and shared: callers leave it unchanged."""
    w = sum(layout)
    columns = [tree_columns(w, n, t, kind) for t in range(count)]
    buffers, first = [], 0
    for per in layout:
        buffers.append(b"".join(columns[t][first + j] + FILLER * pad for t in range(count) for j in range(per)))
        first += per
    levels = Levels(columns) if kind == "bytes" else [cases.levels_packed(columns[t]) for t in range(count)]
    return buffers, list(layout), n + pad, columns, levels


class Levels:
    """levels[t] of a large forest, computed when a test first asks for tree t"""

    def __init__(self, columns):
        self.columns, self.known = columns, {}

    def __getitem__(self, tree):
        if tree not in self.known:
            self.known[tree] = cases.levels_packed(self.columns[tree])
        return self.known[tree]


def roots(levels):
    return [tree[-1][0] for tree in levels]


def path(levels, tree, index):
    return b"".join(cases.path(levels[tree], index))


def row(columns, tree, index):
    return cases.row_of(columns[tree], index)

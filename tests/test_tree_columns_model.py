"""The column forms of the subproduct-tree kernels (tests/emu/polytree_columns_model.py mirrors the *_cols kernels of
csrc/polytree.cuh thread by thread: interleaved level arrays [2^l][K >> l][C'], the tree's tables indexed by flat >> logC)
against the oracle's restatement of the reference (code/ntt.py:82-130).  Pins the index arithmetic of the correlation,
combination, expand, load and store steps before it runs on a device.  CPU only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
from oracle import py_oracle as po
import polytree_columns_model as cm
import synth

P = po.P
ORDER = 128
ROOT = po.primitive_nth_root(ORDER)


def points_of(k):
    pts = synth.synth_ints(9400 + k, k)
    if k > 3:
        pts[2] = 0                    # 0 is also the padding leaves' value
    return pts


@pytest.mark.parametrize("cols", [1, 3, 4])
@pytest.mark.parametrize("k", [3, 5, 17])
def test_evaluate_columns_model_matches_oracle(k, cols):
    pts = points_of(k)
    t = cm.ColumnTree(pts)
    for m in sorted({0, 1, k, t.K, t.K + 1, 2 * t.K + 3}):
        columns = [synth.synth_ints(9500 + 10 * k + c, m) for c in range(cols)]
        got = t.evaluate_columns(columns, m)
        assert got == [[po.evaluate(f, x) for x in pts] for f in columns], (k, cols, m)


@pytest.mark.parametrize("cols", [1, 3, 4])
@pytest.mark.parametrize("k", [3, 5, 17])
def test_interpolate_columns_model_matches_oracle(k, cols):
    pts = points_of(k)
    t = cm.ColumnTree(pts)
    columns = [synth.synth_ints(9600 + 10 * k + c, k) for c in range(cols)]
    columns[-1] = [0] * k
    columns[0][1] = 0
    got = t.interpolate_columns(columns)
    assert got == [po.fast_interpolate(pts, v, ROOT, ORDER) for v in columns], (k, cols)
    assert got == [t.interpolate(v) for v in columns]


def test_single_point_and_padding_lanes():
    t = cm.ColumnTree([7])
    columns = [[3, 4, 5], [1, 0, 2], [0, 0, 9]]
    assert t.evaluate_columns(columns, 3) == [[po.evaluate(f, 7)] for f in columns]
    assert t.interpolate_columns([[5], [0], [P - 1]]) == [[5], [0], [P - 1]]
    assert cm.lanes_log(1) == 0 and cm.lanes_log(2) == 1 and cm.lanes_log(3) == 2 and cm.lanes_log(4) == 2 and cm.lanes_log(5) == 3


def test_repeated_point_is_a_division_by_zero():
    t = cm.ColumnTree([5, 9, 5, 11, 2])
    with pytest.raises(AssertionError, match="divide by zero"):
        t.interpolate_columns([[1, 2, 3, 4, 5]] * 2)
    f = [[4, 0, 1, 7], [1, 1, 1, 1]]
    assert t.evaluate_columns(f, 4) == [[po.evaluate(g, x) for x in [5, 9, 5, 11, 2]] for g in f]

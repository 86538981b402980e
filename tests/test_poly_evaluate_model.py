"""The direct evaluation the device runs (tests/emu/poly_evaluate_model.py mirrors both forms of the kernel of csrc/polyeval.cuh and
the launch that combines the chunks, array by array) against plain Horner on Python integers (tests/emu/poly_evaluate_cases.py), and
the Lagrange formula with inverse(0) = 0 that sc_polytree_interpolate_lagrange_columns_dev serves against the host method's own
body.  Pins the chunking, the Horner stride, the per-thread tails, the split of the points between the two forms.  CPU only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
from oracle import py_oracle as po
import poly_evaluate_cases as cases
import poly_evaluate_model as pem

P = po.P
LOG = cases.MODEL_CHUNK_LOG


@pytest.mark.parametrize("m", cases.lengths(LOG))
@pytest.mark.parametrize("pattern", cases.COLUMN_PATTERNS)
def test_model_equals_horner(m, pattern):
    coeffs = list(cases.column(pattern, m))
    for k in cases.MODEL_POINT_COUNTS:
        xs = list(cases.points(LOG)[:k])
        got = pem.eval_points_model([coeffs], xs, chunk_log=LOG)
        assert got == [list(cases.values(pattern, m, 0, LOG, k))], (m, k, pattern)


def test_both_forms_agree_on_either_side_of_the_threshold():
    m = 3 * (1 << LOG) + 1
    coeffs = list(cases.column("random", m))
    for k in (31, 32, 65):
        xs = list(cases.points(LOG)[:k])
        want = list(cases.values("random", m, 0, LOG, k))
        for across_min, products_log, kb in ((1, 0, k), (32, 0, {31: 0, 32: 32, 65: 64}[k]), (32, 26, 0), (1 << 30, 0, 0)):
            trace = {}
            assert pem.eval_points_model([coeffs], xs, chunk_log=LOG, across_min=across_min, products_log=products_log, trace=trace) == [want]
            assert trace["kb"] == kb, (k, across_min, products_log)
    # in a call that fills the device -- 31 points: coefficients across lanes; 32: points across lanes; 65: one whole wave of points
    # and a single point the other way; 95: the rest of 31 goes the other way; 96: the rest of 32 stays
    big = 1 << pem.ACROSS_MIN_PRODUCTS_LOG
    assert [pem.across(k, big) for k in (1, 31, 32, 64, 65, 95, 96, 257)] == [0, 0, 32, 64, 64, 64, 96, 256]
    # a smaller call spreads every chunk over a workgroup, unless the second key is lowered (the tests' way to either form)
    assert pem.across(257, big - 1) == 0 and pem.across(257, 1, products_log=0) == 256
    assert pem.across(257, 1, across_min=1, products_log=0) == 257 and pem.across(257, big, across_min=1 << 30) == 0


def test_columns_share_the_points():
    m, k = (1 << LOG) + 1, 5
    columns = [list(cases.column(p, m, w)) for p, w in cases.matrix(m, 3, "random")]
    want = [list(cases.values(p, m, w, LOG, k)) for p, w in cases.matrix(m, 3, "random")]
    assert pem.eval_points_model(columns, list(cases.points(LOG)[:k]), chunk_log=LOG) == want


def test_cases_reach_what_they_name():
    chunk = 1 << LOG
    plans = {m: pem.plan(m, 1, 1, chunk_log=LOG) for m in cases.lengths(LOG) if m}
    # a single chunk (the second launch is skipped), a chunk boundary at m, several chunks with a partial last one
    assert [plans[m][3] for m in (1, 63, chunk - 1, chunk, chunk + 1, 3 * chunk + 1)] == [1, 1, 1, 1, 2, 4]
    assert all(p[2] == LOG for p in plans.values())
    # per-thread tails: m below one wave leaves most threads without a coefficient; chunk - 1 costs the last thread its top step
    trace = {}
    pem.eval_points_model([list(cases.column("random", 63))], [3], chunk_log=LOG, trace=trace)
    assert trace["steps"] == [1] * 63 + [0] * (pem.T - 63) and trace["G"] == 1
    pem.eval_points_model([list(cases.column("random", chunk - 1))], [3], chunk_log=LOG, trace=trace)
    assert trace["steps"] == [chunk // pem.T] * (pem.T - 1) + [chunk // pem.T - 1]
    pem.eval_points_model([list(cases.column("random", 3 * chunk + 1))], [3, 4, 5], chunk_log=LOG, trace=trace)
    assert trace["steps"] == [1] + [0] * (pem.T - 1) and trace["chunks"] == 4 and trace["G"] == 4      # the last chunk: one coefficient
    # groups of points: one, two, then fours whose last repeats a point it does not store
    assert [pem.plan(chunk, k, 1, LOG)[1] for k in (1, 2, 3, 5, 31)] == [1, 2, 4, 4, 4]
    # the special points are what they are called
    xs = cases.points(LOG)
    assert xs[1:4] == (0, 1, P - 1) and pow(xs[4], 256, P) == 1 and pow(xs[4], 128, P) != 1
    assert pow(xs[5], chunk, P) == P - 1 and xs[6] == xs[0] and len(set(xs)) == len(xs) - 1


def test_chunks_grow_where_points_and_columns_fill_the_device():
    # one point: 1 024 workgroups of four waves; many points and columns: fewer, longer chunks (fewer partials); a short
    # polynomial: the floor of one Horner stride per chunk; never more chunks than waves wanted
    assert pem.plan(1 << 24, 1, 1) == (0, 1, 14, 1024)
    assert pem.plan(1 << 24, 1024, 16) == (1024, 4, 18, 64)
    assert pem.plan(1 << 16, 1, 1) == (0, 1, 8, 256)
    assert pem.plan(1 << 12, 1024, 1) == (0, 4, 10, 4)                 # 2^22 products: too few to go points-across-lanes
    assert pem.plan(1 << 14, 4096, 1) == (4096, 4, 8, 64)
    assert pem.plan(1 << 20, 4096, 1) == (4096, 4, 12, 256)
    assert pem.plan(1 << 32, 1, 1) == (0, 1, 22, 1024)
    # results do not depend on the chunk length
    coeffs, xs = list(cases.column("random", 1537)), list(cases.points(LOG)[:3])
    assert pem.eval_points_model([coeffs], xs, chunk_log=8) == pem.eval_points_model([coeffs], xs, chunk_log=12) == pem.eval_points_model([coeffs], xs)


def test_degenerate_shapes():
    assert pem.eval_points_model([[], []], [1, 2, 3]) == [[0, 0, 0], [0, 0, 0]]
    assert pem.eval_points_model([[5, 6]], []) == [[]]
    assert pem.eval_points_model([], [1]) == []


@pytest.mark.parametrize("k", cases.LAGRANGE_COUNTS)
def test_inv0_formula_is_the_host_method(k):
    from algebra import Field, FieldElement
    from univariate import Polynomial
    field = Field.main()
    host = Polynomial._interpolate_domain_host
    for label, xs in cases.lagrange_patterns(k):
        for ys in cases.lagrange_values(k, 2):
            want = cases.lagrange_expected(xs, ys)
            assert pem.lagrange_inv0(xs, ys) == want, (k, label)
            got = host([FieldElement(x, field) for x in xs], [FieldElement(y, field) for y in ys])
            assert [c.value for c in got.coefficients] == want, (k, label)

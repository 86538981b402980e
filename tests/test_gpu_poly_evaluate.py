"""GPU tests of the evaluation, interpolation and zerofier routes of Polynomial: sc_poly_eval_points_dev / sc_poly_eval_points
(csrc/polyeval.cuh), sc_polytree_interpolate_lagrange_columns_dev / sc_interpolate_lagrange (csrc/polytree.cuh), the ntt-level
functions, DevicePolynomial.evaluate / evaluate_points and the hand-over of Polynomial.evaluate_domain / interpolate_domain /
zerofier_domain.  Every comparison is exact: the expectations are Python integers (plain Horner, the Lagrange formula with
inverse(0) = 0: tests/emu/poly_evaluate_cases.py, shared with the host model's test) or the host methods' own bodies.  Outputs sit
in sentinel-filled buffers with guard elements behind them, matrices have non-zero junk between a column's length and its stride."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
from oracle import py_oracle as po
import poly_evaluate_cases as cases
import synth

pytestmark = pytest.mark.gpu
P = po.P
SENTINEL = (0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5).to_bytes(16, "little")       # a canonical residue no test value equals
SC_ERR_DIV_ZERO, SC_ERR_BAD_ARG = -5, -6
GUARD = 3
LOG = cases.GPU_CHUNK_LOG
# sc_set_tuning("eval_points_across_min"), ("eval_across_min_products_log")
FORMS = {"default": (32, 26), "points across lanes": (1, 0), "coefficients across lanes": (1 << 30, 26)}


def set_form(sc, least=32, products_log=26):
    sc.set_tuning("eval_points_across_min", least)
    sc.set_tuning("eval_across_min_products_log", products_log)


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    starkcore.set_tuning("eval_chunk_log", LOG)
    yield starkcore
    starkcore.set_tuning("eval_chunk_log", 8)
    set_form(starkcore)


def matrix_of(sc, rows, n, ld):
    """the rows (lists of n ints) as a device matrix of pitch ld with non-zero junk in the gaps"""
    junk = synth.pack_ints([v or 1 for v in synth.synth_ints(4991, ld - n)])
    return sc.DeviceVector.from_bytes(b"".join(synth.pack_ints(list(r)) + junk for r in rows) or SENTINEL)


def dev_eval(sc, columns, xs, ld_in, ld_out, stream=None):
    """sc_poly_eval_points_dev on a junk-padded matrix -> [bytes of k values per column]; the gaps and the guard must stay sentinels"""
    cols, m, k = len(columns), len(columns[0]), len(xs)
    src, pts = matrix_of(sc, columns, m, ld_in), sc.DeviceVector.from_ints(xs)
    out = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out + GUARD))
    sc._check(sc.lib().sc_poly_eval_points_dev(src.ptr, m, ld_in, cols, pts.ptr, k, out.ptr, ld_out, stream))
    raw = out.to_bytes()
    assert raw[16 * cols * ld_out:] == SENTINEL * GUARD, "written past the end"
    assert all(raw[16 * (ld_out * c + k):16 * ld_out * (c + 1)] == SENTINEL * (ld_out - k) for c in range(cols)), "a gap of the output was written"
    return [raw[16 * ld_out * c:16 * (ld_out * c + k)] for c in range(cols)]


@pytest.mark.parametrize("m", cases.lengths(LOG))
def test_values_are_horner(sc, m):
    """every m against every k, one and three columns at strides above their lengths, the three coefficient patterns, each form
    forced: the bytes are Horner's and the same in every form"""
    try:
        for k in cases.GPU_POINT_COUNTS:
            xs = list(cases.points(LOG)[:k])
            for cols in (1, 3):
                for lead in cases.COLUMN_PATTERNS:
                    layout = cases.matrix(m, cols, lead)
                    columns = [list(cases.column(p, m, w)) for p, w in layout]
                    want = [synth.pack_ints(cases.values(p, m, w, LOG, k)) for p, w in layout]
                    seen = {}
                    for form, keys in FORMS.items():
                        set_form(sc, *keys)
                        seen[form] = dev_eval(sc, columns, xs, m + 3, k + 2)
                        assert seen[form] == want, (m, k, cols, lead, form)
                    assert seen["points across lanes"] == seen["coefficients across lanes"]
    finally:
        set_form(sc)


def test_results_do_not_depend_on_the_chunk_length(sc):
    m, k = 3 * (1 << LOG) + 1, 5
    columns, xs = [list(cases.column("random", m))], list(cases.points(LOG)[:k])
    try:
        for log in (8, 9, 12):
            sc.set_tuning("eval_chunk_log", log)
            assert dev_eval(sc, columns, xs, m, k) == [synth.pack_ints(cases.values("random", m, 0, LOG, k))], log
    finally:
        sc.set_tuning("eval_chunk_log", LOG)


def test_return_codes_leave_the_output_alone(sc):
    lib = sc.lib()
    m, k = 70, 5
    src = sc.DeviceVector.from_ints(list(cases.column("random", 2 * m)))
    pts = sc.DeviceVector.from_ints(list(cases.points(LOG)[:k]))
    out = sc.DeviceVector.from_bytes(SENTINEL * (2 * k + GUARD))
    null = None
    assert lib.sc_poly_eval_points_dev(null, m, m, 1, pts.ptr, k, out.ptr, k, None) == SC_ERR_BAD_ARG
    assert lib.sc_poly_eval_points_dev(src.ptr, m, m, 1, null, k, out.ptr, k, None) == SC_ERR_BAD_ARG
    assert lib.sc_poly_eval_points_dev(src.ptr, m, m, 1, pts.ptr, k, null, k, None) == SC_ERR_BAD_ARG
    assert lib.sc_poly_eval_points_dev(src.ptr, m, m - 1, 2, pts.ptr, k, out.ptr, k, None) == SC_ERR_BAD_ARG      # ld_in < m
    assert lib.sc_poly_eval_points_dev(src.ptr, m, m, 2, pts.ptr, k, out.ptr, k - 1, None) == SC_ERR_BAD_ARG      # ld_out < k
    assert lib.sc_poly_eval_points_dev(src.ptr, (1 << 32) + 1, m, 1, pts.ptr, k, out.ptr, k, None) == SC_ERR_BAD_ARG
    assert lib.sc_poly_eval_points_dev(src.ptr, m, m, 1 << 31, pts.ptr, k, out.ptr, k, None) == SC_ERR_BAD_ARG    # k * cols > 2^32
    # an output inside the coefficients, one that ends on the first point
    assert lib.sc_poly_eval_points_dev(src.ptr, m, m, 1, pts.ptr, k, ctypes.c_void_p(int(src.ptr) + 16 * (m - 1)), k, None) == SC_ERR_BAD_ARG
    assert lib.sc_poly_eval_points_dev(src.ptr, m, m, 1, pts.ptr, k, ctypes.c_void_p(int(pts.ptr) - 16 * (k - 1)), k, None) == SC_ERR_BAD_ARG
    assert "overlap" in lib.sc_last_error().decode()
    # nothing to do: SC_OK, nothing enqueued
    assert lib.sc_poly_eval_points_dev(src.ptr, m, m, 1, pts.ptr, 0, out.ptr, k, None) == 0
    assert lib.sc_poly_eval_points_dev(src.ptr, m, m, 0, pts.ptr, k, out.ptr, k, None) == 0
    sc.synchronize()
    assert out.to_bytes() == SENTINEL * (2 * k + GUARD)
    # an output that ends right in front of the coefficients is no overlap
    both = sc.DeviceVector.from_bytes(SENTINEL * k + synth.pack_ints(list(cases.column("random", m))))
    sc._check(lib.sc_poly_eval_points_dev(ctypes.c_void_p(int(both.ptr) + 16 * k), m, m, 1, pts.ptr, k, both.ptr, k, None))
    assert both.to_bytes(0, k) == synth.pack_ints(cases.values("random", m, 0, LOG, k))


@pytest.mark.parametrize("m,k", [(65, 3), (3 * (1 << LOG) + 1, 65)])
def test_host_form(sc, m, k):
    out = ctypes.create_string_buffer(SENTINEL * (k + GUARD), 16 * (k + GUARD))
    sc._check(sc.lib().sc_poly_eval_points(synth.pack_ints(list(cases.column("random", m))), m, synth.pack_ints(list(cases.points(LOG)[:k])), k, out))
    assert out.raw == synth.pack_ints(cases.values("random", m, 0, LOG, k)) + SENTINEL * GUARD


def test_two_calls_in_flight_on_two_streams(sc):
    """include/starkcore.h: the temporaries are the call's own, no one-stream rule.  Two calls of different shapes (several chunks
    each, both forms) are computed one at a time on the library's stream first, then enqueued on two caller streams with no host wait
    in between, the operands copied into place ON the stream that uses them: the same bytes, sentinels included."""
    import torch
    lib = sc.lib()
    shapes = [(3 * (1 << LOG) + 1, 65, 3), ((1 << LOG) + 1, 3, 1)]
    jobs = []
    for m, k, cols in shapes:
        layout = cases.matrix(m, cols, "random")
        columns, xs = [list(cases.column(p, m, w)) for p, w in layout], list(cases.points(LOG)[:k])
        ld_in, ld_out = m + 3, k + 2
        single = dev_eval(sc, columns, xs, ld_in, ld_out)
        assert single == [synth.pack_ints(cases.values(p, m, w, LOG, k)) for p, w in layout]
        staged = [matrix_of(sc, columns, m, ld_in), sc.DeviceVector.from_ints(xs)]
        operands = [sc.DeviceVector(v.n) for v in staged]
        want = b"".join(x + SENTINEL * (ld_out - k) for x in single) + SENTINEL * GUARD
        jobs.append((m, k, cols, ld_in, ld_out, staged, operands, sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out + GUARD)), want))
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    sc.synchronize()
    set_form(sc, 32, 0)                                         # 65 points: a wave of them across lanes, one the other way
    for rnd in range(2):                                        # the second round finds the first one's temporaries in the pool
        for i, (m, k, cols, ld_in, ld_out, staged, operands, out, want) in enumerate(jobs):
            h = ctypes.c_void_p(streams[(i + rnd) % 2].cuda_stream)
            for dst, src in zip(operands, staged):
                sc._check(lib.sc_memcpy_dev(ctypes.c_void_p(int(dst.ptr)), ctypes.c_void_p(int(src.ptr)), src.n, h))
            sc._check(lib.sc_poly_eval_points_dev(operands[0].ptr, m, ld_in, cols, operands[1].ptr, k, out.ptr, ld_out, h))
        torch.cuda.synchronize()
        for job in jobs:
            out, want = job[7], job[8]
            assert out.to_bytes() == want, (rnd, job[:3])
            sc._check(lib.sc_vec_upload(out._h, 0, SENTINEL * out.n, out.n))
        sc.synchronize()
    set_form(sc)


def test_a_call_that_fills_the_device_goes_points_across_lanes(sc):
    """2^14 coefficients at 4 101 points: 2^26 products, so the library itself takes the points-across-lanes form for the 64 whole
    waves and the other one for the last five points; the bytes are those of the coefficients-across-lanes form alone, and Horner's
    where they are sampled"""
    m, k = 1 << 14, 4096 + 5
    coeffs, xs = list(cases.column("random", m)), synth.synth_ints(7500, k)
    try:
        sc.set_tuning("eval_chunk_log", 8)
        own = dev_eval(sc, [coeffs], xs, m, k)
        set_form(sc, 1 << 30)
        assert dev_eval(sc, [coeffs], xs, m, k) == own
    finally:
        set_form(sc)
        sc.set_tuning("eval_chunk_log", LOG)
    for j in (0, 63, 4095, 4096, k - 1):
        assert own[0][16 * j:16 * (j + 1)] == synth.pack_ints([cases.horner(coeffs, xs[j])]), j


# ---- interpolation with inverse(0) = 0

def dev_lagrange(sc, tree, value_columns, ld_in, ld_out, entry="sc_polytree_interpolate_lagrange_columns_dev"):
    cols, k = len(value_columns), tree.k
    src = matrix_of(sc, value_columns, k, ld_in)
    out = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out + GUARD))
    rc = getattr(sc.lib(), entry)(tree._h, src.ptr, ld_in, cols, out.ptr, ld_out, None)
    raw = out.to_bytes()
    assert raw[16 * cols * ld_out:] == SENTINEL * GUARD, "written past the end"
    if rc != 0:
        assert raw == SENTINEL * (cols * ld_out + GUARD), "a refused call wrote"
        return rc
    assert all(raw[16 * (ld_out * c + k):16 * ld_out * (c + 1)] == SENTINEL * (ld_out - k) for c in range(cols)), "a gap of the output was written"
    return [raw[16 * ld_out * c:16 * (ld_out * c + k)] for c in range(cols)]


@pytest.mark.parametrize("k", cases.LAGRANGE_COUNTS)
def test_lagrange_entries(sc, k):
    for label, xs in cases.lagrange_patterns(k):
        tree = sc.PolyTree(synth.pack_ints(xs))
        for cols in (1, 3):
            # one column: all zeros, then random values; three columns: those and another random one, at strides above k
            for value_columns in ([[v] for v in cases.lagrange_values(k, 2)] if cols == 1 else [cases.lagrange_values(k, 3)]):
                want = [synth.pack_ints(cases.lagrange_expected(xs, v)) for v in value_columns]
                ld_in, ld_out = (k, k) if cols == 1 else (k + 2, k + 3)
                assert dev_lagrange(sc, tree, value_columns, ld_in, ld_out) == want, (k, label, cols)
                plain = dev_lagrange(sc, tree, value_columns, ld_in, ld_out, "sc_polytree_interpolate_columns_dev")
                if len(set(xs)) == k:
                    assert plain == want, (k, label)                           # distinct points: the same bytes
                elif k > 1:
                    assert plain == SC_ERR_DIV_ZERO, (k, label)                # the existing entry keeps its contract on this tree
        if k > 1 and len(set(xs)) < k:
            vals, out = sc.DeviceVector.from_ints(cases.lagrange_values(k, 2)[1]), sc.DeviceVector.from_bytes(SENTINEL * k)
            assert sc.lib().sc_polytree_interpolate_dev(tree._h, vals.ptr, out.ptr, None) == SC_ERR_DIV_ZERO, (k, label)
            ys = cases.lagrange_values(k, 2)[1]
            assert dev_lagrange(sc, tree, [ys], k, k) == [synth.pack_ints(cases.lagrange_expected(xs, ys))]      # and the new one its own
        host = ctypes.create_string_buffer(16 * k)
        ys = cases.lagrange_values(k, 2)[1]
        sc._check(sc.lib().sc_interpolate_lagrange(synth.pack_ints(xs), synth.pack_ints(ys), k, host))
        assert host.raw == synth.pack_ints(cases.lagrange_expected(xs, ys)), (k, label)
        tree.free()


def test_plain_weights_first_then_lagrange_shares_them(sc):
    k = 17
    xs = cases.lagrange_patterns(k)[0][1]
    ys = cases.lagrange_values(k, 2)[1]
    tree = sc.PolyTree(synth.pack_ints(xs))
    want = [synth.pack_ints(cases.lagrange_expected(xs, ys))]
    assert dev_lagrange(sc, tree, [ys], k, k, "sc_polytree_interpolate_columns_dev") == want
    assert dev_lagrange(sc, tree, [ys], k, k) == want
    assert tree.interpolate_lagrange(sc.DeviceVector.from_ints(ys)).to_bytes() == want[0]
    geo = sc.GeoDomain(3, 5, k)
    vals = sc.DeviceVector.from_ints(ys)
    assert geo.interpolate_lagrange(vals).to_bytes() == geo.interpolate(vals).to_bytes()
    assert geo.interpolate_lagrange_columns(vals, 1).to_bytes() == geo.interpolate_columns(vals, 1).to_bytes()


# ---- the Python layers

def _field():
    from algebra import Field
    return Field.main()


def _poly(ints, field=None):
    from algebra import FieldElement
    from univariate import Polynomial
    field = field or _field()
    return Polynomial([FieldElement(v, field) for v in ints])


def _elements(ints, field=None):
    from algebra import FieldElement
    field = field or _field()
    return [FieldElement(v, field) for v in ints]


def _same(got, want):
    """values AND list lengths"""
    return [c.value for c in got.coefficients] == [c.value for c in want.coefficients]


def _domains(n):
    """(label, points): a progression, arbitrary points, arbitrary points with a repeat"""
    f = _field()
    g = f.primitive_nth_root(1 << 12).value
    rnd = synth.synth_ints(7600 + n, n)
    rep = list(rnd)
    if n >= 2:
        rep[n - 1] = rep[0]
    return [("progression", [3 * pow(g, i, P) % P for i in range(n)]), ("arbitrary", rnd), ("with a repeated point", rep)]


def _check_methods(n, m):
    """the three methods against their host bodies at n points and a polynomial of degree m - 1 carrying two trailing zeros"""
    from univariate import Polynomial
    poly = _poly(synth.synth_ints(7700 + m, m) + [0, 0])
    for label, xs in _domains(n):
        domain, values = _elements(xs), _elements(synth.synth_ints(7800 + n, n))
        got = poly.evaluate_domain(domain)
        assert [v.value for v in got] == [v.value for v in poly._evaluate_domain_host(domain)] and len(got) == n, (n, m, label)
        assert _same(Polynomial.interpolate_domain(domain, values), Polynomial._interpolate_domain_host(domain, values)), (n, label)
        assert _same(Polynomial.interpolate_domain(domain, _elements([0] * n)), Polynomial._interpolate_domain_host(domain, _elements([0] * n))), (n, label)
        assert _same(Polynomial.zerofier_domain(domain), Polynomial._zerofier_domain_host(domain)), (n, label)


class Census:
    """the bound library with every call counted by name"""

    def __init__(self, lib):
        self.lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("sc_"):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


THRESHOLDS = ("FAST_EVAL_DOMAIN_MIN", "FAST_INTERPOLATE_MIN_POINTS", "FAST_ZEROFIER_MIN_POINTS")


def test_polynomial_methods_hand_over_at_four(sc, monkeypatch):
    import ntt
    from univariate import Polynomial
    for name in THRESHOLDS:
        monkeypatch.setattr(Polynomial, name, 4)
    monkeypatch.setattr(ntt, "EVAL_DIRECT_MAX_POINTS", 64)       # so that these small shapes reach both routes of fast_evaluate_domain
    monkeypatch.setattr(ntt, "EVAL_DIRECT_MAX_COEFFS", 64)
    census = Census(sc.lib())
    with monkeypatch.context() as mp:
        mp.setattr(sc, "lib", lambda: census)
        for n, m in ((4, 4), (5, 40), (33, 7), (70, 70), (100, 300)):
            _check_methods(n, m)
        _check_methods(3, 9)                                   # below the threshold: the host bodies themselves
    calls = census.calls
    assert calls.get("sc_poly_eval_points", 0) > 0 and calls.get("sc_polytree_interpolate_lagrange_columns_dev", 0) > 0
    assert calls.get("sc_polytree_evaluate_dev", 0) + calls.get("sc_geodomain_evaluate_dev", 0) > 0             # (100 points, 300 coefficients: the tree route)
    assert calls.get("sc_polytree_zerofier_dev", 0) > 0 and calls.get("sc_geodomain_zerofier_dev", 0) > 0
    # a long list whose DEGREE is below the threshold stays on the host
    census.calls.clear()
    with monkeypatch.context() as mp:
        mp.setattr(sc, "lib", lambda: census)
        short = _poly([1, 2, 3] + [0] * 20)
        domain = _elements(synth.synth_ints(7900, 8))
        assert [v.value for v in short.evaluate_domain(domain)] == [v.value for v in short._evaluate_domain_host(domain)]
    assert not census.calls


def test_polynomial_methods_at_their_committed_thresholds(sc, monkeypatch):
    """just below and at each threshold that is switched on (10**9: switched off, nothing to run)"""
    from univariate import Polynomial
    assert all(getattr(Polynomial, name) >= 32 for name in THRESHOLDS)
    marks = sorted({getattr(Polynomial, name) for name in THRESHOLDS if getattr(Polynomial, name) < 10**9})
    census = Census(sc.lib())
    with monkeypatch.context() as mp:
        mp.setattr(sc, "lib", lambda: census)
        for mark in marks:
            _check_methods(mark - 1, mark - 1)
            _check_methods(mark, mark)
    assert bool(census.calls) == bool(marks)


def test_another_field_takes_the_host_bodies(sc, monkeypatch):
    from algebra import Field
    from univariate import Polynomial
    for name in THRESHOLDS:
        monkeypatch.setattr(Polynomial, name, 4)
    small = Field(97)
    poly = _poly(list(range(1, 12)), small)
    domain, values = _elements(list(range(2, 10)), small), _elements(list(range(20, 28)), small)
    census = Census(sc.lib())
    with monkeypatch.context() as mp:
        mp.setattr(sc, "lib", lambda: census)
        assert [v.value for v in poly.evaluate_domain(domain)] == [v.value for v in poly._evaluate_domain_host(domain)]
        assert _same(Polynomial.interpolate_domain(domain, values), Polynomial._interpolate_domain_host(domain, values))
        assert _same(Polynomial.zerofier_domain(domain), Polynomial._zerofier_domain_host(domain))
    assert not census.calls


def test_ntt_level_functions(sc, monkeypatch):
    import ntt
    from univariate import Polynomial
    monkeypatch.setattr(ntt, "EVAL_DIRECT_MAX_POINTS", 64)       # 100 points by 300 coefficients: the tree route; everything smaller: direct
    monkeypatch.setattr(ntt, "EVAL_DIRECT_MAX_COEFFS", 64)
    polys = [_poly(synth.synth_ints(8000 + c, n) + [0] * c) for c, n in enumerate((300, 1, 0, 77))]
    for n in (1, 5, 70, 100):
        for label, xs in _domains(n):
            domain = _elements(xs)
            want = [p._evaluate_domain_host(domain) for p in polys]
            got = ntt.fast_evaluate_domain_columns(polys, domain)
            assert [[v.value for v in col] for col in got] == [[v.value for v in col] for col in want], (n, label)
            assert [v.value for v in ntt.fast_evaluate_domain(polys[0], domain)] == [v.value for v in want[0]], (n, label)
            value_lists = [_elements(synth.synth_ints(8100 + c, n)) for c in range(3)]
            got = ntt.fast_interpolate_domain_columns(domain, value_lists)
            assert all(_same(g, Polynomial._interpolate_domain_host(domain, v)) for g, v in zip(got, value_lists)), (n, label)
            assert _same(ntt.fast_zerofier_domain(domain), Polynomial._zerofier_domain_host(domain)), (n, label)
    assert ntt.fast_evaluate_domain(polys[0], []) == [] and ntt.fast_evaluate_domain_columns(polys, []) == [[], [], [], []]


def test_device_polynomial_evaluate(sc, monkeypatch):
    import ntt
    f = _field()
    poly = _poly(synth.synth_ints(8200, 5000))
    resident = ntt.DevicePolynomial.from_polynomial(poly)
    xs = _elements([0, 1, P - 1] + synth.synth_ints(8201, 97))
    assert resident.evaluate(xs[5]).value == poly.evaluate(xs[5]).value and resident.evaluate(xs[5]).field is xs[5].field
    assert resident.evaluate(xs[0]).value == poly.coefficients[0].value
    want = [poly.evaluate(x).value for x in xs]
    got = resident.evaluate_points(xs)
    assert got.n == len(xs) and sc.unpack(got.to_bytes()) == want
    domain = ntt.DeviceDomain(xs)                              # arbitrary points: the tree keeps them
    assert sc.unpack(resident.evaluate_points(domain).to_bytes()) == want
    g = f.primitive_nth_root(64)
    progression = ntt.DeviceDomain.geometric(xs[4], g, 33)     # a progression keeps none: made on demand
    assert sc.unpack(resident.evaluate_points(progression).to_bytes()) == [poly.evaluate(xs[4] * (g ^ i)).value for i in range(33)]
    # many resident polynomials in one call: rows of one matrix where they lie, others copied, an empty one
    rows = ntt.DevicePolynomial.rows_from_polynomials([_poly(synth.synth_ints(8300 + c, 40 + c)) for c in range(3)], f)
    census = Census(sc.lib())
    with monkeypatch.context() as mp:
        mp.setattr(sc, "lib", lambda: census)
        got = ntt.evaluate_points_device(rows, xs[:7])
    assert census.calls.get("sc_memcpy_dev", 0) == 0 and census.calls.get("sc_poly_eval_points_dev", 0) == 1
    assert [sc.unpack(v.to_bytes()) for v in got] == [[r.to_polynomial().evaluate(x).value for x in xs[:7]] for r in rows]
    mixed = [resident, rows[1], ntt.DevicePolynomial(sc.DeviceVector(1), f, 0)]
    got = ntt.evaluate_points_device(mixed, xs[:7])
    assert [sc.unpack(v.to_bytes()) for v in got] == [want[:7], [rows[1].to_polynomial().evaluate(x).value for x in xs[:7]], [0] * 7]
    assert ntt.evaluate_points_device([], xs) == []


def test_fast_stark_with_forty_pinned_cells(sc, monkeypatch):
    """the synthetic instance at FRI 2^12 with 40 cells of register 0 pinned at irregular cycles: the proof with the three methods
    handed over at 4 points is the proof with them switched off, byte for byte, and both verify"""
    import workloads
    from algebra import FieldElement
    from fast_stark import FastStark
    from univariate import Polynomial
    s = 2
    field, T, _, air, boundary = workloads.synthetic_stark_instance(12, s)
    col_a, col_b = synth.synthetic_air_columns(T)
    rows = [[FieldElement(a, field), FieldElement(b, field)] for a, b in zip(col_a, col_b)]
    cycles = sorted(random.Random(41).sample(range(1, T - 1), 40))
    boundary = boundary + [(c, 0, FieldElement(col_a[c], field)) for c in cycles]
    stark = FastStark(field, 4, s, 2 * s, 2, T)
    assert stark.fri_domain_length == 1 << 12
    zerofier, codeword, root = stark.preprocess()
    proofs = {}
    for least in (4, 10**9):
        with monkeypatch.context() as mp:
            for name in THRESHOLDS:
                mp.setattr(Polynomial, name, least)
            rng = random.Random(4242)
            mp.setattr(os, "urandom", lambda n: bytes(rng.getrandbits(8) for _ in range(n)))
            census = Census(sc.lib())
            mp.setattr(sc, "lib", lambda: census)
            proofs[least] = stark.prove([list(r) for r in rows], air, boundary, zerofier, codeword)
            assert stark.verify(proofs[least], air, boundary, root)
            used = census.calls.get("sc_polytree_interpolate_lagrange_columns_dev", 0)
            assert (used > 0) == (least == 4)
    assert proofs[4] == proofs[10**9]

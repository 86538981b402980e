"""GPU tests of interpolation on a geometric progression for MANY COLUMNS per call (sc_geodomain_interpolate_columns_dev,
csrc/geoseq.cuh) and of the degrees of many coefficient vectors per call (sc_vec_degree_columns_dev): bit for bit the single-column
entries' results, whatever the strides, the number of columns and the first point; the set split above 65 536 columns; the
reference's golden interpolation on the trace domain; the subproduct tree on the same points; refused arguments."""
import ctypes

import pytest

from conftest import load_golden
from oracle import py_oracle as po
import synth

pytestmark = pytest.mark.gpu
P = po.P
SENTINEL = (0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5).to_bytes(16, "little")       # a canonical residue no test value equals
SC_ERR_BAD_ARG = -6


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


def single(sc, dom, values):
    """one column through sc_geodomain_interpolate_dev -> packed coefficients"""
    return dom.interpolate(sc.DeviceVector.from_bytes(values)).to_bytes()


def in_columns(sc, dom, columns, ld_in, ld_out):
    """`columns` (packed bytes each) through ONE sc_geodomain_interpolate_columns_dev with the given strides; the gaps of the input
    hold non-zero junk, the whole output is pre-filled with SENTINEL.  Returns the output matrix as bytes."""
    n, cols = dom.k, len(columns)
    junk = synth.pack_ints(synth.synth_ints(991, ld_in - n))
    src = sc.DeviceVector.from_bytes(b"".join(c + junk for c in columns))
    out = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out))
    sc._check(sc.lib().sc_geodomain_interpolate_columns_dev(dom._h, src.ptr, ld_in, cols, out.ptr, ld_out, None))
    return out.to_bytes()


@pytest.mark.parametrize("n", [2, 3, 5, 36, 64, 284, 1000])
def test_columns_equal_the_single_column_entry_bit_for_bit(sc, n):
    ratio = po.primitive_nth_root(2048)                     # order >= 2 n for every n here: the points are distinct
    for first in (1, po.GENERATOR):                         # first point != 1: the c^-j power tables
        dom = sc.GeoDomain(first, ratio, n)
        columns = [synth.synth_packed(9000 + 31 * n + c, n).tobytes() for c in range(17)]
        columns[1] = bytes(16 * n)                          # a zero column among them
        want = [single(sc, dom, c) for c in columns]        # computed once, shared by every shape below
        for cols in (1, 2, 3, 17):
            for ld_in in (n, n + 3):
                for ld_out in (n, n + 5):
                    got = in_columns(sc, dom, columns[:cols], ld_in, ld_out)
                    for c in range(cols):
                        row = got[16 * ld_out * c:16 * ld_out * (c + 1)]
                        assert row[:16 * n] == want[c], (n, first, cols, ld_in, ld_out, c)
                        assert row[16 * n:] == SENTINEL * (ld_out - n), "the gap of the output was written"
        dom.free()


def test_more_columns_than_one_set_holds(sc):
    """65 537 columns of two points (4 MB): the second set of launches (one column) starts where the first ended"""
    n, cols = 2, 65537
    first, ratio = po.GENERATOR, po.primitive_nth_root(8)
    dom = sc.GeoDomain(first, ratio, n)
    values = synth.synth_packed(9100, n * cols).tobytes()
    src = sc.DeviceVector.from_bytes(values)
    out = sc.DeviceVector(n * cols)
    sc._check(sc.lib().sc_geodomain_interpolate_columns_dev(dom._h, src.ptr, n, cols, out.ptr, n, None))
    got = out.to_bytes()
    for c in (0, 1, 65535, 65536):
        assert got[32 * c:32 * (c + 1)] == single(sc, dom, values[32 * c:32 * (c + 1)]), c
    # the line through (x0, v0), (x1, v1) in plain ints: a1 = (v1 - v0) / (x1 - x0), a0 = v0 - a1 x0
    x0, x1 = first, first * ratio % P
    slope = pow(x1 - x0, P - 2, P)
    v = synth.unpack_ints(values)
    want = []
    for c in range(cols):
        a1 = (v[2 * c + 1] - v[2 * c]) * slope % P
        want += [(v[2 * c] - a1 * x0) % P, a1]
    assert got == synth.pack_ints(want)
    dom.free()


def test_reference_golden_on_the_trace_domain_is_one_column_of_three(sc):
    """the reference's fast_interpolate on {omicron^i, i < 36}, omicron of order 128 (the record of tests/golden/poly.json that has
    `omicron_order`), as column 1 of three"""
    rec = [r for r in load_golden("poly.json")["interpolate"] if r.get("omicron_order") == 128 and r["k"] == 36]
    assert len(rec) == 1
    rec = rec[0]
    n = rec["k"]
    dom = sc.GeoDomain(1, po.primitive_nth_root(128), n)
    columns = [synth.synth_packed(9200, n).tobytes(), synth.pack_ints(synth.synth_ints(rec["val_seed"], n)), synth.synth_packed(9201, n).tobytes()]
    got = in_columns(sc, dom, columns, n, n)
    assert [str(v) for v in synth.unpack_ints(got[16 * n:32 * n])] == rec["out"]
    dom.free()


def test_columns_equal_the_subproduct_tree(sc):
    n, cols = 36, 3
    first, ratio = synth.synth_ints(9300, 2)
    points, x = [], first
    for _ in range(n):
        points.append(x)
        x = x * ratio % P
    dom, tree = sc.GeoDomain(first, ratio, n), sc.PolyTree(synth.pack_ints(points))
    columns = [synth.synth_packed(9301 + c, n).tobytes() for c in range(cols)]
    got = in_columns(sc, dom, columns, n, n)
    for c in range(cols):
        assert got[16 * n * c:16 * n * (c + 1)] == tree.interpolate(sc.DeviceVector.from_bytes(columns[c])).to_bytes(), c
    dom.free()
    tree.free()


def test_refused_arguments_enqueue_nothing_and_leave_the_library_usable(sc):
    n, cols = 36, 3
    dom = sc.GeoDomain(po.GENERATOR, po.primitive_nth_root(128), n)
    columns = [synth.synth_packed(9400 + c, n).tobytes() for c in range(cols)]
    want = b"".join(single(sc, dom, c) for c in columns)
    src = sc.DeviceVector.from_bytes(b"".join(columns))
    call = sc.lib().sc_geodomain_interpolate_columns_dev

    def still_right():
        assert in_columns(sc, dom, columns, n, n) == want
    out = sc.DeviceVector.from_bytes(SENTINEL * (cols * n))
    assert call(dom._h, src.ptr, n, 0, out.ptr, n, None) == 0                      # no columns: fine, and nothing happens
    still_right()
    for args in ((None, src.ptr, n, cols, out.ptr, n, None), (dom._h, None, n, cols, out.ptr, n, None), (dom._h, src.ptr, n, cols, None, n, None),
                 (dom._h, src.ptr, n - 1, cols, out.ptr, n, None), (dom._h, src.ptr, n, cols, out.ptr, n - 1, None)):
        assert call(*args) == SC_ERR_BAD_ARG, args
        still_right()
    sc.synchronize()
    assert out.to_bytes() == SENTINEL * (cols * n)                                  # none of the refused calls wrote anything
    dom.free()


# ---- degrees of many vectors per call ---------------------------------------------------------------------------------------------

def degree_single(sc, packed):
    v = sc.DeviceVector.from_bytes(packed)
    deg = ctypes.c_int64(-7)
    sc._check(sc.lib().sc_vec_degree_dev(v.ptr, v.n, ctypes.byref(deg), None))
    return deg.value


@pytest.mark.parametrize("cols", [1, 3, 300])
@pytest.mark.parametrize("n,ld", [(1, 1), (5, 5), (5, 9), (1000, 1000), (1000, 1003), (5000, 5001)])
def test_degrees_of_columns(sc, n, ld, cols):
    one = (1).to_bytes(16, "little")
    patterns = [bytes(16 * n), one + bytes(16 * (n - 1)), bytes(16 * (n - 1)) + one]
    junk = synth.pack_ints([v or 1 for v in synth.synth_ints(9500, ld - n)])          # non-zero entries between the columns: not read
    columns, want = [], []
    for c in range(cols):
        if c % 4 < 3:
            column = patterns[c % 4]
        else:
            column = bytearray(synth.synth_packed(9501 + c, n).tobytes())
            cut = synth.synth_ints(9600 + c, 1)[0] % (n + 1)                            # zero from a random place up
            column[16 * cut:] = bytes(16 * (n - cut))
            column = bytes(column)
        columns.append(column)
        ints = synth.unpack_ints(column)
        want.append(max([i for i, v in enumerate(ints) if v], default=-1))
    matrix = sc.DeviceVector.from_bytes(b"".join(c + junk for c in columns))
    got = (ctypes.c_int64 * cols)(*([-7] * cols))
    sc._check(sc.lib().sc_vec_degree_columns_dev(matrix.ptr, n, ld, cols, got, None))
    assert list(got) == want
    for c in sorted({0, 1, 2, 3, cols - 1} & set(range(cols))):
        assert degree_single(sc, columns[c]) == want[c], c


def test_degrees_arguments(sc):
    v = sc.DeviceVector.from_bytes(synth.synth_packed(9700, 12).tobytes())
    got = (ctypes.c_int64 * 3)(-7, -7, -7)
    call = sc.lib().sc_vec_degree_columns_dev
    assert call(v.ptr, 4, 4, 0, got, None) == 0 and list(got) == [-7, -7, -7]
    assert call(v.ptr, 4, 3, 3, got, None) == SC_ERR_BAD_ARG
    assert call(None, 4, 4, 3, got, None) == SC_ERR_BAD_ARG
    assert call(v.ptr, 4, 4, 3, None, None) == SC_ERR_BAD_ARG
    assert list(got) == [-7, -7, -7]
    sc._check(call(v.ptr, 4, 4, 3, got, None))
    assert list(got) == [3, 3, 3]

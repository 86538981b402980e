"""GPU tests of multipoint evaluation and interpolation for MANY COLUMNS per call: sc_polytree_evaluate_columns_dev and
sc_polytree_interpolate_columns_dev (the *_cols kernels of csrc/polytree.cuh, column index innermost in every level array),
sc_geodomain_evaluate_columns_dev (csrc/geoseq.cuh), and the host API on top of them (ntt.fast_evaluate_columns,
fast_evaluate_columns_device, fast_interpolate_columns on a tree domain).  Every comparison is exact: the CPU oracle on seeded
inputs, the single-column entries byte for byte, the reference's goldens as one column among others."""
import ctypes
import functools

import pytest

from conftest import load_golden
from oracle import py_oracle as po
import synth

pytestmark = pytest.mark.gpu
P = po.P
SENTINEL = (0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5).to_bytes(16, "little")       # a canonical residue no test value equals
ORDER = 512
ROOT = po.primitive_nth_root(ORDER)
MAX_COLS = 8


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


def rows(raw, count, ld, n):
    """(the first n elements of each of `count` rows of pitch ld, the rest of each row), as bytes"""
    body = [raw[16 * ld * c:16 * (ld * c + n)] for c in range(count)]
    gaps = [raw[16 * (ld * c + n):16 * ld * (c + 1)] for c in range(count)]
    return body, gaps


def matrix_of(sc, columns, n, ld):
    """the columns (lists of n ints) as a device matrix of pitch ld with non-zero junk in the gaps"""
    junk = synth.pack_ints([v or 1 for v in synth.synth_ints(4991, ld - n)])
    raw = b"".join(synth.pack_ints(c) + junk for c in columns)
    return sc.DeviceVector.from_bytes(raw) if raw else sc.DeviceVector(1)


def tree_evaluate_columns(sc, tree, columns, m, ld_in, ld_out):
    cols, k = len(columns), tree.k
    src = matrix_of(sc, columns, m, ld_in)
    out = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out))
    sc._check(sc.lib().sc_polytree_evaluate_columns_dev(tree._h, src.ptr, m, ld_in, cols, tree.points.ptr, out.ptr, ld_out, None))
    body, gaps = rows(out.to_bytes(), cols, ld_out, k)
    assert all(g == SENTINEL * (ld_out - k) for g in gaps), "a gap of the output was written"
    return [synth.unpack_ints(b) for b in body]


def tree_interpolate_columns(sc, tree, columns, ld_in, ld_out):
    cols, k = len(columns), tree.k
    src = matrix_of(sc, columns, k, ld_in)
    out = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out))
    sc._check(sc.lib().sc_polytree_interpolate_columns_dev(tree._h, src.ptr, ld_in, cols, out.ptr, ld_out, None))
    body, gaps = rows(out.to_bytes(), cols, ld_out, k)
    assert all(g == SENTINEL * (ld_out - k) for g in gaps), "a gap of the output was written"
    return [synth.unpack_ints(b) for b in body]


# ---- 1. the tree against the oracle ---------------------------------------------------------------------------------------------

def points_of(k):
    pts = synth.synth_ints(5000 + k, k)
    if k > 3:
        pts[2] = 0                                   # the point 0 is also what the tree pads with
    return pts


def lengths_of(k):
    K = 1 << max(0, (k - 1).bit_length())
    return sorted({0, 1, k, K, K + 1, 2 * K + 3})


@functools.lru_cache(maxsize=None)
def oracle_case(k):
    """the seeded inputs of MAX_COLS columns and the oracle's answers, computed once per k and shared by every column count"""
    pts = points_of(k)
    polys = {m: [synth.synth_ints(5100 + 16 * m + c, m) for c in range(MAX_COLS)] for m in lengths_of(k)}
    values = {m: [[po.evaluate(f, x) for x in pts] for f in columns] for m, columns in polys.items()}
    given = [synth.synth_ints(5200 + 16 * k + c, k) for c in range(MAX_COLS)]
    given[0][k // 2] = 0                             # one value zero
    given[1] = [0] * k                               # one column all zeros (from two columns on)
    interpolants = [po.fast_interpolate(pts, v, ROOT, ORDER) for v in given]
    return pts, polys, values, given, interpolants


@pytest.mark.parametrize("k", [1, 2, 3, 5, 16, 17, 33, 129])
def test_tree_columns_against_the_oracle(sc, k):
    pts, polys, values, given, interpolants = oracle_case(k)
    tree = sc.PolyTree(synth.pack_ints(pts))
    for cols in (1, 2, 3, 5, 8):
        for m in lengths_of(k):
            got = tree_evaluate_columns(sc, tree, polys[m][:cols], m, m + 3, k + 5)
            assert got == values[m][:cols], (k, cols, m)
        got = tree_interpolate_columns(sc, tree, given[:cols], k + 3, k + 5)
        assert got == interpolants[:cols], (k, cols)
    tree.free()


# ---- 2. column c equals the single entry, byte for byte -------------------------------------------------------------------------

@pytest.mark.parametrize("k,cols", [(1000, 7), ((1 << 12) + 5, 3)])
def test_columns_equal_the_single_entries_byte_for_byte(sc, k, cols):
    tree = sc.PolyTree(synth.synth_packed(5300 + cols, k).tobytes())
    K = 1 << (k - 1).bit_length()
    for m in (k, K + 1, 2 * K + 3):
        columns = [synth.synth_packed(5310 + 8 * cols + c, m).tobytes() for c in range(cols)]
        got = tree.evaluate_columns(sc.DeviceVector.from_bytes(b"".join(columns)), m, cols).to_bytes()
        for c in range(cols):
            assert got[16 * k * c:16 * k * (c + 1)] == tree.evaluate(sc.DeviceVector.from_bytes(columns[c])).to_bytes(), (k, m, c)
    columns = [synth.synth_packed(5350 + 8 * cols + c, k).tobytes() for c in range(cols)]
    got = tree.interpolate_columns(sc.DeviceVector.from_bytes(b"".join(columns)), cols).to_bytes()
    for c in range(cols):
        assert got[16 * k * c:16 * k * (c + 1)] == tree.interpolate(sc.DeviceVector.from_bytes(columns[c])).to_bytes(), (k, c)
    tree.free()


@pytest.mark.parametrize("k,cols", [(1000, 7), ((1 << 12) + 5, 3)])
def test_progression_columns_equal_the_single_entry_byte_for_byte(sc, k, cols):
    dom = sc.GeoDomain(po.GENERATOR, po.primitive_nth_root(1 << 14), k)
    for m in (k, k + 1, 2 * k + 3):
        columns = [synth.synth_packed(5400 + 8 * cols + c, m).tobytes() for c in range(cols)]
        got = dom.evaluate_columns(sc.DeviceVector.from_bytes(b"".join(columns)), m, cols).to_bytes()
        for c in range(cols):
            assert got[16 * k * c:16 * k * (c + 1)] == dom.evaluate(sc.DeviceVector.from_bytes(columns[c])).to_bytes(), (k, m, c)
    dom.free()


def test_reference_goldens_as_one_column_among_others(sc):
    """the `evaluate` and `interpolate` records of tests/golden/poly.json (outputs of the reference's code/ntt.py:82-130), each as
    column 1 of three, the other two seeded"""
    g = load_golden("poly.json")
    seen = 0
    for rec in g["evaluate"]:
        k, m = rec["k"], rec["poly_len"]
        if k == 0:
            continue                                  # (no tree over no points; the host API answers [] itself)
        tree = sc.PolyTree(synth.pack_ints(synth.synth_ints(rec["dom_seed"], k)))
        columns = [synth.synth_ints(5500, m), synth.synth_ints(rec["poly_seed"], m), synth.synth_ints(5501, m)]
        got = tree_evaluate_columns(sc, tree, columns, m, m + 3, k + 5)
        assert [str(v) for v in got[1]] == rec["out"], (k, m)
        tree.free()
        seen += 1
    for rec in g["interpolate"]:
        k = rec["k"]
        if k == 0:
            continue
        if "omicron_order" in rec:
            om = po.primitive_nth_root(rec["omicron_order"])
            dom = [pow(om, i, P) for i in range(k)]
        else:
            dom = synth.synth_ints(rec["dom_seed"], k)
        tree = sc.PolyTree(synth.pack_ints(dom))
        columns = [synth.synth_ints(5502, k), synth.synth_ints(rec["val_seed"], k), synth.synth_ints(5503, k)]
        got = tree_interpolate_columns(sc, tree, columns, k + 3, k + 5)
        assert [str(v) for v in got[1]] == rec["out"], k
        tree.free()
        seen += 1
    assert seen >= 8


# ---- 3. the set loop -----------------------------------------------------------------------------------------------------------

def test_more_columns_than_one_set_holds(sc):
    """k = 16 (temporaries of 2K = 32 elements per column) with the launch budget lowered to 2^7 elements: sets of four columns,
    so eleven columns take three sets, the last one padded from three columns to four lanes"""
    k, cols = 16, 11
    pts = points_of(k)
    tree = sc.PolyTree(synth.pack_ints(pts))
    polys = {m: [synth.synth_ints(5600 + 16 * m + c, m) for c in range(cols)] for m in (k, 2 * k + 3)}
    given = [synth.synth_ints(5650 + c, k) for c in range(cols)]
    want = ({m: tree_evaluate_columns(sc, tree, polys[m], m, m + 3, k + 5) for m in polys}, tree_interpolate_columns(sc, tree, given, k + 3, k + 5))
    assert want[0][k] == [[po.evaluate(f, x) for x in pts] for f in polys[k]]
    try:
        sc.set_tuning("tree_cols_launch_log", 7)
        got = ({m: tree_evaluate_columns(sc, tree, polys[m], m, m + 3, k + 5) for m in polys}, tree_interpolate_columns(sc, tree, given, k + 3, k + 5))
    finally:
        sc.set_tuning("tree_cols_launch_log", 26)
    assert got == want
    tree.free()


# ---- 4. a repeated point -------------------------------------------------------------------------------------------------------

def test_repeated_point_is_a_division_by_zero(sc):
    k, cols = 40, 3
    pts = synth.synth_ints(5700, k)
    pts[17] = pts[3]
    tree = sc.PolyTree(synth.pack_ints(pts))
    values = sc.DeviceVector.from_bytes(synth.synth_packed(5701, k * cols).tobytes())
    for _ in range(2):                                # the failure is not remembered as a table: it fails the same way again
        with pytest.raises(AssertionError, match="divide by zero"):
            tree.interpolate_columns(values, cols)
    # evaluation does not mind repeated points
    polys = [synth.synth_ints(5702 + c, 33) for c in range(cols)]
    assert tree_evaluate_columns(sc, tree, polys, 33, 33, k) == [[po.evaluate(f, x) for x in pts] for f in polys]
    tree.free()
    # a tree built afterwards works: nothing poisoned is left behind
    good = synth.synth_ints(5710, k)
    other = sc.PolyTree(synth.pack_ints(good))
    given = [synth.synth_ints(5711 + c, k) for c in range(cols)]
    assert tree_interpolate_columns(sc, other, given, k, k) == [po.fast_interpolate(good, v, ROOT, ORDER) for v in given]
    other.free()


# ---- 5. levels longer than the batched plans take --------------------------------------------------------------------------------

def test_long_levels_on_the_subgroup_of_order_2_19(sc):
    """on the full subgroup evaluation = ntt and interpolation = intt; at 2^19 the top levels' columns are longer than the batched
    plans take (per-column transforms inside the level transform)"""
    logk, cols = 19, 2
    K = 1 << logk
    w = po.primitive_nth_root(K)
    delta = bytearray(16 * K)
    delta[16] = 1
    powers = po.C.ntt(w, bytes(delta), K)             # the ntt of the delta at index 1 is w^i
    tree = sc.PolyTree(powers)
    f = synth.synth_packed(5800, K * cols).tobytes()
    fv = sc.DeviceVector.from_bytes(f)
    vals = tree.evaluate_columns(fv, K, cols)
    want = sc.DeviceVector(K * cols)
    sc._check(sc.lib().sc_ntt_columns_dev(fv.ptr, want.ptr, K, cols, sc.fe_bytes(w), 0, None))
    assert vals.to_bytes() == want.to_bytes()
    assert tree.interpolate_columns(vals, cols).to_bytes() == f
    tree.free()


# ---- 6. progression domains ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 17, 64])
def test_progression_columns_against_the_oracle_and_the_single_entry(sc, n):
    ratio = po.primitive_nth_root(256)
    for first in (1, po.GENERATOR):
        pts, x = [], first
        for _ in range(n):
            pts.append(x)
            x = x * ratio % P
        dom = sc.GeoDomain(first, ratio, n)
        for m in (0, 1, n, n + 1, 2 * n + 3):
            polys = [synth.synth_ints(5900 + 16 * m + c, m) for c in range(3)]
            want = [[po.evaluate(f, x) for x in pts] for f in polys]
            single = [dom.evaluate(sc.DeviceVector.from_bytes(synth.pack_ints(f)) if m else sc.DeviceVector(0)).to_bytes() for f in polys]
            for cols in (1, 3):
                ld_in, ld_out = m + 3, n + 5
                src = matrix_of(sc, polys[:cols], m, ld_in)
                out = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out))
                sc._check(sc.lib().sc_geodomain_evaluate_columns_dev(dom._h, src.ptr, m, ld_in, cols, out.ptr, ld_out, None))
                body, gaps = rows(out.to_bytes(), cols, ld_out, n)
                assert all(g == SENTINEL * (ld_out - n) for g in gaps), "a gap of the output was written"
                assert [synth.unpack_ints(b) for b in body] == want[:cols], (n, first, m, cols)
                assert body == single[:cols], (n, first, m, cols)
        dom.free()


# ---- 7. the host API -----------------------------------------------------------------------------------------------------------

def test_host_api(sc):
    import ntt as ntt_mod
    from ntt import (fast_evaluate, fast_evaluate_columns, fast_evaluate_columns_device, fast_evaluate_device, fast_interpolate,
                     fast_interpolate_columns, fast_interpolate_columns_device, fast_interpolate_device, DeviceDomain)
    from algebra import Field, FieldElement
    from univariate import Polynomial
    field = Field.main()
    order = 128
    root = field.primitive_nth_root(order)

    def elements(seed, n):
        return [FieldElement(v, field) for v in synth.synth_ints(seed, n)]
    scattered, progression = elements(6000, 40), [root ^ i for i in range(32)]
    assert isinstance(ntt_mod._device_tree(scattered), sc.PolyTree) and isinstance(ntt_mod._device_tree(progression), sc.GeoDomain)
    polynomials = [Polynomial(elements(6001, 17)), Polynomial([]), Polynomial(elements(6002, 40)), Polynomial(elements(6003, 100)),
                   Polynomial(elements(6004, 5) + [field.zero()] * 3), Polynomial([field.zero()] * 4)]
    for domain in (scattered, progression):
        got = fast_evaluate_columns(polynomials, domain, root, order)
        assert got == [fast_evaluate(p, domain, root, order) for p in polynomials]
        assert fast_evaluate_columns([], domain, root, order) == []
        assert fast_evaluate_columns([Polynomial([])], domain, root, order) == [[field.zero()] * len(domain)]
    # below the size that goes to the device at all: the reference's recursion per polynomial
    assert fast_evaluate_columns(polynomials, scattered[:5], root, order) == [fast_evaluate(p, scattered[:5], root, order) for p in polynomials]
    # interpolation on a tree domain takes the column entry
    values = [elements(6010 + c, 40) for c in range(3)]
    got = fast_interpolate_columns(scattered, values, root, order)
    assert [p.coefficients for p in got] == [fast_interpolate(scattered, v, root, order).coefficients for v in values]
    with pytest.raises(AssertionError, match="cannot interpolate over domain of different length than values list"):
        fast_interpolate_columns(scattered, [values[0], values[1][:39]], root, order)
    # the device forms: views of one matrix
    for domain in (DeviceDomain(scattered), DeviceDomain.geometric(field.one(), root, 32)):
        n = len(domain)
        codewords = [sc.DeviceCodeword.from_list(elements(6020 + c, length), field) for c, length in enumerate((17, n, 3 * n + 1, 1))]
        got = fast_evaluate_columns_device(codewords, domain)
        assert [g.vec.to_bytes() for g in got] == [fast_evaluate_device(c, domain).vec.to_bytes() for c in codewords]
        assert [g.vec.ptr for g in got] == [got[0].vec.ptr + 16 * n * c for c in range(len(got))]
        # rows of one matrix go in without a copy and give the same values
        again = fast_evaluate_columns_device(got, domain)
        assert [a.vec.to_bytes() for a in again] == [fast_evaluate_device(g, domain).vec.to_bytes() for g in got]
        assert fast_evaluate_columns_device([], domain) == []
        back = fast_interpolate_columns_device(domain, got)
        assert [b.vec.to_bytes() for b in back] == [fast_interpolate_device(domain, g).vec.to_bytes() for g in got]
        assert [b.vec.ptr for b in back] == [back[0].vec.ptr + 16 * n * c for c in range(len(back))]
        with pytest.raises(AssertionError, match="cannot interpolate over domain of different length than values list"):
            fast_interpolate_columns_device(domain, [got[0], codewords[0]])


def test_refused_arguments(sc):
    SC_ERR_BAD_ARG = -6
    k, cols = 20, 3
    tree = sc.PolyTree(synth.synth_packed(6100, k).tobytes())
    dom = sc.GeoDomain(po.GENERATOR, po.primitive_nth_root(64), k)
    src = sc.DeviceVector.from_bytes(synth.synth_packed(6101, 80 * cols).tobytes())
    out = sc.DeviceVector.from_bytes(SENTINEL * (k * cols))
    ev, ip, ge = sc.lib().sc_polytree_evaluate_columns_dev, sc.lib().sc_polytree_interpolate_columns_dev, sc.lib().sc_geodomain_evaluate_columns_dev
    assert ev(tree._h, src.ptr, k, k, 0, None, out.ptr, k, None) == 0                # no columns: fine, nothing happens
    assert ip(tree._h, src.ptr, k, 0, out.ptr, k, None) == 0
    assert ge(dom._h, src.ptr, k, k, 0, out.ptr, k, None) == 0
    assert ev(tree._h, src.ptr, 80, 80, cols, None, out.ptr, k, None) == SC_ERR_BAD_ARG   # m > K without the points
    assert ev(tree._h, src.ptr, k, k - 1, cols, None, out.ptr, k, None) == SC_ERR_BAD_ARG
    assert ev(tree._h, src.ptr, k, k, cols, None, out.ptr, k - 1, None) == SC_ERR_BAD_ARG
    assert ev(None, src.ptr, k, k, cols, None, out.ptr, k, None) == SC_ERR_BAD_ARG
    assert ev(tree._h, src.ptr, k, k, cols, None, None, k, None) == SC_ERR_BAD_ARG
    assert ip(tree._h, src.ptr, k - 1, cols, out.ptr, k, None) == SC_ERR_BAD_ARG
    assert ip(tree._h, src.ptr, k, cols, out.ptr, k - 1, None) == SC_ERR_BAD_ARG
    assert ip(tree._h, None, k, cols, out.ptr, k, None) == SC_ERR_BAD_ARG
    assert ge(dom._h, src.ptr, k, k - 1, cols, out.ptr, k, None) == SC_ERR_BAD_ARG
    assert ge(dom._h, src.ptr, k, k, cols, out.ptr, k - 1, None) == SC_ERR_BAD_ARG
    assert ge(dom._h, None, k, k, cols, out.ptr, k, None) == SC_ERR_BAD_ARG
    sc.synchronize()
    assert out.to_bytes() == SENTINEL * (k * cols)                                  # none of these wrote anything
    tree.free()
    dom.free()

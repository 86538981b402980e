"""GPU tests of the domain tables at the edges their feature tests leave out (cases, operands and expectations:
tests/domain_tables_cases.py; that the cases reach what they claim: tests/test_domain_tables_cases_cpu.py):

  * the progression tables of csrc/geoseq.cuh where a prefix-product scan first takes a second workgroup (n = 1025, 2049, 2050) and
    where it takes a third launch level (n = 2^21 + 1, M = 2^23), on full subgroups of the orders 11, 37, 88, 407 and 2368, on the
    last progression before such a subgroup wraps, and every refusal of sc_geodomain_create;
  * the subproduct tree of csrc/polytree.cuh over 2^18 + 1 arbitrary points -- the smallest tree whose top level takes the per-column
    transforms of ntt_cols, and the heaviest padding a tree carries -- and at k = 130, 257, 513 against the oracle.

Every entry writes into a window with sentinels in front of it, behind it and (column calls) between the columns, every input is read
back unchanged, and every comparison is exact: Python integers by the definitions, never the code under test."""
import ctypes

import pytest

from oracle import py_oracle as po
import domain_tables_cases as dc
import synth

pytestmark = pytest.mark.gpu
P = po.P
S, GUARD, COLS = dc.SENTINEL, dc.GUARD, dc.COLS
SC_ERR_UNSUPPORTED = -7


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


# ---- windows ------------------------------------------------------------------------------------------------------------------

class Window:
    """`count` output elements with GUARD sentinels in front and behind, all of it sentinels before the call"""

    def __init__(self, sc, count):
        self.count = count
        self.vec = sc.DeviceVector.from_bytes(S * (count + 2 * GUARD))
        self.ptr = self.vec.ptr + 16 * GUARD

    def read(self, what):
        raw = self.vec.to_bytes()
        assert raw[:16 * GUARD] == S * GUARD, "%s: written in front of the output" % (what,)
        assert raw[16 * (GUARD + self.count):] == S * GUARD, "%s: written past the end" % (what,)
        return raw[16 * GUARD:16 * (GUARD + self.count)]

    def read_columns(self, what, ld, n):
        """the n elements of each of COLS columns at pitch ld; the elements between the columns are still sentinels"""
        raw = self.read(what)
        for c in range(COLS - 1):
            assert raw[16 * (ld * c + n):16 * ld * (c + 1)] == S * (ld - n), "%s: a gap of the output was written" % (what,)
        return [raw[16 * ld * c:16 * (ld * c + n)] for c in range(COLS)]


class Operand:
    """device copy of packed input bytes; `unchanged` reads it back"""

    def __init__(self, sc, raw):
        self.raw = raw
        self.vec = sc.DeviceVector.from_bytes(raw) if raw else sc.DeviceVector(1)
        self.ptr = self.vec.ptr

    def unchanged(self, what):
        assert not self.raw or self.vec.to_bytes() == self.raw, "%s: the input was written" % (what,)


def matrix(sc, columns, n, ld):
    """packed columns of n elements as a device matrix of pitch ld, non-zero junk in the gaps (the last column has no gap behind it)"""
    junk = synth.pack_ints([v or 1 for v in synth.synth_ints(4991, ld - n)])
    return Operand(sc, junk.join(columns))


# ---- the entries of one domain, progression tables or tree -----------------------------------------------------------------------

class GeoEntries:
    def __init__(self, sc, case, dom):
        self.sc, self.lib, self.h, self.n = sc, sc.lib(), dom._h, case.n

    def zerofier(self, out):
        self.sc._check(self.lib.sc_geodomain_zerofier_dev(self.h, out, None))

    def evaluate(self, src, m, out):
        self.sc._check(self.lib.sc_geodomain_evaluate_dev(self.h, src, m, out, None))

    def evaluate_columns(self, src, m, ld_in, out, ld_out):
        self.sc._check(self.lib.sc_geodomain_evaluate_columns_dev(self.h, src, m, ld_in, COLS, out, ld_out, None))

    def interpolate(self, src, out):
        self.sc._check(self.lib.sc_geodomain_interpolate_dev(self.h, src, out, None))

    def interpolate_columns(self):
        def call(src, ld_in, out, ld_out):
            self.sc._check(self.lib.sc_geodomain_interpolate_columns_dev(self.h, src, ld_in, COLS, out, ld_out, None))
        return {"sc_geodomain_interpolate_columns_dev": call}


class TreeEntries:
    def __init__(self, sc, case, tree):
        self.sc, self.lib, self.h, self.n, self.points = sc, sc.lib(), tree._h, case.n, tree.points

    def zerofier(self, out):
        self.sc._check(self.lib.sc_polytree_zerofier_dev(self.h, out, None))

    def evaluate(self, src, m, out):
        self.sc._check(self.lib.sc_polytree_evaluate_dev(self.h, src, m, self.points.ptr, out, None))

    def evaluate_columns(self, src, m, ld_in, out, ld_out):
        self.sc._check(self.lib.sc_polytree_evaluate_columns_dev(self.h, src, m, ld_in, COLS, self.points.ptr, out, ld_out, None))

    def interpolate(self, src, out):
        self.sc._check(self.lib.sc_polytree_interpolate_dev(self.h, src, out, None))

    def interpolate_columns(self):
        def entry(fn):
            def call(src, ld_in, out, ld_out):
                self.sc._check(fn(self.h, src, ld_in, COLS, out, ld_out, None))
            return call
        return {name: entry(getattr(self.lib, name)) for name in ("sc_polytree_interpolate_columns_dev", "sc_polytree_interpolate_lagrange_columns_dev")}


def run_all_entries(sc, case, e):
    """every entry of one domain on every operand of its case.  The single entries are checked against the expectations; column c of a
    column call must then be the single entry's bytes for the same operand (include/starkcore.h: bit for bit)."""
    n, ld_out = case.n, case.n + 2
    w = Window(sc, n + 1)
    e.zerofier(w.ptr)
    dc.check_zerofier(case, dc.Packed(w.read((case.id, "zerofier"))))
    for m in dc.lengths(case):
        names = dc.evaluation_operands(m)
        if m == 0:
            w = Window(sc, n)
            e.evaluate(None, 0, w.ptr)
            assert w.read((case.id, "m=0")) == bytes(16 * n), (case.id, "m=0")
            w = Window(sc, (COLS - 1) * ld_out + n)
            e.evaluate_columns(Operand(sc, b"").ptr, 0, 0, w.ptr, ld_out)
            assert w.read_columns((case.id, "m=0 columns"), ld_out, n) == [bytes(16 * n)] * COLS, (case.id, "m=0 columns")
            continue
        packed = [dc.packed_coefficients(case, name) for name in names]
        single = []
        for name, raw in zip(names, packed):
            src, w = Operand(sc, raw), Window(sc, n)
            e.evaluate(src.ptr, m, w.ptr)
            single.append(w.read((case.id, name)))
            src.unchanged((case.id, name))
            dc.check_values(case, name, dc.Packed(single[-1]))
        src, w = matrix(sc, packed, m, m + 2), Window(sc, (COLS - 1) * ld_out + n)
        e.evaluate_columns(src.ptr, m, m + 2, w.ptr, ld_out)
        assert w.read_columns((case.id, "columns m=%d" % m), ld_out, n) == single, (case.id, "columns m=%d" % m)
        src.unchanged((case.id, "columns m=%d" % m))
    packed = {name: dc.packed_interpolation_values(case, name) for name in dc.INTERPOLATION_OPERANDS}
    single = {}
    for name, raw in packed.items():
        src, w = Operand(sc, raw), Window(sc, n)
        e.interpolate(src.ptr, w.ptr)
        single[name] = w.read((case.id, "interpolate", name))
        src.unchanged((case.id, "interpolate", name))
        dc.check_interpolant(case, name, dc.Packed(single[name]))
    for entry, call in e.interpolate_columns().items():
        src, w = matrix(sc, [packed[name] for name in dc.INTERPOLATION_COLUMNS], n, n + 2), Window(sc, (COLS - 1) * ld_out + n)
        call(src.ptr, n + 2, w.ptr, ld_out)
        assert w.read_columns((case.id, entry), ld_out, n) == [single[name] for name in dc.INTERPOLATION_COLUMNS], (case.id, entry)
        src.unchanged((case.id, entry))


# ---- progressions ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", dc.SMALL_GEO_CASES, ids=lambda c: c.id)
def test_progression(sc, case):
    dom = sc.GeoDomain.create(case.first, case.ratio, case.n)
    assert dom is not None, "an accepted progression was refused"
    assert sc.lib().sc_geodomain_points(dom._h) == case.n
    run_all_entries(sc, case, GeoEntries(sc, case, dom))
    dom.free()


@pytest.mark.parametrize("case", dc.DEEP_CASES, ids=lambda c: c.id)
def test_deep_scan(sc, case):
    """n = 2^21 + 1: the scan over t_j has 2^23 elements, 4096 workgroup totals and therefore a third launch level; n = 2^21 + 2049 also
    reads what the middle level's second workgroup scanned (tests/domain_tables_cases.py: DEEP_N_SEEN).  One domain each, every entry."""
    dom = sc.GeoDomain.create(case.first, case.ratio, case.n)
    assert dom is not None
    run_all_entries(sc, case, GeoEntries(sc, case, dom))
    dom.free()


@pytest.mark.parametrize("case", dc.SMALL_GEO_CASES, ids=lambda c: c.id)
def test_detection_picks_the_progression_tables(sc, case):
    pts = sc.DeviceVector.from_bytes(synth.pack_ints(dc.points(case)))
    first, ratio, flag = (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 2)(), ctypes.c_int(0)
    sc._check(sc.lib().sc_geodomain_detect_dev(pts.ptr, case.n, first, ratio, ctypes.byref(flag), None))
    assert flag.value == 1 and first[0] | (first[1] << 64) == case.first and ratio[0] | (ratio[1] << 64) == case.ratio
    tables = sc.domain_tables(pts)
    assert isinstance(tables, sc.GeoDomain) and tables.k == case.n
    w = Window(sc, case.n + 1)
    sc._check(sc.lib().sc_geodomain_zerofier_dev(tables._h, w.ptr, None))
    dc.check_zerofier(case, dc.Packed(w.read((case.id, "zerofier of the detected domain"))))
    assert pts.to_bytes() == synth.pack_ints(dc.points(case))
    tables.free()


@pytest.mark.parametrize("n", [2368, 2049])
def test_both_routes_give_the_same_bytes(sc, n):
    case = next(c for c in dc.SMALL_GEO_CASES if c.n == n and c.first == po.GENERATOR)
    pts = sc.DeviceVector.from_bytes(synth.pack_ints(dc.points(case)))
    geo, tree = sc.domain_tables(pts), sc.PolyTree(pts)
    assert isinstance(geo, sc.GeoDomain)
    assert geo.zerofier().to_bytes() == tree.zerofier().to_bytes()
    for m in dc.lengths(case):
        for name in dc.evaluation_operands(m):
            f = sc.DeviceVector.from_bytes(synth.pack_ints(dc.coefficients(case, name)))
            assert geo.evaluate(f).to_bytes() == tree.evaluate(f).to_bytes(), (case.id, name)
    for name in dc.INTERPOLATION_OPERANDS:
        v = sc.DeviceVector.from_bytes(synth.pack_ints(dc.interpolation_values(case, name)))
        assert geo.interpolate(v).to_bytes() == tree.interpolate(v).to_bytes(), (case.id, name)
    geo.free()
    tree.free()


def test_refusals(sc):
    """every refusal returns SC_ERR_UNSUPPORTED and no handle; as points the refused progressions go to the tree; the library is as good
    as before afterwards"""
    for r in dc.REFUSALS:
        h = ctypes.c_void_p()
        rc = sc.lib().sc_geodomain_create(r.first.to_bytes(16, "little"), r.ratio.to_bytes(16, "little"), r.n, ctypes.byref(h), None)
        assert rc == SC_ERR_UNSUPPORTED and not h.value, r.id
        assert sc.GeoDomain.create(r.first, r.ratio, r.n) is None, r.id
        if r.n >= 2 and r.first < P and r.ratio < P:
            pts = [r.first * pow(r.ratio, i, P) % P for i in range(r.n)]
            tables = sc.domain_tables(synth.pack_ints(pts))
            assert isinstance(tables, sc.PolyTree) and tables.k == r.n, r.id
            f = synth.synth_ints(4990, 7)
            assert synth.unpack_ints(tables.evaluate(sc.DeviceVector.from_bytes(synth.pack_ints(f))).to_bytes()) == [dc.horner(f, x) for x in pts], r.id
            tables.free()
    case = next(c for c in dc.SMALL_GEO_CASES if c.kind == "full" and c.n == 11 and c.first == po.GENERATOR)
    dom = sc.GeoDomain.create(case.first, case.ratio, case.n)
    assert dom is not None
    run_all_entries(sc, case, GeoEntries(sc, case, dom))
    dom.free()


# ---- trees --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", dc.TREE_CASES, ids=lambda c: c.id)
def test_tree_at_its_heaviest_padding(sc, case):
    tree = sc.PolyTree(synth.pack_ints(dc.points(case)))
    assert sc.lib().sc_polytree_points(tree._h) == case.n
    run_all_entries(sc, case, TreeEntries(sc, case, tree))
    assert tree.points.to_bytes() == synth.pack_ints(dc.points(case))
    tree.free()


def test_big_tree(sc):
    """k = 2^18 + 1 arbitrary points: 19 levels, so the top level's transforms go column by column (pt_col_gather_kernel,
    pt_col_scatter_kernel), and 2^18 - 1 padding leaves; one tree, every entry"""
    case = dc.BIG_TREE_CASE
    tree = sc.PolyTree(synth.pack_ints(dc.points(case)))
    run_all_entries(sc, case, TreeEntries(sc, case, tree))
    assert tree.points.to_bytes() == synth.pack_ints(dc.points(case))
    tree.free()

"""GPU tests of the product family: sc_poly_mul_dev, sc_poly_mul_columns_dev, sc_poly_pow_dev and sc_poly_product_dev
(csrc/polymul.cuh, the entries in csrc/polytree_geo.hip), DevicePolynomial.multiply / power, ntt.multiply_columns_device /
fast_multiply_columns / fast_power / fast_product and the dispatch of Polynomial.__xor__.  Every comparison is exact and byte for
byte: the expectations are products of Python integers on seeded operands (tests/emu/poly_multiply_cases.py, shared with the host
model's test), the single entry's bytes for the columns form.  Outputs sit in sentinel-filled buffers with guard elements behind
them, matrices have non-zero junk between a row's length and its stride."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
from oracle import py_oracle as po
import poly_multiply_cases as cases
import synth

pytestmark = pytest.mark.gpu
P = po.P
SENTINEL = (0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5).to_bytes(16, "little")       # a canonical residue no test value equals
SC_ERR_BAD_ARG = -6
GUARD = 3                                             # sentinel elements kept behind every output
LAUNCH_KEY = "div_cols_launch_log"


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    starkcore.set_tuning(LAUNCH_KEY, 26)


@pytest.fixture
def small_sets(sc):
    """lowers the launch key for one test and restores it"""
    def lower(value):
        sc.set_tuning(LAUNCH_KEY, value)
    yield lower
    sc.set_tuning(LAUNCH_KEY, 26)


def matrix_of(sc, rows, n, ld):
    """the rows (lists of n ints) as a device matrix of pitch ld with non-zero junk in the gaps"""
    junk = synth.pack_ints([v or 1 for v in synth.synth_ints(4991, ld - n)])
    return sc.DeviceVector.from_bytes(b"".join(synth.pack_ints(list(r)) + junk for r in rows))


def guarded(sc, n):
    return sc.DeviceVector.from_bytes(SENTINEL * (n + GUARD))


def checked(vec, n, what):
    raw = vec.to_bytes()
    assert raw[16 * n:] == SENTINEL * GUARD, "%s: written past the end" % what
    return raw[:16 * n]


def dev_mul(sc, a, b, same=False):
    """sc_poly_mul_dev -> bytes of the na + nb - 1 coefficients; same: d_b IS d_a"""
    da = sc.DeviceVector.from_ints(a)
    db = da if same else sc.DeviceVector.from_ints(b)
    out = guarded(sc, len(a) + len(b) - 1)
    sc._check(sc.lib().sc_poly_mul_dev(da.ptr, len(a), db.ptr, len(b), out.ptr, None))
    return checked(out, len(a) + len(b) - 1, "product")


def dev_mul_columns(sc, columns, others, ld_a, ld_b, ld_out):
    """sc_poly_mul_columns_dev on junk-padded matrices -> [bytes per column]; others: ONE list of ints (ld_b == 0) or one per column"""
    cols, na = len(columns), len(columns[0])
    shared = not isinstance(others[0], list)
    nb = len(others) if shared else len(others[0])
    n = na + nb - 1
    src = matrix_of(sc, columns, na, ld_a)
    mult = sc.DeviceVector.from_ints(others) if shared else matrix_of(sc, others, nb, ld_b)
    out = guarded(sc, cols * ld_out)
    sc._check(sc.lib().sc_poly_mul_columns_dev(src.ptr, na, ld_a, cols, mult.ptr, nb, 0 if shared else ld_b, out.ptr, ld_out, None))
    raw = checked(out, cols * ld_out, "columns")
    assert all(raw[16 * (ld_out * c + n):16 * ld_out * (c + 1)] == SENTINEL * (ld_out - n) for c in range(cols)), "a gap of the output was written"
    return [raw[16 * ld_out * c:16 * (ld_out * c + n)] for c in range(cols)]


def dev_pow(sc, a, exponent):
    n = exponent * (len(a) - 1) + 1
    da, out = sc.DeviceVector.from_ints(a), guarded(sc, n)
    sc._check(sc.lib().sc_poly_pow_dev(da.ptr, len(a), exponent, out.ptr, None))
    return checked(out, n, "power")


def dev_product(sc, rows, ld):
    count, n = len(rows), len(rows[0])
    total = count * (n - 1) + 1
    src, out = matrix_of(sc, rows, n, ld), guarded(sc, total)
    sc._check(sc.lib().sc_poly_product_dev(src.ptr, n, ld, count, out.ptr, None))
    return checked(out, total, "product of many")


def _poly(values):
    from algebra import Field, FieldElement
    from univariate import Polynomial
    field = Field.main()
    return Polynomial([FieldElement(v, field) for v in values])


def _ints(polynomial):
    return [c.value for c in polynomial.coefficients]


# ---- 1. single products -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("na,nb", cases.MUL_SHAPES)
def test_product(sc, na, nb):
    """every shape of the list, every operand kind (general, zero top coefficients, an all-zero multiplicand, both all zero, edge
    residues): the ABI's bytes and DevicePolynomial.multiply's list against the exact product"""
    from ntt import DevicePolynomial
    if (na, nb) == (1025, 1025):
        # the planner's boundary: (1025, 1024) fills the last one-pass transform, this shape takes the first two-pass one
        assert sc.lib().sc_ntt_num_passes(1 << 11) == 1 and sc.lib().sc_ntt_num_passes(1 << 12) == 2
    for (label, a, b), want in zip(cases.mul_operands(na, nb), cases.mul_expected(na, nb)):
        assert dev_mul(sc, a, b) == synth.pack_ints(want), (na, nb, label)
        product = DevicePolynomial.from_polynomial(_poly(a)).multiply(DevicePolynomial.from_polynomial(_poly(b)))
        assert len(product) == na + nb - 1 and product.vec.to_bytes(0, len(product)) == synth.pack_ints(want), (na, nb, label)
        assert product.degree() == po.degree(want), (na, nb, label)


@pytest.mark.parametrize("n", [1, 2, 5, 33, 2049])
def test_square_through_one_buffer(sc, n):
    """d_a == d_b with na == nb transforms once: the same bytes as the product from two separate buffers, and the exact square"""
    from ntt import DevicePolynomial
    a = cases.square_operand(n)
    once, twice = dev_mul(sc, a, a, same=True), dev_mul(sc, a, a)
    assert once == twice == synth.pack_ints(cases.exact_product(a, a))
    p = DevicePolynomial.from_polynomial(_poly(a))
    assert p.multiply(p).vec.to_bytes() == once


def test_prefix_of_the_same_buffer(sc):
    """d_a == d_b with na != nb is no square"""
    a = cases.square_operand(33)
    da, out = sc.DeviceVector.from_ints(a), guarded(sc, 33 + 20 - 1)
    sc._check(sc.lib().sc_poly_mul_dev(da.ptr, 33, da.ptr, 20, out.ptr, None))
    assert checked(out, 52, "product") == synth.pack_ints(cases.exact_product(a, a[:20]))


# ---- 2. columns -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", cases.COLUMN_COUNTS)
@pytest.mark.parametrize("na,nb", cases.COLUMN_SHAPES)
def test_columns_match_single(sc, na, nb, cols):
    """a shared multiplicand (ld_b == 0) and one per column, tight strides and ld_a, ld_b, ld_out each above its length with junk in
    the gaps: every column equals the single entry's bytes and the exact product; the output's gaps keep the sentinel"""
    columns, others = cases.column_operands(na, nb, cols)
    n = na + nb - 1
    single_shared = [dev_mul(sc, a, others[0]) for a in columns]
    single_each = [dev_mul(sc, a, b) for a, b in zip(columns, others)]
    assert single_each == [synth.pack_ints(cases.exact_product(a, b)) for a, b in zip(columns, others)]
    assert single_shared == [synth.pack_ints(cases.exact_product(a, others[0])) for a in columns]
    for ld_a, ld_b, ld_out in ((na, nb, n), (na + 5, nb + 2, n + 3)):
        assert dev_mul_columns(sc, columns, others[0], ld_a, 0, ld_out) == single_shared, (na, nb, cols, ld_a)
        assert dev_mul_columns(sc, columns, others, ld_a, ld_b, ld_out) == single_each, (na, nb, cols, ld_a)


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_column"])
def test_columns_in_sets(sc, small_sets, shared):
    """five columns with the launch limit lowered to two columns' worth of values (2^8 against transforms of 2^7): sets of 2, 2 and 1
    columns that reuse the temporaries"""
    na, nb, cols = 33, 33, 5
    columns, others = cases.column_operands(na, nb, cols)
    single = [dev_mul(sc, a, others[0] if shared else b) for a, b in zip(columns, others)]
    small_sets(8)
    assert dev_mul_columns(sc, columns, others[0] if shared else others, na + 5, 0 if shared else nb + 2, na + nb + 2) == single


def test_columns_two_pass(sc, small_sets):
    """three columns whose transforms have two passes (2^13), then the same in sets of 2 and 1"""
    na, nb, cols = 4097, 100, 3
    columns, others = cases.column_operands(na, nb, cols)
    single = [dev_mul(sc, a, b) for a, b in zip(columns, others)]
    assert single[0] == synth.pack_ints(cases.exact_product(columns[0], others[0]))
    assert dev_mul_columns(sc, columns, others, na + 3, nb + 1, na + nb + 4) == single
    small_sets(14)
    assert dev_mul_columns(sc, columns, others, na + 3, nb + 1, na + nb + 4) == single
    assert dev_mul_columns(sc, columns, others[0], na + 3, 0, na + nb + 4)[0] == single[0]


# ---- 3. powers --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("na,exponent", cases.POW_SHAPES)
def test_power(sc, na, exponent):
    """the ABI's bytes, DevicePolynomial.power's and fast_power's lists against the exact power (general operands, edge residues, a
    base with a zero top coefficient)"""
    from ntt import DevicePolynomial, fast_power
    for (label, a), want in zip(cases.pow_operands(na, exponent), cases.pow_expected(na, exponent)):
        assert dev_pow(sc, a, exponent) == synth.pack_ints(want), (na, exponent, label)
        if any(a):
            power = DevicePolynomial.from_polynomial(_poly(a)).power(exponent)
            assert len(power) == len(want) and power.vec.to_bytes(0, len(power)) == synth.pack_ints(want), (na, exponent, label)
            assert power.degree() == po.degree(want)
            assert _ints(fast_power(_poly(a), exponent)) == want, (na, exponent, label)


def test_power_of_zero(sc):
    """the all-zero base: zeros from the ABI (the constant 1 for exponent 0); the host API keeps Polynomial.__xor__'s empty polynomial"""
    from ntt import DevicePolynomial, fast_power
    zero = [0] * 4
    assert dev_pow(sc, zero, 0) == synth.pack_ints([1])
    assert dev_pow(sc, zero, 1) == bytes(16 * 4)
    assert dev_pow(sc, zero, 3) == bytes(16 * 10)
    assert dev_pow(sc, [0] * 40, 7) == bytes(16 * 274)
    for exponent in (0, 1, 3):
        assert _ints(_poly(zero) ^ exponent) == [] == _ints(fast_power(_poly(zero), exponent))
        assert len(DevicePolynomial.from_polynomial(_poly(zero)).power(exponent)) == 0


# ---- 4. products of many ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count,n", cases.PRODUCT_SHAPES)
def test_product_of_many(sc, small_sets, count, n):
    """tight rows, rows at a stride above their length with junk behind them, and the launch key lowered so that the lowest level
    takes several sets: the exact left-to-right product every time; fast_product gives the same list"""
    from ntt import fast_product
    rows = [list(r) for r in cases.product_rows(count, n)]
    want = synth.pack_ints(cases.product_expected(count, n))
    assert dev_product(sc, rows, n) == want
    assert dev_product(sc, rows, n + 3) == want
    assert _ints(fast_product([_poly(r) for r in rows])) == cases.product_expected(count, n)
    small_sets(max(2, (2 * n - 2).bit_length() + 1))          # two rows of the lowest level per set
    assert dev_product(sc, rows, n + 3) == want


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_outputs_alone(sc):
    na, nb, cols = 40, 9, 2
    n = na + nb - 1
    a = sc.DeviceVector.from_ints(synth.synth_ints(9950, cols * na))
    b = sc.DeviceVector.from_ints(synth.synth_ints(9951, cols * nb))
    out = sc.DeviceVector.from_bytes(SENTINEL * (cols * n * 4))
    one, many, power, product = sc.lib().sc_poly_mul_dev, sc.lib().sc_poly_mul_columns_dev, sc.lib().sc_poly_pow_dev, sc.lib().sc_poly_product_dev
    huge = 1 << 32
    refused = [
        one(None, na, b.ptr, nb, out.ptr, None), one(a.ptr, na, None, nb, out.ptr, None), one(a.ptr, na, b.ptr, nb, None, None),      # null
        one(a.ptr, 0, b.ptr, nb, out.ptr, None), one(a.ptr, na, b.ptr, 0, out.ptr, None),                                              # zero lengths
        one(a.ptr, na, b.ptr, nb, a.ptr, None), one(a.ptr, na, b.ptr, nb, b.ptr, None), one(a.ptr, na, b.ptr, nb, a.ptr + 16 * (na - 1), None),   # overlap
        one(a.ptr, huge, b.ptr, 2, out.ptr, None),                                                                                     # too long
        many(None, na, na, cols, b.ptr, nb, nb, out.ptr, n, None), many(a.ptr, na, na, cols, None, nb, 0, out.ptr, n, None),
        many(a.ptr, na, na, cols, b.ptr, nb, nb, None, n, None),
        many(a.ptr, 0, na, cols, b.ptr, nb, nb, out.ptr, n, None), many(a.ptr, na, na, cols, b.ptr, 0, 0, out.ptr, n, None),
        many(a.ptr, na, na - 1, cols, b.ptr, nb, nb, out.ptr, n, None), many(a.ptr, na, na, cols, b.ptr, nb, nb - 1, out.ptr, n, None),   # strides
        many(a.ptr, na, na, cols, b.ptr, nb, nb, out.ptr, n - 1, None),
        many(a.ptr, na, na, cols, b.ptr, nb, nb, a.ptr, n, None), many(a.ptr, na, na, cols, b.ptr, nb, 0, b.ptr, n, None),
        many(a.ptr, na, na, cols, b.ptr, nb, nb, b.ptr + 16 * (cols * nb - 1), n, None),
        many(a.ptr, huge, huge, 1, b.ptr, 2, 0, out.ptr, huge + 1, None),
        power(None, na, 3, out.ptr, None), power(a.ptr, na, 3, None, None), power(a.ptr, 0, 3, out.ptr, None),
        power(a.ptr, na, 3, a.ptr, None), power(a.ptr, na, 0, a.ptr + 16 * (na - 1), None),
        power(a.ptr, 2, huge, out.ptr, None), power(a.ptr, na, (1 << 64) - 1, out.ptr, None),
        product(None, na, na, cols, out.ptr, None), product(a.ptr, na, na, cols, None, None), product(a.ptr, 0, na, cols, out.ptr, None),
        product(a.ptr, na, na - 1, cols, out.ptr, None), product(a.ptr, na, na, cols, a.ptr + 16 * na, None),
        product(a.ptr, 2, 2, huge, out.ptr, None),
    ]
    assert refused == [SC_ERR_BAD_ARG] * len(refused)
    assert many(a.ptr, na, na, 0, b.ptr, nb, nb, out.ptr, n, None) == 0                   # no columns: fine, nothing happens
    assert product(a.ptr, na, na, 0, out.ptr, None) == 0
    sc.synchronize()
    assert out.to_bytes() == SENTINEL * (cols * n * 4)                                   # none of these wrote anything
    assert a.to_bytes() == synth.pack_ints(synth.synth_ints(9950, cols * na)) and b.to_bytes() == synth.pack_ints(synth.synth_ints(9951, cols * nb))


# ---- 6. the host API --------------------------------------------------------------------------------------------------------------

def test_fast_multiply_columns(sc):
    from ntt import fast_multiply_columns
    a, b = synth.synth_ints(9960, 60), synth.synth_ints(9961, 40)
    lhs = [_poly(a), _poly(a[:50] + [0] * 4), _poly(a[:3]), _poly([0] * 5), _poly([]), _poly(a[7:] + [0]), _poly([5])]
    for rhs in (_poly(b), _poly(b + [0, 0]), _poly([3]), _poly([0, 0]), _poly([]), _poly(b[:2])):
        got = fast_multiply_columns(lhs, rhs)
        assert len(got) == len(lhs)
        for g, l in zip(got, lhs):
            want = l._schoolbook_mul(rhs) if l.coefficients and rhs.coefficients else _poly([])
            assert _ints(g) == _ints(want)
    assert fast_multiply_columns([], _poly(b)) == []
    assert [_ints(g) for g in fast_multiply_columns(lhs[:1], _poly(b))] == [cases.exact_product(a, b)]


def test_fast_power_and_product(sc):
    from ntt import fast_power, fast_product
    a = synth.synth_ints(9962, 40)
    for values in (a, a[:37] + [0] * 3, a[:3], [7], a[:2] + [0]):
        for exponent in (0, 1, 2, 3, 7):
            assert _ints(fast_power(_poly(values), exponent)) == _ints(_poly(values)._binary_power(exponent)), (len(values), exponent)
    members = [a, a[:20] + [0, 0], a[:3], [9], a[5:30]]
    want = [1]
    for m in members:
        want = cases.exact_product(want, m)
    assert _ints(fast_product([_poly(m) for m in members])) == want
    assert _ints(fast_product([_poly(a)])) == a
    assert _ints(fast_product([_poly(a), _poly([0] * 3), _poly(a[:4])])) == [0] * (40 + 2 + 3)
    assert _ints(fast_product([_poly(a), _poly([])])) == []
    assert _ints(fast_product([_poly(a[:3]), _poly(a[:2])])) == cases.exact_product(a[:3], a[:2])


def test_resident_operands(sc):
    from ntt import DevicePolynomial, multiply_columns_device
    field = _poly([1]).coefficients[0].field
    a, b = synth.synth_ints(9963, 60), synth.synth_ints(9964, 40)
    # DevicePolynomial.multiply / power: list lengths with trailing zeros, empty operands
    pa, pb = DevicePolynomial.from_polynomial(_poly(a + [0, 0])), DevicePolynomial.from_polynomial(_poly(b + [0]))
    product = pa.multiply(pb)
    assert len(product) == 62 + 41 - 1 and product.degree() == po.degree(cases.exact_product(a, b))
    assert _ints(product.to_polynomial()) == cases.exact_product(a + [0, 0], b + [0])
    assert len(pa.multiply(DevicePolynomial.from_polynomial(_poly([]), field))) == 0
    power = pb.power(3)
    assert len(power) == 3 * 40 + 1 and _ints(power.to_polynomial()) == cases.exact_power(b + [0], 3)
    assert _ints(pb.power(0).to_polynomial()) == [1] and _ints(pb.power(1).to_polynomial()) == b + [0]
    # rows of one matrix, one shared multiplicand and one per column
    polys = [_poly(a), _poly(a[:50]), _poly(a[3:] + [0] * 3)]
    rows = DevicePolynomial.rows_from_polynomials(polys, field)
    shared = multiply_columns_device(rows, pb)
    assert [len(p) for p in shared] == [60 + 41 - 1] * 3
    for p, l in zip(shared, polys):
        want = cases.exact_product(_ints(l) + [0] * (60 - len(_ints(l))), b + [0])
        assert _ints(p.to_polynomial()) == want and p.degree() == po.degree(want)
    each = multiply_columns_device(rows, rows)
    for p, l in zip(each, polys):
        padded = _ints(l) + [0] * (60 - len(_ints(l)))
        assert _ints(p.to_polynomial()) == cases.exact_product(padded, padded)
    # separately allocated operands of unequal length on both sides
    lhs = [DevicePolynomial.from_polynomial(_poly(v)) for v in (a, a[:17], a[:33] + [0])]
    rhs = [DevicePolynomial.from_polynomial(_poly(v)) for v in (b, b[:40], b[:5])]
    got = multiply_columns_device(lhs, rhs)
    assert [len(p) for p in got] == [60 + 40 - 1] * 3
    for p, l, r in zip(got, (a, a[:17], a[:33] + [0]), (b, b[:40], b[:5])):
        want = cases.exact_product(l, r)
        assert _ints(p.to_polynomial()) == want + [0] * (99 - len(want))
    assert multiply_columns_device([], pb) == []
    one = multiply_columns_device(lhs[:1], pb)
    assert _ints(one[0].to_polynomial()) == cases.exact_product(a, b + [0])


# ---- 7. the dispatch of Polynomial.__xor__ ------------------------------------------------------------------------------------------

def test_dispatch(sc, monkeypatch):
    import ntt as ntt_mod
    from univariate import Polynomial
    calls = []
    real = ntt_mod.fast_power
    monkeypatch.setattr(ntt_mod, "fast_power", lambda p, e: calls.append((len(p.coefficients), e)) or real(p, e))
    base = _poly(synth.synth_ints(9970, 37) + [0] * 3)           # 40 coefficients, three of them trailing zeros
    want = {e: _ints(base._binary_power(e)) for e in (0, 1, 2, 3, 7)}
    assert [len(want[e]) for e in (2, 3, 7)] == [79, 118, 274]
    monkeypatch.setattr(Polynomial, "FAST_POW_MIN_LEN", 10**9)
    for e in (2, 3, 7):
        assert _ints(base ^ e) == want[e]
    assert calls == []                                            # switched off: the device entry is not called
    monkeypatch.setattr(Polynomial, "FAST_POW_MIN_LEN", 32)
    for e in (2, 3, 7):
        assert _ints(base ^ e) == want[e]
    assert calls == [(40, 2), (40, 3), (40, 7)]
    for e in (0, 1):
        assert _ints(base ^ e) == want[e]
    short = _poly(synth.synth_ints(9971, 31) + [0] * 9)           # 40 coefficients, degree 30: decided on the degree
    assert _ints(short ^ 3) == _ints(short._binary_power(3))
    assert _ints(_poly([0] * 40) ^ 3) == []
    assert len(calls) == 3


def test_evaluate_symbolic_gains_through_the_dispatch(sc, monkeypatch):
    """a three-variable constraint with exponents 0 to 3 on host points of 40 coefficients: _evaluate_symbolic_host raises its powers
    through Polynomial.__xor__, so with the dispatch on it answers exactly what it answers with the dispatch off -- and so does
    evaluate_symbolic"""
    import ntt as ntt_mod
    from algebra import Field, FieldElement
    from multivariate import MPolynomial
    from univariate import Polynomial
    field = Field.main()
    x, y, z = MPolynomial.variables(3, field)
    constraint = (x ^ 3) * (y ^ 2) + (y ^ 3) * z * MPolynomial.constant(FieldElement(5, field)) - (z ^ 3) + (x ^ 2) - y + MPolynomial.constant(FieldElement(7, field))
    point = [_poly(synth.synth_ints(9980 + i, 38) + [0, 0]) for i in range(3)]
    monkeypatch.setattr(Polynomial, "FAST_POW_MIN_LEN", 10**9)
    want = _ints(constraint._evaluate_symbolic_host(point))
    calls = []
    real = ntt_mod.fast_power
    monkeypatch.setattr(ntt_mod, "fast_power", lambda p, e: calls.append(e) or real(p, e))
    monkeypatch.setattr(Polynomial, "FAST_POW_MIN_LEN", 32)
    assert _ints(constraint._evaluate_symbolic_host(point)) == want
    assert sorted(calls) == [2, 2, 3, 3, 3]                       # x^3, y^2, y^3, z^3, x^2: once per distinct (variable, exponent)
    got = constraint.evaluate_symbolic(point)
    assert _ints(got)[:po.degree(want) + 1] == want[:po.degree(want) + 1]

"""GPU tests of division with remainder: sc_poly_divmod, sc_poly_divmod_dev and sc_poly_divmod_columns_dev (csrc/polydiv.cuh, the
entries in csrc/polytree_geo.hip), ntt.fast_divide / fast_divide_columns / divide_columns_device, DevicePolynomial.divmod and the
dispatch of Polynomial.divide.  Every comparison is exact: the oracle's long division on seeded operands (tests/emu/poly_divide_cases.py,
shared with the host model's test), the defining property a = q b + r, deg r < deg b where the long division is too slow, the
single-column entry byte for byte for the columns form."""
import ctypes
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
from oracle import py_oracle as po
import poly_divide_cases as cases
import synth

pytestmark = pytest.mark.gpu
P = po.P
SENTINEL = (0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5).to_bytes(16, "little")       # a canonical residue no test value equals (tests/test_gpu_tree_columns.py)
SC_ERR_DIV_ZERO, SC_ERR_BAD_ARG = -5, -6
GUARD = 3                                             # sentinel elements kept behind every output


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    starkcore.set_tuning("div_cols_launch_log", 26)


@functools.lru_cache(maxsize=None)
def shape_cases(m, nb):
    """((label, a, b, q, r), ...) of one shape, the expectation computed once"""
    return tuple((label, a, b) + cases.expected(a, b) for label, a, b in cases.operands(m, nb))


def rows(raw, count, ld, n):
    """(the first n elements of each of `count` rows of pitch ld, the rest of each row), as bytes"""
    body = [raw[16 * ld * c:16 * (ld * c + n)] for c in range(count)]
    gaps = [raw[16 * (ld * c + n):16 * ld * (c + 1)] for c in range(count)]
    return body, gaps


def matrix_of(sc, columns, n, ld):
    """the columns (lists of n ints) as a device matrix of pitch ld with non-zero junk in the gaps"""
    junk = synth.pack_ints([v or 1 for v in synth.synth_ints(4991, ld - n)])
    return sc.DeviceVector.from_bytes(b"".join(synth.pack_ints(c) + junk for c in columns))


def dev_divmod(sc, a, b, want_q=True, want_r=True):
    """sc_poly_divmod_dev -> (q bytes or None, r bytes or None); nothing behind the m resp. nb - 1 elements may change"""
    na, nb = len(a), len(b)
    m, nr = na - nb + 1, nb - 1
    da, db = sc.DeviceVector.from_ints(a), sc.DeviceVector.from_ints(b)
    dq, dr = sc.DeviceVector.from_bytes(SENTINEL * (m + GUARD)), sc.DeviceVector.from_bytes(SENTINEL * (nr + GUARD))
    sc._check(sc.lib().sc_poly_divmod_dev(da.ptr, na, db.ptr, nb, dq.ptr if want_q else None, dr.ptr if want_r else None, None))
    q, r = dq.to_bytes(), dr.to_bytes()
    assert q[16 * (m if want_q else 0):] == SENTINEL * (GUARD + (0 if want_q else m)), "the quotient's buffer was written past its end"
    assert r[16 * (nr if want_r else 0):] == SENTINEL * (GUARD + (0 if want_r else nr)), "the remainder's buffer was written past its end"
    return (q[:16 * m] if want_q else None), (r[:16 * nr] if want_r else None)


def dev_divmod_columns(sc, columns, b, ld_a, ld_q, ld_r, want_q=True, want_r=True):
    """sc_poly_divmod_columns_dev on a junk-padded matrix -> ([q bytes per column] or None, [r bytes per column] or None); the gaps of
    the outputs must still hold the sentinel"""
    cols, na, nb = len(columns), len(columns[0]), len(b)
    m, nr = na - nb + 1, nb - 1
    src, db = matrix_of(sc, columns, na, ld_a), sc.DeviceVector.from_ints(b)
    dq, dr = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_q + GUARD)), sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_r + GUARD))
    sc._check(sc.lib().sc_poly_divmod_columns_dev(src.ptr, na, ld_a, cols, db.ptr, nb, dq.ptr if want_q else None, ld_q, dr.ptr if want_r else None, ld_r, None))
    out = []
    for vec, ld, n, want in ((dq, ld_q, m, want_q), (dr, ld_r, nr, want_r)):
        raw = vec.to_bytes()
        if not want:
            assert raw == SENTINEL * (cols * ld + GUARD), "an output that was not asked for was written"
            out.append(None)
            continue
        body, gaps = rows(raw, cols, ld, n)
        assert all(g == SENTINEL * (ld - n) for g in gaps), "a gap of the output was written"
        assert raw[16 * cols * ld:] == SENTINEL * GUARD
        out.append(body)
    return out


# ---- 1. against the oracle, small shapes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", cases.M_GRID)
def test_divmod_against_oracle(sc, m):
    """every shape of the grid (this m, every nb), every operand kind of tests/emu/poly_divide_cases.py: non-monic divisors (leading
    p - 1 and 2), a zero constant term, the monomial, a numerator with zero top coefficients, an exact product (zero remainder),
    a == b (m == 1), edge residues"""
    for nb in cases.NB_GRID:
        for label, a, b, want_q, want_r in shape_cases(m, nb):
            q, r = dev_divmod(sc, a, b)
            assert synth.unpack_ints(q) == want_q, (m, nb, label)
            assert synth.unpack_ints(r) == want_r, (m, nb, label)
            if label == "exact product":
                assert r == bytes(16 * (nb - 1)), (m, nb)


# ---- 2. across the planner's pass boundary ----------------------------------------------------------------------------------------

def oracle_product(x, y):
    """x * y by the oracle's transforms.  po.fast_multiply is this very computation on Python integers (17 s at 2^17 points); its C
    restatement does the three transforms here."""
    n = 1 << (len(x) + len(y) - 2).bit_length()
    root = po.primitive_nth_root(n)
    fx, fy = (po.C.ntt(root, synth.pack_ints(v + [0] * (n - len(v))), n) for v in (x, y))
    return synth.unpack_ints(po.C.intt(root, po.C.pointwise_mul(fx, fy, n), n))[:len(x) + len(y) - 1]


def trim(c):
    return c[:po.degree(c) + 1]


@pytest.mark.parametrize("na,nb", [(5000, 1500), ((1 << 16) + 3, (1 << 15) - 7)])
def test_divmod_large(sc, na, nb):
    """the largest transform (2P, P = the power of two above m) is 2^13 resp. 2^17: beyond single_pass_max_log (2^11), so multi-pass
    plans.  The long division is too slow here: a = q b + r with len(r) = nb - 1 determines (q, r) uniquely."""
    a = synth.synth_ints(7700 + nb, na)
    b = synth.synth_ints(7701 + nb, nb)
    b[-1] = P - 2
    q, r = dev_divmod(sc, a, b)
    q, r = synth.unpack_ints(q), synth.unpack_ints(r)
    assert len(q) == na - nb + 1 and len(r) == nb - 1
    assert max(q) < P and max(r) < P
    if na < 10000:
        assert oracle_product(q, b) == po.fast_multiply(q, b, po.primitive_nth_root(8192), 8192)     # (the helper above is the oracle's product)
    assert trim(po.poly_add(oracle_product(q, b), r)) == trim(a)


# ---- 3. the host-buffer entry -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,nb", [(1, 1), (33, 31), (65, 100)])
def test_host_entry_matches_dev(sc, m, nb):
    for label, a, b, want_q, want_r in shape_cases(m, nb)[:3]:
        na = len(a)
        q, r = ctypes.create_string_buffer(SENTINEL * (m + GUARD)), ctypes.create_string_buffer(SENTINEL * (nb - 1 + GUARD))
        sc._check(sc.lib().sc_poly_divmod(synth.pack_ints(a), na, synth.pack_ints(b), nb, q, r))
        dq, dr = dev_divmod(sc, a, b)
        assert q.raw[:16 * (m + GUARD)] == dq + SENTINEL * GUARD, (m, nb, label)
        assert r.raw[:16 * (nb - 1 + GUARD)] == dr + SENTINEL * GUARD, (m, nb, label)
        only_q = ctypes.create_string_buffer(16 * m)
        sc._check(sc.lib().sc_poly_divmod(synth.pack_ints(a), na, synth.pack_ints(b), nb, only_q, None))
        assert only_q.raw[:16 * m] == dq


# ---- 4. columns -------------------------------------------------------------------------------------------------------------------

def columns_of(m, nb, cols):
    """`cols` numerators of m + nb - 1 coefficients and one divisor: the shape's general operands, an exact product and a numerator with
    zero top coefficients among them"""
    ops = shape_cases(m, nb)
    by_label = {label: a for label, a, b, _, _ in ops if b == ops[0][2]}
    na = m + nb - 1
    columns = [by_label["general"], by_label["exact product"], by_label["numerator with two zero top coefficients"]]
    columns += [synth.synth_ints(7800 + 17 * c + m, na) for c in range(3, cols)]
    return columns[:cols], ops[0][2]


@pytest.mark.parametrize("m,nb", [(1, 1), (2, 33), (33, 31), (65, 100), (64, 3)])
@pytest.mark.parametrize("cols", [1, 3, 8])
def test_columns_match_single(sc, m, nb, cols):
    """input pitches above na with junk in the gaps, output pitches above what is stored: every column equals the single-column entry
    byte for byte, the gaps keep the sentinel, and leaving out one output leaves the other as it was"""
    columns, b = columns_of(m, nb, cols)
    na, nr = m + nb - 1, nb - 1
    single = [dev_divmod(sc, a, b) for a in columns]
    for ld_a, ld_q, ld_r in ((na, m, max(nr, 1)), (na + 5, m + 3, nr + 2)):
        q, r = dev_divmod_columns(sc, columns, b, ld_a, ld_q, ld_r)
        assert q == [s[0] for s in single], (m, nb, cols, ld_a)
        assert r == [s[1] for s in single], (m, nb, cols, ld_a)
    q_only, none = dev_divmod_columns(sc, columns, b, na + 5, m + 3, nr + 2, want_r=False)
    assert none is None and q_only == q
    none, r_only = dev_divmod_columns(sc, columns, b, na + 5, m + 3, nr + 2, want_q=False)
    assert none is None and r_only == r
    want = [cases.expected(a, b) for a in columns]
    assert [synth.unpack_ints(x) for x in q] == [w[0] for w in want]
    assert [synth.unpack_ints(x) for x in r] == [w[1] for w in want]


@pytest.mark.parametrize("want_r", [True, False], ids=["with_remainder", "quotient_only"])
def test_columns_in_chunks(sc, want_r):
    """five columns with the launch limit lowered to two columns' worth of values ("div_cols_launch_log" = 9 against transforms of
    2^8): the entry works through chunks of 2, 2 and 1 columns that reuse its temporaries"""
    m, nb, cols = 65, 100, 5
    columns, b = columns_of(m, nb, cols)
    single = [dev_divmod(sc, a, b) for a in columns]
    sc.set_tuning("div_cols_launch_log", 9)
    try:
        q, r = dev_divmod_columns(sc, columns, b, m + nb + 1, m + 2, nb + 2, want_r=want_r)
    finally:
        sc.set_tuning("div_cols_launch_log", 26)
    assert q == [s[0] for s in single]
    assert r == ([s[1] for s in single] if want_r else None)


MULTI_PASS = (2101, 2100, 3)                          # m, nb, cols: Newton up to 2^13, the quotient product at 2^13, the remainder product at 2^12


@functools.lru_cache(maxsize=None)
def multi_pass_columns():
    """(columns, b) of MULTI_PASS: a general numerator, an exact product (by the oracle's transforms) and a numerator with two zero
    top coefficients"""
    m, nb, cols = MULTI_PASS
    na = m + nb - 1
    b = synth.synth_ints(8200, nb)
    b[-1] = P - 2
    columns = [synth.synth_ints(8201 + c, na) for c in range(cols)]
    columns[1] = oracle_product(synth.synth_ints(8210, m - 1) + [3], b)
    columns[2][-2:] = [0, 0]
    assert all(len(c) == na for c in columns)
    return columns, b


def check_defining_property(columns, b, q, r):
    """a = q b + r with len(r) = nb - 1, column by column: that determines (q, r) uniquely (the long division is too slow here)"""
    m, nb, _ = MULTI_PASS
    for a, qc, rc in zip(columns, q, r):
        qc, rc = synth.unpack_ints(qc), synth.unpack_ints(rc)
        assert len(qc) == m and len(rc) == nb - 1 and max(qc) < P and max(rc) < P
        assert trim(po.poly_add(oracle_product(qc, b), rc)) == trim(a)


def test_columns_multi_pass(sc):
    """the columns form where every transform that matters has more than one pass (above single_pass_max_log = 2^11; the shapes of
    test_columns_match_single are all single-pass): NttOpts::cols > 1 with in_limit < n, the default column stride, columns of X and Y
    at pitch n2 = 2^13 resp. n3 = 2^12.  Every column equals the single-column entry byte for byte and satisfies a = q b + r by the
    oracle's product; the gaps keep the sentinel; leaving out one output leaves the other as it was."""
    m, nb, cols = MULTI_PASS
    assert sc.lib().sc_ntt_num_passes(1 << 12) > 1
    columns, b = multi_pass_columns()
    na, nr = m + nb - 1, nb - 1
    single = [dev_divmod(sc, a, b) for a in columns]
    check_defining_property(columns, b, [s[0] for s in single], [s[1] for s in single])
    assert single[1][1] == bytes(16 * nr)                                   # the exact product
    for ld_a, ld_q, ld_r in ((na, m, nr), (na + 5, m + 3, nr + 2)):
        q, r = dev_divmod_columns(sc, columns, b, ld_a, ld_q, ld_r)
        assert q == [s[0] for s in single], ld_a
        assert r == [s[1] for s in single], ld_a
    check_defining_property(columns, b, q, r)
    q_only, none = dev_divmod_columns(sc, columns, b, na + 5, m + 3, nr + 2, want_r=False)
    assert none is None and q_only == q
    none, r_only = dev_divmod_columns(sc, columns, b, na + 5, m + 3, nr + 2, want_q=False)
    assert none is None and r_only == r


@pytest.mark.parametrize("want_r", [True, False], ids=["with_remainder", "quotient_only"])
def test_columns_multi_pass_in_chunks(sc, want_r):
    """the same three columns with the launch limit lowered to 2^14 values against temporaries of 2^13 per column: sets of 2 and 1
    columns that reuse X and Y, every transform multi-pass"""
    m, nb, cols = MULTI_PASS
    columns, b = multi_pass_columns()
    single = [dev_divmod(sc, a, b) for a in columns]
    sc.set_tuning("div_cols_launch_log", 14)
    try:
        q, r = dev_divmod_columns(sc, columns, b, m + nb + 4, m + 3, nb + 1, want_r=want_r)
    finally:
        sc.set_tuning("div_cols_launch_log", 26)
    assert q == [s[0] for s in single]
    assert r == ([s[1] for s in single] if want_r else None)
    if want_r:
        check_defining_property(columns, b, q, r)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------

def test_errors_leave_outputs_alone(sc):
    na, nb, cols = 40, 9, 2
    m, nr = na - nb + 1, nb - 1
    a = sc.DeviceVector.from_ints(synth.synth_ints(7900, cols * na))
    b = sc.DeviceVector.from_ints(synth.synth_ints(7901, nb - 1) + [5])
    zero_top = sc.DeviceVector.from_ints(synth.synth_ints(7901, nb - 1) + [0])
    q, r = sc.DeviceVector.from_bytes(SENTINEL * (cols * m)), sc.DeviceVector.from_bytes(SENTINEL * (cols * nr))
    one, many, host = sc.lib().sc_poly_divmod_dev, sc.lib().sc_poly_divmod_columns_dev, sc.lib().sc_poly_divmod
    assert one(a.ptr, na, b.ptr, 0, q.ptr, r.ptr, None) == SC_ERR_BAD_ARG                       # nb == 0
    assert one(a.ptr, nb - 1, b.ptr, nb, q.ptr, r.ptr, None) == SC_ERR_BAD_ARG                  # na < nb
    assert one(a.ptr, na, b.ptr, nb, None, None, None) == SC_ERR_BAD_ARG                        # both outputs NULL
    assert one(a.ptr, na, zero_top.ptr, nb, q.ptr, r.ptr, None) == SC_ERR_DIV_ZERO              # b[nb-1] == 0
    assert b"divide by zero" in sc.lib().sc_last_error()
    assert many(a.ptr, na, na, cols, b.ptr, 0, q.ptr, m, r.ptr, nr, None) == SC_ERR_BAD_ARG
    assert many(a.ptr, nb - 1, na, cols, b.ptr, nb, q.ptr, m, r.ptr, nr, None) == SC_ERR_BAD_ARG
    assert many(a.ptr, na, na, cols, b.ptr, nb, None, m, None, nr, None) == SC_ERR_BAD_ARG
    assert many(a.ptr, na, na, cols, zero_top.ptr, nb, q.ptr, m, r.ptr, nr, None) == SC_ERR_DIV_ZERO
    assert many(a.ptr, na, na - 1, cols, b.ptr, nb, q.ptr, m, r.ptr, nr, None) == SC_ERR_BAD_ARG      # short pitches
    assert many(a.ptr, na, na, cols, b.ptr, nb, q.ptr, m - 1, r.ptr, nr, None) == SC_ERR_BAD_ARG
    assert many(a.ptr, na, na, cols, b.ptr, nb, q.ptr, m, r.ptr, nr - 1, None) == SC_ERR_BAD_ARG
    assert many(a.ptr, na, na, cols, b.ptr, nb, a.ptr, m, r.ptr, nr, None) == SC_ERR_BAD_ARG          # an output over an operand
    assert many(a.ptr, na, na, cols, b.ptr, nb, q.ptr, m, q.ptr, nr, None) == SC_ERR_BAD_ARG          # the outputs over each other
    assert many(a.ptr, na, na, 0, b.ptr, nb, q.ptr, m, r.ptr, nr, None) == 0                          # no columns: fine, nothing happens
    hq, hr = ctypes.create_string_buffer(SENTINEL * m), ctypes.create_string_buffer(SENTINEL * nr)
    pa, pb = synth.pack_ints(synth.synth_ints(7900, na)), synth.pack_ints(synth.synth_ints(7901, nb - 1) + [0])
    assert host(pa, na, pb, 0, hq, hr) == SC_ERR_BAD_ARG
    assert host(pa, nb - 1, pb, nb, hq, hr) == SC_ERR_BAD_ARG
    assert host(pa, na, pb, nb, None, None) == SC_ERR_BAD_ARG
    assert host(pa, na, pb, nb, hq, hr) == SC_ERR_DIV_ZERO
    assert hq.raw[:16 * m] == SENTINEL * m and hr.raw[:16 * nr] == SENTINEL * nr
    assert q.to_bytes() == SENTINEL * (cols * m) and r.to_bytes() == SENTINEL * (cols * nr)          # none of these wrote anything
    # a short pitch that is not used is no error: one column's pitch, and the pitch of an output left out
    assert many(a.ptr, na, na, 1, b.ptr, nb, q.ptr, m, None, 0, None) == 0
    want_q, _ = cases.expected(synth.synth_ints(7900, na), synth.synth_ints(7901, nb - 1) + [5])
    assert synth.unpack_ints(q.to_bytes(0, m)) == want_q


# ---- 6. the host API --------------------------------------------------------------------------------------------------------------

def _poly(values):
    from algebra import Field, FieldElement
    from univariate import Polynomial
    field = Field.main()
    return Polynomial([FieldElement(v, field) for v in values])


def _same(got, want):
    """values AND list lengths of a (quotient, remainder) pair"""
    assert (got is None) == (want is None)
    if want is not None:
        for g, w in zip(got, want):
            assert [c.value for c in g.coefficients] == [c.value for c in w.coefficients]


def host_api_operands():
    a, b = synth.synth_ints(8000, 100), synth.synth_ints(8001, 40)
    q = synth.synth_ints(8002, 61)
    return [
        (a, b),
        (a + [0, 0, 0], b),                            # trailing zeros on the numerator's list
        (a, b + [0, 0]),                               # ... on the denominator's: the remainder's list grows
        (a + [0], b + [0, 0, 0]),
        (a[:97] + [0, 0, 0], b),                       # ... and inside the numerator's length
        (po.schoolbook_mul(q, b), b),                  # exact
        (b, a),                                        # deg n < deg d
        (a, [0] * 5),                                  # a zero denominator
        (a, [7]),                                      # a constant
        (a[:40], b),                                   # equal degrees
        (a[:6], b[:3]),                                # short: the long division
        ([0] * 4, b),                                  # a zero numerator
    ]


def test_host_api(sc):
    from ntt import DevicePolynomial, divide_columns_device, fast_divide, fast_divide_columns
    for a, b in host_api_operands():
        n, d = _poly(a), _poly(b)
        _same(fast_divide(n, d), n._schoolbook_divide(d))
    a, b = synth.synth_ints(8000, 100), synth.synth_ints(8001, 40)
    numerators = [_poly(a), _poly(a[:70] + [0] * 5), _poly(a[:20]), _poly(a[5:] + [0]), _poly([0] * 3), _poly(a[:40])]
    for d in (_poly(b), _poly(b + [0, 0]), _poly([3]), _poly([0, 0])):
        got = fast_divide_columns(numerators, d)
        assert len(got) == len(numerators)
        for g, n in zip(got, numerators):
            _same(g, n._schoolbook_divide(d))
    assert fast_divide_columns([], _poly(b)) == []
    # resident operands
    n, d = _poly(a + [0, 0]), _poly(b + [0])
    want_q, want_r = n._schoolbook_divide(d)
    q, r = DevicePolynomial.from_polynomial(n).divmod(DevicePolynomial.from_polynomial(d))
    assert len(q) == 61 and len(r) == 39 and q.degree() == 60
    assert [c.value for c in q.to_polynomial().coefficients] == [c.value for c in want_q.coefficients]
    assert [c.value for c in r.to_polynomial().coefficients] == [c.value for c in want_r.coefficients[:39]]
    low = DevicePolynomial.from_polynomial(_poly(a[:10]))
    q, r = low.divmod(DevicePolynomial.from_polynomial(d))
    assert len(q) == 0 and r is low
    with pytest.raises(AssertionError, match="cannot divide by zero polynomial"):
        low.divmod(DevicePolynomial.from_polynomial(_poly([0, 0])))
    # many resident numerators of different lengths, one divisor
    dev = [DevicePolynomial.from_polynomial(p) for p in numerators if p.coefficients]
    divisor = DevicePolynomial.from_polynomial(d)
    quos, rems = divide_columns_device(dev, divisor)
    for p, q, r in zip(dev, quos, rems):
        want_q, want_r = p.to_polynomial()._schoolbook_divide(d)
        wq = [c.value for c in want_q.coefficients]
        assert len(q) == 61 and len(r) == 39
        assert [c.value for c in q.to_polynomial().coefficients] == wq + [0] * (61 - len(wq))
        assert [c.value for c in r.to_polynomial().coefficients] == ([c.value for c in want_r.coefficients] + [0] * 39)[:39]
        assert q.degree() == len(wq) - 1
    only_q, none = divide_columns_device(dev, divisor, remainders=False)
    assert none is None and [q.vec.to_bytes() for q in only_q] == [q.vec.to_bytes() for q in quos]
    none, only_r = divide_columns_device(dev, divisor, quotients=False)
    assert none is None and [r.vec.to_bytes() for r in only_r] == [r.vec.to_bytes() for r in rems]
    one_q, one_r = divide_columns_device(dev[:1], divisor)
    assert one_q[0].vec.to_bytes() == quos[0].vec.to_bytes() and one_r[0].vec.to_bytes() == rems[0].vec.to_bytes()


# ---- 7. the dispatch of Polynomial.divide -----------------------------------------------------------------------------------------

def test_dispatch(sc, monkeypatch):
    import ntt as ntt_mod
    from univariate import Polynomial
    monkeypatch.setattr(Polynomial, "FAST_DIV_MIN_LEN", 32)
    calls = []
    real = ntt_mod.fast_divide
    monkeypatch.setattr(ntt_mod, "fast_divide", lambda n, d: calls.append((len(n.coefficients), len(d.coefficients))) or real(n, d))
    a, b = synth.synth_ints(8100, 100), synth.synth_ints(8101, 40)
    n, d = _poly(a), _poly(b)
    _same(n.divide(d), n._schoolbook_divide(d))
    assert calls == [(100, 40)]
    assert [c.value for c in (n % d).coefficients] == [c.value for c in n._schoolbook_divide(d)[1].coefficients]
    assert calls == [(100, 40)] * 2
    q = _poly(synth.synth_ints(8102, 61))
    product = _poly(po.schoolbook_mul([c.value for c in q.coefficients], b))
    assert [c.value for c in (product / d).coefficients] == [c.value for c in q.coefficients]
    assert calls == [(100, 40)] * 3
    with pytest.raises(AssertionError, match="cannot perform polynomial division because remainder is not zero"):
        n / d
    assert len(calls) == 4
    # trailing zeros do not count: the decision is on degrees
    _same(_poly(a + [0] * 4).divide(_poly(b + [0])), _poly(a + [0] * 4)._schoolbook_divide(_poly(b + [0])))
    assert calls[4:] == [(104, 41)]
    # below the threshold on either side: the long division
    for short_n, short_d in ((a[:70], b), (a, b[:31]), (a[:62] + [0] * 38, b), (a, b[:20] + [0] * 20)):
        _same(_poly(short_n).divide(_poly(short_d)), _poly(short_n)._schoolbook_divide(_poly(short_d)))
    assert len(calls) == 5
    assert _poly(a).divide(_poly([0] * 40)) is None and len(calls) == 5

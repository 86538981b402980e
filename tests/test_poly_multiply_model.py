"""The products, powers and products of many the device runs (tests/emu/poly_multiply_model.py mirrors polymul_columns, polypow and
polyproduct of csrc/polytree_geo.hip and the kernels of csrc/polymul.cuh array by array) against exact products of Python integers
(tests/emu/poly_multiply_cases.py: the schoolbook product, Kronecker substitution above 512 coefficients).  Pins the chosen
transform size, the zero extension, the sets of columns, the tree's levels and its odd carry.  CPU only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
from oracle import py_oracle as po
import poly_multiply_cases as cases
import poly_multiply_model as pmm
import synth

P = po.P


def test_kronecker_is_the_schoolbook_product():
    for na, nb in ((1, 1), (3, 40), (64, 64), (513, 7)):
        a, b = synth.synth_ints(9100 + na, na), synth.synth_ints(9101 + nb, nb)
        a[0], b[-1] = P - 1, P - 1
        assert cases.kronecker(a, b) == cases.schoolbook(a, b) == po.schoolbook_mul(a, b)
    worst = [P - 1] * 300
    assert cases.kronecker(worst, worst) == cases.schoolbook(worst, worst)          # the fullest slots


@pytest.mark.parametrize("na,nb", cases.MUL_SHAPES)
def test_product_matches_exact(na, nb):
    n = 1 << pmm.transform_log(na + nb - 1)
    assert n >= na + nb - 1 and (n == 2 or n // 2 < na + nb - 1)
    for (label, a, b), want in zip(cases.mul_operands(na, nb), cases.mul_expected(na, nb)):
        got = pmm.multiply_model(a, b)
        assert len(got) == na + nb - 1 and got == want, (na, nb, label)
        if label == "general" and n >= 4 and max(na, nb) <= 64:
            # one step smaller and the product wraps: the shapes are chosen so that it would show
            assert pmm.wrapped_product(a, b) != want[:n // 2], (na, nb)


def test_square_matches_exact():
    for n in (2, 5, 33):
        a = cases.square_operand(n)
        assert pmm.multiply_model(a, a) == cases.exact_product(a, a)


@pytest.mark.parametrize("cols", cases.COLUMN_COUNTS)
@pytest.mark.parametrize("na,nb", cases.COLUMN_SHAPES)
def test_columns_match_exact(na, nb, cols):
    columns, others = cases.column_operands(na, nb, cols)
    want_shared = [cases.exact_product(a, others[0]) for a in columns]
    want_each = [cases.exact_product(a, b) for a, b in zip(columns, others)]
    assert pmm.multiply_columns_model(columns, others[0]) == want_shared
    assert pmm.multiply_columns_model(columns, others) == want_each


def test_columns_in_sets():
    # transforms of 2^7, 2^8 values per set: five columns go as 2 + 2 + 1
    columns, others = cases.column_operands(33, 33, 5)
    for multiplicands in (others[0], others):
        trace = []
        got = pmm.multiply_columns_model(columns, multiplicands, launch_log=8, trace=trace)
        assert trace == [(128, [2, 2, 1])]
        assert got == pmm.multiply_columns_model(columns, multiplicands)
    assert pmm.per_set(128) == 65535 and pmm.per_set(1 << 26) == 1 and pmm.per_set(1 << 30) == 1 and pmm.per_set(1 << 12) == 1 << 14


@pytest.mark.parametrize("na,exponent", cases.POW_SHAPES)
def test_power_matches_exact(na, exponent):
    for (label, a), want in zip(cases.pow_operands(na, exponent), cases.pow_expected(na, exponent)):
        got = pmm.power_model(a, exponent)
        assert len(got) == exponent * (na - 1) + 1 and got == want, (na, exponent, label)


def test_power_of_zero():
    # the ABI's answer (Polynomial.__xor__ answers the empty polynomial before the device is asked)
    assert pmm.power_model([0] * 4, 0) == [1]
    assert pmm.power_model([0] * 4, 1) == [0] * 4
    assert pmm.power_model([0] * 4, 3) == [0] * 10


@pytest.mark.parametrize("count,n", cases.PRODUCT_SHAPES)
def test_product_of_many_matches_exact(count, n):
    rows = [list(r) for r in cases.product_rows(count, n)]
    got = pmm.product_model(rows)
    assert len(got) == count * (n - 1) + 1 and got == cases.product_expected(count, n)


def test_product_levels_and_carries():
    # (rows, length, out_length, transform size)
    assert pmm.product_levels(1, 4) == []
    assert pmm.product_levels(2, 4) == [(2, 4, 7, 8)]
    assert pmm.product_levels(3, 4) == [(3, 4, 7, 8), (2, 7, 10, 16)]
    assert pmm.product_levels(5, 2) == [(5, 2, 3, 4), (3, 3, 5, 8), (2, 5, 6, 8)]
    assert pmm.product_levels(7, 3) == [(7, 3, 5, 8), (4, 5, 9, 16), (2, 9, 15, 16)]
    assert pmm.product_levels(64, 2)[-1] == (2, 33, 65, 128)
    # 17 rows of 129: the last level multiplies the product of 16 rows by the row carried up four times, at the result's size
    assert pmm.product_levels(17, 129) == [(17, 129, 257, 512), (9, 257, 513, 1024), (5, 513, 1025, 2048), (3, 1025, 2049, 4096), (2, 2049, 2177, 4096)]
    trace = []
    pmm.product_model([list(r) for r in cases.product_rows(7, 3)], trace=trace)
    assert trace == [(8, [6], True), (16, [4], False), (16, [2], False)]
    trace = []
    got = pmm.product_model([list(r) for r in cases.product_rows(7, 3)], launch_log=4, trace=trace)
    assert trace == [(8, [2, 2, 2], True), (16, [2, 2], False), (16, [2], False)]
    assert got == cases.product_expected(7, 3)

"""The division with remainder the device runs (tests/emu/poly_divide_model.py mirrors polydiv_columns of csrc/polytree_geo.hip and
the kernels of csrc/polydiv.cuh array by array: Newton doubling of rev(b)^-1, rev(q) = rev(a) h mod y^m, the remainder as a cyclic
product at the divisor's size) against the oracle's restatement of the reference's long division (code/univariate.py:80-97).
Pins the precision doubling, the truncation lengths and the transform sizes.  CPU only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
from oracle import py_oracle as po
import poly_divide_cases as cases
import poly_divide_model as pdm

P = po.P


@pytest.mark.parametrize("nb", cases.NB_GRID)
@pytest.mark.parametrize("m", cases.M_GRID)
def test_model_matches_oracle(m, nb):
    for label, a, b in cases.operands(m, nb):
        want_q, want_r = cases.expected(a, b)
        q, r = pdm.divmod_model(a, b)
        assert q == want_q, (m, nb, label)
        assert r == want_r, (m, nb, label)
        if label == "exact product":
            assert not any(r), (m, nb)


def test_outputs_left_out():
    a, b = cases.operands(33, 31)[0][1:]
    q, r = pdm.divmod_model(a, b)
    assert pdm.divmod_model(a, b, want_r=False) == (q, None)
    assert pdm.divmod_model(a, b, want_q=False) == (None, r)


def test_shapes():
    # (m, nr, g, logP, log2, log3): the transform of step 2 holds 2m - 1 coefficients, the one of step 3 the divisor; both at least 2
    assert pdm.shape(1, 1) == (1, 0, 1, 0, 1, 1)
    assert pdm.shape(100, 100) == (1, 99, 1, 0, 1, 7)
    assert pdm.shape(64, 32) == (33, 31, 32, 6, 7, 5)
    assert pdm.shape(64, 33) == (32, 32, 32, 5, 6, 6)
    assert pdm.shape(164, 100) == (65, 99, 65, 7, 8, 7)


def test_series_is_the_inverse():
    # h * rev(b) = 1 mod y^m, for a non-monic divisor and an m that is no power of two
    m, nb = 33, 31
    _, a, b = cases.operands(m, nb)[1]
    h = pdm.inverse_series(b, len(a))[:m]
    prod = po.schoolbook_mul(h, b[::-1])[:m]
    assert prod == [1] + [0] * (m - 1)

"""GPU tests of the host API for many columns per call (ntt.py: ntt_columns, intt_columns, fast_coset_evaluate_columns,
fast_interpolate_columns, fast_interpolate_columns_device, DevicePolynomial.degrees): each returns exactly what the per-column
function returns for each member, and refuses what it refuses."""
import pytest

from conftest import load_golden
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import ntt as ntt_mod                               # noqa: E402
from ntt import (ntt, intt, ntt_columns, intt_columns, fast_coset_evaluate, fast_coset_evaluate_columns, fast_interpolate,      # noqa: E402
                 fast_interpolate_columns, fast_interpolate_columns_device, fast_interpolate_device, DeviceDomain, DevicePolynomial)
from algebra import Field, FieldElement            # noqa: E402
from univariate import Polynomial                  # noqa: E402
import starkcore as sc                              # noqa: E402

field = Field.main()


def elements(seed, n):
    return [FieldElement(v, field) for v in synth.synth_ints(seed, n)]


@pytest.mark.parametrize("cols", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 8, 1024])
def test_transform_columns_equal_the_loop(n, cols):
    root = field.primitive_nth_root(n) if n > 1 else field.one()
    columns = [elements(100 + c, n) for c in range(cols)]
    forward = ntt_columns(root, columns)
    assert forward == [ntt(root, c) for c in columns]
    assert intt_columns(root, forward) == [intt(root, c) for c in forward] == columns
    assert all(isinstance(c, list) and len(c) == n for c in forward)


@pytest.mark.parametrize("logn", [3, 10])
def test_transform_columns_against_the_reference_goldens(logn):
    """the reference's ntt / intt of the seeded inputs of tests/golden/ntt.json (SHA-256 of the packed output) as the middle column of three"""
    import hashlib
    g = load_golden("ntt.json")
    n = 1 << logn
    for kind, transform in (("ntt", ntt_columns), ("intt", intt_columns)):
        records = [r for r in g[kind] if r["logn"] == logn]
        assert records
        for rec in records:
            root = FieldElement(int(rec["root"]), field)
            got = transform(root, [elements(200, n), elements(rec["seed"], n), elements(201, n)])
            assert hashlib.sha256(synth.pack_ints([v.value for v in got[1]])).hexdigest() == rec["sha256"], (kind, rec["seed"])
            if "out" in rec:
                assert [str(v.value) for v in got[1]] == rec["out"]


def test_coset_evaluate_columns_pads_shorter_lists():
    order = 64
    generator, offset = field.primitive_nth_root(order), field.generator()
    polynomials = [Polynomial(elements(300, 17)), Polynomial(elements(301, 1)), Polynomial(elements(302, 64)), Polynomial([]),
                   Polynomial(elements(303, 5) + [field.zero()] * 3)]
    got = fast_coset_evaluate_columns(polynomials, offset, generator, order)
    assert got == [fast_coset_evaluate(p, offset, generator, order) for p in polynomials]
    assert fast_coset_evaluate_columns([Polynomial([])], offset, generator, order) == [[field.zero()] * order]
    assert fast_coset_evaluate_columns([polynomials[1]], offset, generator, order) == [fast_coset_evaluate(polynomials[1], offset, generator, order)]
    # an order of one goes the per-polynomial way (the reference's own formula on the host) and gives its answers
    short = [Polynomial(elements(304, 1)), Polynomial([])]
    assert fast_coset_evaluate_columns(short, offset, field.one(), 1) == [fast_coset_evaluate(p, offset, field.one(), 1) for p in short]


def test_interpolate_columns_on_a_progression_and_on_other_points():
    order = 128
    root = field.primitive_nth_root(order)
    n, cols = 40, 3
    progression = [root ^ i for i in range(n)]
    scattered = elements(400, n)
    values = [elements(401 + c, n) for c in range(cols)]
    assert isinstance(ntt_mod._device_tree(progression), sc.GeoDomain) and isinstance(ntt_mod._device_tree(scattered), sc.PolyTree)
    for domain in (progression, scattered):
        got = fast_interpolate_columns(domain, values, root, order)
        want = [fast_interpolate(domain, v, root, order) for v in values]
        assert [p.coefficients for p in got] == [p.coefficients for p in want]
    # below the size that goes to the device at all: the reference's recursion per column
    small = fast_interpolate_columns(progression[:5], [v[:5] for v in values], root, order)
    assert [p.coefficients for p in small] == [fast_interpolate(progression[:5], v[:5], root, order).coefficients for v in values]


def test_interpolate_columns_device_returns_views_of_one_matrix():
    order, n, cols = 128, 40, 5
    root = field.primitive_nth_root(order)
    domain = DeviceDomain.geometric(field.one(), root, n)
    assert isinstance(domain.tree, sc.GeoDomain)
    separate = [sc.DeviceCodeword.from_list(elements(500 + c, n), field) for c in range(cols)]
    want = [fast_interpolate_device(domain, v).vec.to_bytes() for v in separate]
    got = fast_interpolate_columns_device(domain, separate)
    assert [g.vec.to_bytes() for g in got] == want
    assert [g.vec.ptr for g in got] == [got[0].vec.ptr + 16 * n * c for c in range(cols)]      # rows of ONE matrix
    # columns that already are the consecutive rows of one matrix are not copied first: the results are fed back in
    again = fast_interpolate_columns_device(domain, got)
    assert [a.vec.to_bytes() for a in again] == [fast_interpolate_device(domain, g).vec.to_bytes() for g in got]
    # degrees of the rows in one call, against the single form
    polynomials = [DevicePolynomial.from_codeword(g) for g in got]
    assert DevicePolynomial.degrees(polynomials) == [DevicePolynomial.from_codeword(g).degree() for g in got]
    assert all(p._degree is not None for p in polynomials)
    # a tree domain: the per-column loop, same answers as the single entry
    tree_domain = DeviceDomain(elements(510, n))
    assert isinstance(tree_domain.tree, sc.PolyTree)
    looped = fast_interpolate_columns_device(tree_domain, separate)
    assert [l.vec.to_bytes() for l in looped] == [fast_interpolate_device(tree_domain, v).vec.to_bytes() for v in separate]


def test_degrees_fills_only_what_is_unknown_and_handles_scattered_members():
    a = DevicePolynomial.from_polynomial(Polynomial(elements(600, 7) + [field.zero()] * 2))
    b = DevicePolynomial(sc.DeviceVector.from_bytes(synth.pack_ints(synth.synth_ints(601, 9))), field)
    c = DevicePolynomial(sc.DeviceVector.zeros(9), field)
    assert a._degree == 6 and b._degree is None
    assert DevicePolynomial.degrees([a, b, c]) == [6, 8, -1]
    assert DevicePolynomial.degrees([]) == []


def test_empty_input():
    root = field.primitive_nth_root(8)
    assert ntt_columns(root, []) == [] and intt_columns(root, []) == []
    assert fast_coset_evaluate_columns([], field.generator(), root, 8) == []
    assert fast_interpolate_columns([root ^ i for i in range(4)], [], root, 8) == []
    assert fast_interpolate_columns_device(DeviceDomain.geometric(field.one(), root, 4), []) == []


def test_unequal_lengths_raise_before_any_library_call(monkeypatch):
    calls = []

    class Recorder:
        def __getattr__(self, name):
            calls.append(name)
            raise AssertionError("the library was reached: " + name)
    root = field.primitive_nth_root(8)
    monkeypatch.setattr(sc, "lib", lambda: Recorder())
    for transform in (ntt_columns, intt_columns):
        with pytest.raises(AssertionError, match="one length"):
            transform(root, [elements(700, 8), elements(701, 4)])
    with pytest.raises(AssertionError, match="cannot interpolate over domain of different length than values list"):
        fast_interpolate_columns([root ^ i for i in range(4)], [elements(702, 4), elements(703, 3)], root, 8)
    assert calls == []

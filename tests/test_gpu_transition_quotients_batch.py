"""FastStark.transition_quotients_batch: the transition quotients of the members of a batch of proofs, the work of each value-domain
order done for all members in one call per step.  Per member and constraint the coefficients and the degree are those of the
per-member method (_transition_quotients_on_device), for the smallest instance also those of the host route (evaluate_symbolic, then
fast_coset_divide); the library calls are counted; a false witness in one member of three leaves the other two alone."""
import os
import random

import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import starkcore as sc                              # noqa: E402
import synth                                        # noqa: E402
import workloads                                    # noqa: E402
from algebra import Field, FieldElement             # noqa: E402
from fast_stark import FastStark                    # noqa: E402
from multivariate import MPolynomial                # noqa: E402
from ntt import DevicePolynomial, _shrink_order, fast_coset_divide, fast_interpolate_columns_device    # noqa: E402
from rescue_prime import RescuePrime                # noqa: E402
from starkcore import DeviceCodeword, DeviceVector  # noqa: E402
from univariate import Polynomial                   # noqa: E402

field = Field.main()


@pytest.fixture(autouse=True)
def forced_batches(monkeypatch):
    monkeypatch.setattr(FastStark, "COLUMN_BATCH_MIN", 2)


def seeded_urandom(monkeypatch, seed):
    rng = random.Random(seed)
    monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))


class Instance:
    """K members of one AIR: stark, air, the transition zerofier, and per member the randomized trace as host columns"""


def randomized(stark, columns):
    """the columns of one member with the randomizer rows appended, drawn as `prove` draws them: row by row, register by register"""
    extra = [[field.sample(os.urandom(17)).value for _ in columns] for _ in range(stark.num_randomizers)]
    return [list(column) + [row[s] for row in extra] for s, column in enumerate(columns)]


def rescue_instance(K, monkeypatch):
    rec = load_golden("fast_stark.json")["runs"][0]
    seeded_urandom(monkeypatch, rec["urandom_seed"])
    rp = RescuePrime()
    inst = Instance()
    inst.stark = FastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"], rp.m, rp.N + 1)
    assert (inst.stark.omicron_domain_length, inst.stark.fri_domain_length) == (rec["omicron_domain_length"], rec["fri_domain_length"])
    inst.air = rp.transition_constraints(inst.stark.omicron)
    inst.zerofier = inst.stark.preprocess()[0]
    inst.columns = []
    for m in range(K):
        rows = rp.trace(FieldElement(int(rec["input"]) + 977 * m, field))
        inst.columns.append(randomized(inst.stark, [[row[s].value for row in rows] for s in range(rp.m)]))
    return inst


def synthetic_instance(K, monkeypatch):
    rec = [r for r in load_golden("fast_stark_synth.json")["runs"] if r["log_fri"] == 10][0]
    seeded_urandom(monkeypatch, rec["urandom_seed"])
    s = rec["num_colinearity_checks"]
    _, T, _, air, _ = workloads.synthetic_stark_instance(10, s)
    inst = Instance()
    inst.stark = FastStark(field, rec["expansion_factor"], s, rec["security_level"], 2, T)
    assert inst.stark.fri_domain_length == 1 << 10
    inst.air = air
    inst.zerofier = inst.stark.preprocess()[0]
    # members: the AIR's trace from different starting rows
    inst.columns = [randomized(inst.stark, synth.synthetic_air_columns(T, 3 + 2 * m, 5 + m)) for m in range(K)]
    return inst


def points_of(inst, columns=None):
    """the members' points as `prove` builds them, the trace polynomials of ALL members interpolated as one matrix of K R columns"""
    stark = inst.stark
    columns = inst.columns if columns is None else columns
    flat = [column for member in columns for column in member]
    rows = len(flat[0])
    matrix = DeviceVector.from_ints([v for column in flat for v in column])
    views = [DeviceCodeword(DeviceVector.wrap(matrix.ptr + 16 * rows * c, rows, matrix), field) for c in range(len(flat))]
    polynomials = [DevicePolynomial.from_codeword(c) for c in fast_interpolate_columns_device(stark._trace_domain(rows), views)]
    DevicePolynomial.degrees(polynomials)
    x = DevicePolynomial.from_polynomial(Polynomial([field.zero(), field.one()]), field)
    R = stark.num_registers
    points = []
    for m in range(len(columns)):
        mine = polynomials[m * R:(m + 1) * R]
        points.append([x] + mine + [tp.scaled_later(stark.omicron) for tp in mine])
    return points


def as_data(quotients):
    """[(list length, degree, coefficient bytes)]"""
    return [(len(q), q.degree(), q.vec.to_bytes(0, len(q)) if len(q) else b"") for q in quotients]


def per_member(inst, points, pending=None):
    zerofier = inst.stark._lift(inst.zerofier)
    return [as_data(inst.stark._transition_quotients_on_device(inst.air, point, zerofier, pending, True)) for point in points]


def order_groups(inst, points):
    """the value-domain orders the constraints fall into (as _transition_quotients_on_device groups them)"""
    stark = inst.stark
    degrees = [q.degree() for q in points[0]]
    dr = stark._lift(inst.zerofier).degree()
    orders = set()
    for a in inst.air:
        bound, _ = a.value_domain_terms(degrees)
        assert bound >= max(dr, MPolynomial.VALUE_DOMAIN_MIN_DEGREE)
        orders.add(_shrink_order(stark.omicron, stark.omicron_domain_length, max(bound, dr))[1])
    return orders


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


def batch_with_census(inst, points, monkeypatch, pending=None):
    census = Census(sc.lib())
    with monkeypatch.context() as mp:
        mp.setattr(sc, "lib", lambda: census)
        got = inst.stark.transition_quotients_batch(inst.air, points, inst.zerofier, pending)
    return got, census.calls


def check_census(calls, groups, evaluations):
    assert calls.get("sc_mpoly_eval_columns_dev", 0) == groups
    assert calls.get("sc_mpoly_eval_rot_dev", 0) == 0
    assert calls.get("sc_pointwise_div_columns_later_dev", 0) == groups
    assert calls.get("sc_pointwise_div_later_dev", 0) == calls.get("sc_pointwise_div_dev", 0) == 0
    assert calls.get("sc_ntt_columns_dev", 0) == groups
    assert calls.get("sc_ntt_dev", 0) == 0
    assert calls.get("sc_scale_columns_dev", 0) == groups and calls.get("sc_scale_dev", 0) == 0
    assert calls.get("sc_vec_degree_columns_dev", 0) == groups and calls.get("sc_vec_degree_dev", 0) == 0
    assert calls.get("sc_coset_evaluate_columns_dev", 0) == evaluations


@pytest.mark.parametrize("K", [1, 2, 5])
def test_rescue_prime_members_equal_the_per_member_method(K, monkeypatch):
    inst = rescue_instance(K, monkeypatch)
    points = points_of(inst)
    want = per_member(inst, points)
    groups = order_groups(inst, points)
    assert groups == {inst.stark.omicron_domain_length}        # both constraints on g <omicron>: the scaled copies are turned, not stored
    pending = []
    got, calls = batch_with_census(inst, points, monkeypatch, pending)
    assert len(pending) == 1                                   # one verdict for K members x 2 constraints
    for verdict in pending:
        verdict()
    assert [as_data(q) for q in got] == want
    bounds = inst.stark.transition_quotient_degree_bounds(inst.air)
    for quotients in got:
        assert [q.degree() for q in quotients] == bounds      # honest traces: the degrees `prove` asserts
    # the K R trace polynomials are rows of one matrix: ONE evaluation call for all of them (a single row when K R == 1 goes alone)
    check_census(calls, 1, 1)
    # the quotients are views of the rows of one matrix
    order = inst.stark.omicron_domain_length
    places = [q.vec.ptr for quotients in got for q in quotients]
    assert [p - places[0] for p in places] == [16 * order * c for c in range(len(places))]


@pytest.mark.parametrize("K", [1, 3])
def test_synthetic_members_equal_the_per_member_method_and_the_host_route(K, monkeypatch):
    inst = synthetic_instance(K, monkeypatch)
    points = points_of(inst)
    want = per_member(inst, points)
    groups = order_groups(inst, points)
    assert len(groups) == 2                                    # a linear and a quadratic constraint: two orders
    got, calls = batch_with_census(inst, points, monkeypatch)  # (no list of pending checks: the verdicts are waited for on the spot)
    assert [as_data(q) for q in got] == want
    # Neither order is the omicron domain's (64 and 128 against 256), so the scaled copies are stored, evaluated at the offset
    # g omicron.  Order 64, a' - b: b at g and a' at g omicron, no two rows with one offset.  Order 128, b' - a a - b:
    # a and b are two consecutive rows at g -- one columns call per member --, then b' at g omicron.
    stark = inst.stark
    assert groups == {64, 128} and stark.omicron_domain_length == 256
    check_census(calls, 2, K)
    # the host route on the same polynomials
    x = Polynomial([field.zero(), field.one()])
    for m in range(K):
        trace_polynomials = [q.to_polynomial() for q in points[m][1:3]]
        point = [x] + trace_polynomials + [tp.scale(stark.omicron) for tp in trace_polynomials]
        for a, quotient in zip(inst.air, got[m]):
            host = fast_coset_divide(a.evaluate_symbolic(point), inst.zerofier, stark.generator, stark.omicron, stark.omicron_domain_length)
            assert quotient.to_polynomial() == host and quotient.degree() == host.degree()


def outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:      # noqa: BLE001
        return ("raised", type(e), str(e))


def test_false_witness_in_one_member_of_three(monkeypatch):
    inst = rescue_instance(3, monkeypatch)
    honest = per_member(inst, points_of(inst))
    columns = [[list(column) for column in member] for member in inst.columns]
    columns[1][0][5] = (columns[1][0][5] + 1) % field.p        # one trace entry of member 1
    points = points_of(inst, columns)
    alone = outcome(lambda: as_data(inst.stark._transition_quotients_on_device(inst.air, points[1], inst.stark._lift(inst.zerofier), None, True)))
    together = outcome(lambda: [as_data(q) for q in inst.stark.transition_quotients_batch(inst.air, points, inst.zerofier)])
    # The per-member method does not raise on a false witness: its value-domain pass finds the interpolant longer than bound - deg Z
    # and hands the constraint to coset_divide_device WITHOUT the exactness check (like fast_coset_divide, "clean division only"),
    # which returns the quotient of the division with remainder.  So both calls return, and everything below is checked.
    assert alone[0] == "ok" and together[0] == "ok", (alone, together)
    got = together[1]
    assert got[1] == alone[1]                                  # whatever the per-member method makes of it
    assert got[1] != honest[1]
    assert got[0] == honest[0] and got[2] == honest[2]         # the other two are unaffected
    # ... and those two went through the batched calls, the false one alone through the per-member method
    got_again, calls = batch_with_census(inst, points, monkeypatch)
    assert [as_data(q) for q in got_again] == got
    assert calls.get("sc_mpoly_eval_columns_dev", 0) == 1 and calls.get("sc_pointwise_div_columns_later_dev", 0) == 1
    assert calls.get("sc_mpoly_eval_rot_dev", 0) == len(inst.air)      # member 1's constraints, once more, on its own

"""The cases of tests/rescue_prime_cases.py, proven on the host before tests/test_gpu_rescue_prime_edges.py runs them on the GPU:
the plain-integer model equals the package's mirror of the reference (pinned by tests/golden/), the steered lanes pass through the
states they name -- every table entry in front of a cube and in front of an inverse cube --, the structured inputs have their orders,
and the g++ build of the kernel's own permutation (tests/emu/rescue_emu.cpp over csrc/rescue_prime.cuh) equals the model on every
case, hash and trace, every lane."""
import collections
import ctypes

import pytest

from algebra import FieldElement
import rescue_prime
import rescue_prime_cases as rc
from test_rescue_prime_cpu import emu             # noqa: F401  (the fixture that builds tests/emu/librescue_emu.so)

P = rc.P


def test_constants_of_the_module():
    assert rc.ALPHA * rc.ALPHAINV % (P - 1) == 1
    assert rc.R * rc.RINV % P == 1 and rc.R == (1 << 128) - P
    assert P >> 96 == 0xCB800000                   # why no form below p has an all-one top limb
    forms = {name: v * rc.R % P for name, v in rc.SPECIAL.items()}
    assert forms["form 1"] == 1 and forms["form R^2"] == pow(2, 256, P)
    assert forms["form low32 zero"] & 0xFFFFFFFF == 0 and forms["form low32 zero"] >> 32
    assert forms["form low32 ones"] & 0xFFFFFFFF == 0xFFFFFFFF
    assert forms["form high32 zero"] >> 96 == 0 and forms["form high32 zero"] >> 64
    assert forms["form p-2"] == P - 2 and (P - 2) & ((1 << 96) - 1) == (1 << 96) - 1
    assert forms["form low64 zero"] == 1 << 64 and forms["form low64 ones high64 zero"] == (1 << 64) - 1 and forms["form 2^32"] == 1 << 32
    assert len(set(rc.SPECIAL.values())) == len(rc.SPECIAL) and all(0 < v < P for v in rc.SPECIAL.values())
    assert rc.TABLE[:6] == ((0, 0), (0, 1), (1, 0), (P - 1, P - 1), (1, P - 1), (0, P - 1))


def test_model_equals_the_mirror_of_the_reference():
    rp = rescue_prime.RescuePrime()
    assert rc.REF_MDS == [v.value for row in rp.MDS for v in row] and rc.REF_RC == [v.value for v in rp.round_constants]
    assert rc.pack(rc.REF_MDS + rc.REF_RC) == rp._params
    for x in [0, 1, P - 1, P, P + 1, rc.TOP] + rc.batch(5, 20, 0, 12345) + list(rc.STRUCTURED):
        want = rp.trace(FieldElement(x % P, rp.field))
        assert rc.states(x, rc.REF_MDS, rc.REF_RC, 27) == [[v.value for v in row] for row in want], x
        assert rc.expected_hash([x], rc.REF_MDS, rc.REF_RC, 27) == [rp.hash(FieldElement(x % P, rp.field)).value]
        for rounds in (1, 2, 13):
            assert rc.states(x, rc.REF_MDS, rc.REF_RC[:4 * rounds], rounds) == [[v.value for v in row] for row in want[:rounds + 1]]


def test_steered_lanes_pass_through_their_targets():
    for case in rc.ALL_CASES:
        assert len(case.rc) == 4 * case.rounds and all(0 <= v < P for v in case.rc)
        assert len(case.params) == 16 * (4 + 4 * case.rounds + 1) and rc.unpack(case.params[-16:])[0] >= P
        assert case.inputs[case.k_star] == case.x and len(case.inputs) == case.n
        halves = rc.half_states(case.x, case.mds, case.rc, case.rounds)
        assert halves[0] == [case.x % P, 0]
        assert [tuple(h) for h in halves[1:]] == list(case.targets), case
        assert case.lane_states[case.k_star] == halves[::2]
        # no other lane follows: the targets are the steered lane's alone
        for k, st in enumerate(case.lane_states):
            if k != case.k_star and case.matrix != "zero" and case.inputs[k] % P != case.x % P:
                assert st[1:] != halves[2::2], (case, k)


def test_every_table_entry_stands_in_front_of_both_powers():
    """per table entry: how often it is the state in front of a cube and in front of an inverse cube; per register and scalar value
    of the table likewise.  The last target of a case is the final state: in front of nothing, and not counted."""
    entries = collections.Counter()
    scalars = collections.Counter()
    for case in rc.CASES:
        for j, target in enumerate(case.targets[:-1]):
            power = "inverse cube" if j % 2 == 0 else "cube"      # target j is the state after half-round j: j even follows a cube's mix
            entries[target, power] += 1
            for register in range(2):
                scalars[target[register], register, power] += 1
    for entry in rc.TABLE:
        for power in ("cube", "inverse cube"):
            assert entries[entry, power] > 0, "table entry %r never stands in front of a %s" % (entry, power)
    values = {"0": 0, "1": 1, "p-1": P - 1}
    values.update(rc.SPECIAL)
    for name, v in values.items():
        for register in range(2):
            for power in ("cube", "inverse cube"):
                assert scalars[v, register, power] > 0, "%s never stands in register %d in front of a %s" % (name, register, power)
    structured = collections.Counter()
    case = rc.STRUCTURED_STEERED
    for j, target in enumerate(case.targets[:-1]):
        for register in range(2):
            structured[target[register], register, "inverse cube" if j % 2 == 0 else "cube"] += 1
    for v in rc.STRUCTURED:
        for register in range(2):
            for power in ("cube", "inverse cube"):
                assert structured[v, register, power] > 0, (v, register, power)


def test_every_value_of_every_axis_appears():
    cases = rc.CASES
    assert 90 <= 2 * len(rc.ALL_CASES) + 2 <= 110                            # launches: both entries per case, and the structured inputs
    assert {(c.rounds, c.matrix) for c in cases} == {(r, m) for r in rc.ROUNDS for m in rc.MATRICES}
    assert {c.x for c in cases} == set(rc.STEERED_INPUTS.values()) == {0, 1, P - 1, P, P + 1, rc.TOP, rc.STEERED_INPUTS["seeded"]}
    assert {c.n for c in cases} == set(rc.SIZES) == {1, 2, 64, 255, 256, 257, 513}
    assert {(c.n, c.k_star) for c in cases} >= {(n, k) for n in rc.SIZES for k in rc.positions_of(n)}
    assert {c.k_star for c in cases} >= {0, 63, 64, 255, 256, 512}
    assert len({(c.x, c.n) for c in cases}) == 49
    assert max(c.n for c in rc.ALL_CASES) == 513
    for case in cases:
        if case.n > 4:
            assert sum(x >= P for x in case.inputs) > case.n // 2, case   # most of the other lanes are reduced on load
    # constants equal to 0 and p - 1 are read, and the matrices are what their names say
    assert any(0 in c.rc for c in cases) and any(P - 1 in c.rc for c in cases)
    assert rc.MATRICES["zero"] == [0] * 4 and rc.MATRICES["identity"] == [1, 0, 0, 1] and rc.MATRICES["all p-1"] == [P - 1] * 4
    assert all(0 < v < P - 1 for v in rc.MATRICES["random"])
    assert len({c.name for c in rc.ALL_CASES}) == len(rc.ALL_CASES)
    assert {c.n for c in rc.STREAM_CASES} >= {1, 257, 513} and any(c.rounds == 27 and c.n == 513 for c in rc.STREAM_CASES)


def test_structured_inputs_have_their_orders():
    assert len(rc.STRUCTURED) == 2 * len(rc.ORDERS) == 14
    for d, e, neg in zip(rc.ORDERS, rc.STRUCTURED[0::2], rc.STRUCTURED[1::2]):
        assert 0 < e < P and (e + neg) % P == 0
        assert pow(e, d, P) == 1
        for q in (2, 11, 37):
            if d % q == 0:
                assert pow(e, d // q, P) != 1, (d, q)
        # the negative of an element of odd order d has order 2 d; of order 2, order 1; of a higher two-power order, the same order
        if d == 2:
            assert neg == 1
        else:
            assert rc.has_order(neg, 2 * d if d % 2 else d)
    assert rc.STRUCTURED[0] == P - 1 and rc.STRUCTURED[1] == 1
    assert pow(rc.STRUCTURED[2], 2, P) == P - 1                              # order 4: a square root of -1
    # squarings of an element of order 2^60 reach 1 after 60 of them, midway through the chain's 126
    e = rc.STRUCTURED[10]
    assert pow(e, 1 << 59, P) == P - 1 and pow(e, 1 << 60, P) == 1


def run_emu(emu, case):                            # noqa: F811
    out = ctypes.create_string_buffer(16 * case.n)
    emu.emu_rescue_hash(case.input_bytes, case.n, case.params, case.rounds, out)
    tr = ctypes.create_string_buffer(16 * 2 * case.n * (case.rounds + 1))
    emu.emu_rescue_trace(case.input_bytes, case.n, case.params, case.rounds, tr)
    return out.raw, tr.raw


@pytest.mark.parametrize("case", rc.ALL_CASES + [rc.StructuredInputs], ids=lambda c: c.name)
def test_host_build_of_the_kernel_equals_the_model(emu, case):    # noqa: F811
    got_hash, got_trace = run_emu(emu, case)
    assert got_hash == case.hash
    assert got_trace == case.trace
    rows = case.rounds + 1
    trace = rc.unpack(got_trace)
    # the hash is the last row of the trace's register 0, the first row is the input reduced, register 1 starts at zero
    assert [trace[2 * k * rows + case.rounds] for k in range(case.n)] == rc.unpack(got_hash)
    assert [trace[2 * k * rows] for k in range(case.n)] == [x % P for x in case.inputs]
    assert [trace[(2 * k + 1) * rows] for k in range(case.n)] == [0] * case.n


def test_model_hash_is_the_last_row_of_register_zero():
    for case in rc.ALL_CASES + [rc.StructuredInputs]:
        rows = case.rounds + 1
        trace = rc.unpack(case.trace)
        assert len(trace) == 2 * case.n * rows
        assert [trace[2 * k * rows + case.rounds] for k in range(case.n)] == rc.unpack(case.hash), case
    small = rc.CASES[1]
    assert rc.unpack(small.hash) == rc.expected_hash(small.inputs, small.mds, small.rc, small.rounds)
    assert rc.unpack(small.trace) == rc.expected_trace(small.inputs, small.mds, small.rc, small.rounds)

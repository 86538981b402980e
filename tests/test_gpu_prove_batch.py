"""FastStark.prove_batch: K proofs with the members' work on the device done together.  Under a seeded os.urandom the proofs are those
of K sequential `prove` calls byte for byte -- member 0's is the reference's golden proof -- and verify: Rescue-Prime at FRI 2^9, the
synthetic two-register AIR at FRI 2^10 from DeviceTraces and from host rows, the 16-register AIR; in chunks when FOREST_MAX_LEAVES is
small; on streams that already hold an object; K = 1 and the empty batch; batches that are not served fall back to `prove`; a false
witness raises what `prove` raises for that member and leaves no verdict slot behind; the forests and library calls are counted."""
import functools
import hashlib
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
from fast_rpsss import SignatureProofStream         # noqa: E402
from fast_stark import DeviceTrace, FastStark       # noqa: E402
from ip import ProofStream                          # noqa: E402
from rescue_prime import RescuePrime                # noqa: E402

field = Field.main()


@pytest.fixture
def seeded(monkeypatch):
    """os.urandom -> the generator the golden runs were drawn with"""
    def seed(value):
        rng = random.Random(value)
        monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    return seed


class Instance:
    """K members of one AIR: the prover, its preprocessing (from host lists and device-resident), the members' traces as host rows,
    their boundaries, the golden record whose proof member 0's is"""

    def __init__(self, rec, stark, air, rows, boundaries):
        self.rec, self.stark, self.air, self.rows, self.boundaries = rec, stark, air, rows, boundaries
        self.host, self.resident = stark.preprocess(), stark.preprocess(device_resident=True)
        assert self.host[2].hex() == self.resident[2].hex() == rec["zerofier_root"]
        self.seed = rec["urandom_seed"]

    def traces(self, how):
        return [DeviceTrace.from_rows(rows, field) for rows in self.rows] if how == "device" else [list(rows) for rows in self.rows]

    def sequential(self, seeded, how="host", streams=None, rows=None, boundaries=None):
        """K calls of `prove` under the instance's seed"""
        seeded(self.seed)
        pre = self.resident if how == "device" else self.host
        traces = self.traces(how) if rows is None else rows
        streams = [None] * len(traces) if streams is None else streams
        return [self.stark.prove(trace, self.air, boundary, pre[0], pre[1], stream)
                for trace, boundary, stream in zip(traces, self.boundaries if boundaries is None else boundaries, streams)]

    def batch(self, seeded, how="host", streams=None, rows=None, boundaries=None):
        seeded(self.seed)
        pre = self.resident if how == "device" else self.host
        return self.stark.prove_batch(self.traces(how) if rows is None else rows, self.air, self.boundaries if boundaries is None else boundaries,
                                      pre[0], pre[1], streams)

    def all_verify(self, proofs, boundaries=None):
        return self.stark.verify_batch(proofs, self.air, self.boundaries if boundaries is None else boundaries, self.host[2])


@functools.lru_cache(maxsize=None)
def rescue(K=3):
    rec = load_golden("fast_stark.json")["runs"][0]
    rp = RescuePrime()
    stark = FastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"], rp.m, rp.N + 1)
    assert stark.fri_domain_length == rec["fri_domain_length"] == 1 << 9
    inputs = [FieldElement(int(rec["input"]) + 977 * m, field) for m in range(K)]
    return Instance(rec, stark, rp.transition_constraints(stark.omicron), [rp.trace(x) for x in inputs], [rp.boundary_constraints(rp.hash(x)) for x in inputs])


@functools.lru_cache(maxsize=None)
def synthetic(K=3):
    rec = [r for r in load_golden("fast_stark_synth.json")["runs"] if r["log_fri"] == 10][0]
    s = rec["num_colinearity_checks"]
    _, T, _, air, _ = workloads.synthetic_stark_instance(10, s)
    stark = FastStark(field, rec["expansion_factor"], s, rec["security_level"], 2, T)
    rows, boundaries = [], []
    for m in range(K):                                 # the AIR's trace from different starting rows; member 0 is the golden's
        a, b = synth.synthetic_air_columns(T, 3 + 2 * m, 5 + m)
        rows.append([[FieldElement(x, field), FieldElement(y, field)] for x, y in zip(a, b)])
        boundaries.append([(0, 0, FieldElement(a[0], field)), (0, 1, FieldElement(b[0], field)), (T - 1, 1, FieldElement(b[T - 1], field))])
    return Instance(rec, stark, air, rows, boundaries)


@functools.lru_cache(maxsize=None)
def wide(K=2):
    rec = [r for r in load_golden("fast_stark_wide.json")["runs"] if r["log_fri"] == 10][0]
    w, s = rec["registers"], rec["num_colinearity_checks"]
    _, T, _, _, air, _ = workloads.synthetic_wide_instance(10, w, s)
    stark = FastStark(field, rec["expansion_factor"], s, rec["security_level"], w, T)
    rows, boundaries = [], []
    for m in range(K):                                 # workloads.synthetic_wide_columns from row 0 = (7 i + 3 + m): member 0 is the golden's
        row = [7 * i + 3 + m for i in range(w)]
        mine = [row]
        for _ in range(T - 1):
            row = [(row[i] * row[i] + row[(i + 1) % w]) % field.p for i in range(w)]
            mine.append(row)
        rows.append([[FieldElement(v, field) for v in row] for row in mine])
        boundaries.append([(0, i, FieldElement(mine[0][i], field)) for i in range(w)] + [(T - 1, 0, FieldElement(mine[T - 1][0], field))])
    return Instance(rec, stark, air, rows, boundaries)


CASES = {"rescue-prime": (rescue, "host"), "rescue-prime-device": (rescue, "device"), "synthetic-host-rows": (synthetic, "host"),
         "synthetic-device-traces": (synthetic, "device"), "wide-host-rows": (wide, "host"), "wide-device-traces": (wide, "device")}


@pytest.mark.parametrize("case", list(CASES))
def test_batch_is_the_sequential_proofs(case, seeded):
    make, how = CASES[case]
    inst = make()
    want = inst.sequential(seeded, how)
    got = inst.batch(seeded, how)
    assert len(got) == len(want) == len(inst.rows)
    for m, (a, b) in enumerate(zip(got, want)):
        assert a == b, m
    assert len(set(got)) == len(got)                                   # different inputs: different proofs
    assert len(got[0]) == inst.rec["proof_len"] and hashlib.sha256(got[0]).hexdigest() == inst.rec["proof_sha256"]      # the reference's
    assert inst.all_verify(got) == [True] * len(got)


def test_streams_hold_what_prove_pushes(seeded):
    """fresh streams handed in by the caller hold `prove`'s objects afterwards: serialize() is the proof"""
    inst = rescue()
    streams = [ProofStream() for _ in inst.rows]
    got = inst.batch(seeded, "host", streams)
    assert [s.serialize() for s in streams] == got == inst.sequential(seeded)
    assert len(streams[0].objects) == inst.rec["num_objects"]


@pytest.mark.parametrize("kind", ["plain", "signature"])
def test_streams_that_already_hold_an_object(kind, seeded):
    inst = synthetic()

    def streams():
        made = [ProofStream() if kind == "plain" else SignatureProofStream(b"document %d" % m) for m in range(len(inst.rows))]
        for m, stream in enumerate(made):
            stream.push(b"said before, by member %d" % m)
        return made
    want = inst.sequential(seeded, "device", streams())
    got = inst.batch(seeded, "device", streams())
    assert got == want
    assert got[0] != inst.batch(seeded, "device")[0]                   # the earlier object is part of the transcript


def test_chunks_when_a_forest_takes_two_members(seeded, monkeypatch):
    """FOREST_MAX_LEAVES = the leaves of two members' boundary-quotient codewords: three members go as 2 + 1, the bytes do not move"""
    inst = synthetic()
    want = inst.sequential(seeded)
    inst.batch(seeded)                                                 # (the zerofier's forest exists from here on)
    rounds, R, N = inst.stark.fri.num_rounds(), inst.stark.num_registers, inst.stark.fri_domain_length
    monkeypatch.setattr(sc, "FOREST_MAX_LEAVES", 2 * R * N)
    before = sc.forest_stats()
    got = inst.batch(seeded)
    after = sc.forest_stats()
    assert got == want
    assert after[0] - before[0] == 2 * (2 + rounds)
    assert after[1] - before[1] == 3 * (R + 1 + rounds)


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


def test_forest_and_call_census(seeded, monkeypatch):
    """one served chunk builds 2 + rounds forests (boundary quotients, randomizers, one per FRI round) and the zerofier's once per
    prover; the steps are one library call each for all members"""
    fresh = rescue.__wrapped__(3)                                      # a prover that has no zerofier forest yet
    rounds, R, K = fresh.stark.fri.num_rounds(), fresh.stark.num_registers, 3
    before = sc.forest_stats()
    first = fresh.batch(seeded, "device")
    middle = sc.forest_stats()
    census = Census(sc.lib())
    with monkeypatch.context() as mp:
        mp.setattr(sc, "lib", lambda: census)
        second = fresh.batch(seeded, "device")
    after = sc.forest_stats()
    assert first == second == rescue().sequential(seeded)
    assert (middle[0] - before[0], middle[1] - before[1]) == (2 + rounds + 1, K * R + K + K * rounds + 1)
    assert (after[0] - middle[0], after[1] - middle[1]) == (2 + rounds, K * R + K + K * rounds)
    calls = census.calls
    assert calls.get("sc_randomized_columns_dev", 0) == 2              # the trace matrix, the randomizer polynomials
    assert calls.get("sc_sample_bytes_dev", 0) == calls.get("sc_sample_urandom_dev", 0) == 0
    assert calls.get("sc_geodomain_interpolate_columns_dev", 0) == 1 and calls.get("sc_geodomain_interpolate_dev", 0) == 0
    assert calls.get("sc_coset_divide_columns_later_dev", 0) == 1 and calls.get("sc_coset_divide_later_dev", 0) == 0
    assert calls.get("sc_mpoly_eval_columns_dev", 0) == 1
    assert calls.get("sc_combine_columns_dev", 0) == 2                 # the boundary numerators, the nonlinear combination
    assert calls.get("sc_merkle_forest_query_dev", 0) == 1             # every opening of every member
    assert calls.get("sc_merkle_build_async_dev", 0) == calls.get("sc_merkle_build_dev", 0) == 0      # no tree of a single codeword


def test_device_traces_that_are_rows_of_one_matrix_are_read_in_place(seeded, monkeypatch):
    """RescuePrime.trace_batch_device's layout is used where it lies: against DeviceTraces of separate columns, which are copied into
    one matrix column by column, the batch makes K R device copies less -- and the same proofs"""
    inst = rescue()
    rp, K = RescuePrime(), len(inst.rows)
    rows = rp.N + 1
    inputs = [FieldElement(int(inst.rec["input"]) + 977 * m, field) for m in range(K)]
    whole = rp.trace_batch_device(sc.DeviceVector.from_bytes(sc.pack([x.value for x in inputs])))
    in_place = [DeviceTrace([sc.DeviceVector.wrap(whole.ptr + 16 * rows * (rp.m * k + s), rows, whole) for s in range(rp.m)], field) for k in range(K)]
    copies = {}
    for name, traces in (("in place", in_place), ("separate", inst.traces("device"))):
        census = Census(sc.lib())
        with monkeypatch.context() as mp:
            mp.setattr(sc, "lib", lambda: census)
            got = inst.batch(seeded, rows=traces)
        assert got == inst.sequential(seeded), name
        copies[name] = census.calls.get("sc_memcpy_dev", 0)
    assert copies["separate"] - copies["in place"] == K * rp.m


def test_one_member(seeded):
    inst = rescue()
    seeded(inst.seed)
    got = inst.stark.prove_batch([inst.rows[0]], inst.air, [inst.boundaries[0]], inst.host[0], inst.host[1])
    assert len(got) == 1 and hashlib.sha256(got[0]).hexdigest() == inst.rec["proof_sha256"]


def test_empty_batch_and_mismatched_lengths(seeded):
    inst = rescue()
    before = sc.forest_stats()
    drawn = []
    seeded(inst.seed)
    genuine = os.urandom
    os.urandom = lambda k: drawn.append(k) or genuine(k)             # (restored by the `seeded` fixture's monkeypatch)
    assert inst.stark.prove_batch([], inst.air, [], inst.host[0], inst.host[1]) == []
    assert inst.stark.prove_batch([], inst.air, [], inst.host[0], inst.host[1], []) == []
    for traces, boundaries, streams in ((inst.rows[:2], inst.boundaries, None), (inst.rows, inst.boundaries[:2], None),
                                        (inst.rows, inst.boundaries, [ProofStream()]), ([], [], [ProofStream()])):
        with pytest.raises(AssertionError):
            inst.stark.prove_batch(traces, inst.air, boundaries, inst.host[0], inst.host[1], streams)
    assert drawn == [] and sc.forest_stats() == before                 # before any work


def test_another_boundary_layout_falls_back_to_prove(seeded):
    """member 1 names one pair less (the last cycle stays named: the verifier reads the trace length off it): the batch is not served,
    decided before any draw, and is K calls of `prove`"""
    inst = synthetic()
    boundaries = [inst.boundaries[0], [inst.boundaries[1][0], inst.boundaries[1][2]], inst.boundaries[2]]
    want = inst.sequential(seeded, boundaries=boundaries)
    before = sc.forest_stats()
    got = inst.batch(seeded, boundaries=boundaries)
    assert sc.forest_stats() == before                                 # no forest: every member went through `prove`
    assert got == want
    assert inst.all_verify(got, boundaries) == [True] * 3


def outcome(fn):
    try:
        return ("ok", fn())
    except AssertionError as e:
        return ("raised", str(e))


def test_traces_of_two_lengths_fall_back_to_prove(seeded):
    """a member one row short is no witness; whatever `prove` makes of it, member after member, the batch makes of it too"""
    inst = synthetic()
    rows = [inst.rows[0], inst.rows[1][:-1], inst.rows[2]]
    before = sc.forest_stats()
    together = outcome(lambda: inst.batch(seeded, rows=rows))
    assert sc.forest_stats() == before
    assert together == outcome(lambda: inst.sequential(seeded, rows=rows))


def test_false_witness_raises_what_prove_raises_and_leaves_no_slot_behind(seeded):
    """member 1 of 3 with a bent cell that a boundary condition pins: the boundary division leaves a remainder, and the batch raises the
    reference's assertion (Polynomial.__truediv__) as `prove` does for that member.  A bent cell in the middle of the trace breaks
    transition constraints only: whatever `prove` does with it, the batch does the same.  Every check was read: correct batches run
    afterwards, more of them than a leaked slot per failure would leave room for."""
    inst = rescue()
    one = FieldElement(1, field)

    def bend(cycle, register):
        bent = [list(row) for row in inst.rows[1]]
        bent[cycle][register] = bent[cycle][register] + one
        return [inst.rows[0], bent, inst.rows[2]]
    pinned = bend(0, 1)                                                # (Rescue-Prime pins the capacity at cycle 0 and the output at cycle N)
    alone = outcome(lambda: inst.stark.prove(pinned[1], inst.air, inst.boundaries[1], inst.host[0], inst.host[1]))
    assert alone == ("raised", "cannot perform polynomial division because remainder is not zero")
    for _ in range(3):
        streams = [ProofStream() for _ in range(3)]
        assert outcome(lambda: inst.batch(seeded, rows=pinned, streams=streams)) == alone
        honest = [ProofStream() for _ in range(3)]
        inst.batch(seeded, streams=honest)
        for bad, good in zip(streams, honest):                         # a prefix of what `prove` would have pushed
            assert bad.objects == good.objects[:len(bad.objects)] or bad is streams[1]
    middle = bend(inst.stark.original_trace_length // 2, 0)
    assert outcome(lambda: inst.batch(seeded, rows=middle)) == outcome(lambda: inst.sequential(seeded, rows=middle))
    assert inst.batch(seeded) == inst.sequential(seeded)

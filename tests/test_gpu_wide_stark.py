"""FastStark.prove on WIDE traces (FastStark.COLUMN_BATCH_MIN): the registers go through trace interpolation, the degrees, the
boundary-quotient LDEs and the trace's values on the transition quotients' coset as the rows of one matrix, one library call per
stage.  The proofs must be the reference's byte for byte (tests/golden/fast_stark_wide.json: the 16-register instance of
workloads.synthetic_wide_instance proven by the reference with a seeded os.urandom), on the batch path and on the per-register
one; the existing goldens must not move when the batch path is forced on their two registers; and the library calls are COUNTED,
which is what tells the batch path from a loop."""
import functools
import hashlib
import os
import random

import pytest

from conftest import load_golden
from workload_rescue_prime import RescuePrime

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import fast_stark                                  # noqa: E402
from fast_stark import FastStark, DeviceTrace      # noqa: E402
from algebra import Field, FieldElement            # noqa: E402
import starkcore as sc                              # noqa: E402
import workloads                                    # noqa: E402

LOOP = 10 ** 9                                      # a COLUMN_BATCH_MIN no trace reaches: the per-register code


@pytest.fixture
def seeded(monkeypatch):
    """os.urandom -> the generator the golden runs were drawn with (os is one module: fast_stark.os.urandom is the same attribute)"""
    def seed(value):
        rng = random.Random(value)
        monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    return seed


@functools.lru_cache(maxsize=None)
def wide(log_fri):
    """(record, instance, prover, preprocessing from host lists, preprocessing on the device) of one golden record, made once"""
    rec = [r for r in load_golden("fast_stark_wide.json")["runs"] if r["log_fri"] == log_fri][0]
    instance = workloads.synthetic_wide_instance(log_fri, rec["registers"], rec["num_colinearity_checks"])
    field, T = instance[0], instance[1]
    assert T == rec["original_trace_length"]
    stark = FastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"], rec["registers"], T)
    assert (stark.omicron_domain_length, stark.fri_domain_length) == (rec["omicron_domain_length"], rec["fri_domain_length"])
    host, resident = stark.preprocess(), stark.preprocess(device_resident=True)
    assert host[2].hex() == resident[2].hex() == rec["zerofier_root"]
    return rec, instance, stark, host, resident


@pytest.mark.parametrize("how", ["host rows", "device trace", "per-register loop"])
@pytest.mark.parametrize("log_fri", [10, 12])
def test_wide_golden_proofs(log_fri, how, seeded, monkeypatch):
    rec, (field, T, rows, packed, air, boundary), stark, host, resident = wide(log_fri)
    assert FastStark.COLUMN_BATCH_MIN == 4 <= rec["registers"]
    if how == "per-register loop":
        monkeypatch.setattr(FastStark, "COLUMN_BATCH_MIN", LOOP)
    seeded(rec["urandom_seed"])
    if how == "device trace":
        proof = stark.prove(DeviceTrace.from_packed(packed, field), air, boundary, resident[0], resident[1])
    else:
        proof = stark.prove(rows, air, boundary, host[0], host[1])
    assert len(proof) == rec["proof_len"]
    assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]                # byte-identical to the reference
    assert stark.verify(proof, air, boundary, host[2]) is True


def test_rescue_prime_goldens_on_the_batch_path(seeded, monkeypatch):
    """the Rescue-Prime proofs of tests/golden/fast_stark.json (two registers) with the batch path forced"""
    monkeypatch.setattr(FastStark, "COLUMN_BATCH_MIN", 2)
    field, rp = Field.main(), RescuePrime()
    for rec in load_golden("fast_stark.json")["runs"]:
        seeded(rec["urandom_seed"])
        input_element = FieldElement(int(rec["input"]), field)
        output_element = rp.hash(input_element)
        stark = FastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"], rp.m, rp.N + 1)
        tz, tz_codeword, tz_root = stark.preprocess()
        assert tz_root.hex() == rec["zerofier_root"]
        air, boundary = rp.transition_constraints(stark.omicron), rp.boundary_constraints(output_element)
        proof = stark.prove(rp.trace(input_element), air, boundary, tz, tz_codeword)
        assert len(proof) == rec["proof_len"] and hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]
        assert stark.verify(proof, air, boundary, tz_root) is True


@pytest.mark.parametrize("log_fri", [10, 12])
def test_synthetic_goldens_on_the_batch_path(log_fri, seeded, monkeypatch):
    """the two-register workload bench.py times (tests/golden/fast_stark_synth.json) with the batch path forced, from host rows and
    from device-resident columns"""
    import synth
    monkeypatch.setattr(FastStark, "COLUMN_BATCH_MIN", 2)
    records = [r for r in load_golden("fast_stark_synth.json")["runs"] if r["log_fri"] == log_fri]
    assert records
    for rec in records:
        s = rec["num_colinearity_checks"]
        field, T, packed, air, boundary = workloads.synthetic_stark_instance(log_fri, s)
        stark = FastStark(field, rec["expansion_factor"], s, rec["security_level"], 2, T)
        for device_resident in (False, True):
            seeded(rec["urandom_seed"])
            tz, tz_codeword, tz_root = stark.preprocess(device_resident=True) if device_resident else stark.preprocess()
            if device_resident:
                trace = DeviceTrace.from_packed(packed, field)
            else:
                trace = [[FieldElement(a, field), FieldElement(b, field)] for a, b in zip(*synth.synthetic_air_columns(T))]
            proof = stark.prove(trace, air, boundary, tz, tz_codeword)
            assert len(proof) == rec["proof_len"], device_resident
            assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"], device_resident
        assert stark.verify(proof, air, boundary, tz_root) is True


def test_rpsss_signature_on_the_batch_path(seeded, monkeypatch):
    """the reference's signature (tests/golden/rpsss.json) with the batch path forced on the two-register Rescue-Prime trace"""
    from fast_rpsss import FastRPSSS
    monkeypatch.setattr(FastStark, "COLUMN_BATCH_MIN", 2)
    g = load_golden("rpsss.json")
    rpsss = FastRPSSS()
    seeded(g["seed"])
    pairs = [rpsss.keygen() for _ in range(len(g["keys"]))]
    signature = rpsss.sign(pairs[g["signed_key"]][0], g["document"].encode())
    assert len(signature) == g["signature_len"] and hashlib.sha256(signature).hexdigest() == g["signature_sha256"]


class Census:
    """the bound library with every call counted by name, and the vectors sc_vec_degree_dev was asked about"""

    def __init__(self, lib):
        self.lib, self.calls, self.degree_asked_of = lib, {}, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("sc_"):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            if name == "sc_vec_degree_dev":
                self.degree_asked_of.append(int(getattr(args[0], "value", args[0]) or 0))
            return fn(*args)
        return counted


@pytest.mark.parametrize("batch_min", [4, LOOP])
def test_call_census(batch_min, seeded, monkeypatch):
    """16 registers at FRI 2^10: on the batch path ONE interpolation call, no degree asked of a trace polynomial, at most three
    column evaluations (boundary-quotient LDEs, trace(X), trace(omicron X)) and no coset evaluation per register; the loop makes
    16 interpolation calls"""
    rec, (field, T, rows, packed, air, boundary), stark, host, resident = wide(10)
    w = rec["registers"]
    monkeypatch.setattr(FastStark, "COLUMN_BATCH_MIN", batch_min)
    seeded(rec["urandom_seed"])
    trace = DeviceTrace.from_packed(packed, field)
    census = Census(sc.lib())
    trace_polynomials = []
    real = fast_stark.DevicePolynomial.from_codeword

    def noted(codeword):
        polynomial = real(codeword)
        trace_polynomials.append((polynomial.vec.ptr, polynomial.vec.n))
        return polynomial
    monkeypatch.setattr(sc, "lib", lambda: census)
    monkeypatch.setattr(fast_stark.DevicePolynomial, "from_codeword", staticmethod(noted))
    proof = stark.prove(trace, air, boundary, resident[0], resident[1])
    monkeypatch.undo()
    assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]
    calls = census.calls
    if batch_min == LOOP:
        assert calls.get("sc_geodomain_interpolate_dev", 0) == w and "sc_geodomain_interpolate_columns_dev" not in calls
        return
    assert calls.get("sc_geodomain_interpolate_dev", 0) == 0
    assert calls.get("sc_geodomain_interpolate_columns_dev", 0) == 1
    assert len(trace_polynomials) == w
    inside = lambda p: any(start <= p < start + 16 * n for start, n in trace_polynomials)
    assert not any(inside(p) for p in census.degree_asked_of)
    assert calls.get("sc_vec_degree_columns_dev", 0) == 1
    assert calls.get("sc_coset_evaluate_columns_dev", 0) <= 3
    # what is left is not per register: X (if a constraint uses it), the transition zerofier, the randomizer, the combination
    assert calls.get("sc_coset_evaluate_dev", 0) <= 4 < w


def test_false_witness_raises_the_same_on_both_paths(seeded, monkeypatch):
    """16 registers.  A perturbed trace cell that a boundary condition pins, and a perturbed boundary value, leave a remainder in
    that register's boundary division: both paths raise the reference's assertion (Polynomial.__truediv__), word for word.  A
    perturbed cell in the middle of the trace breaks two transition constraints only; whatever the per-register code does with
    it -- an assertion, or a proof that does not verify -- the batch path does the same, byte for byte."""
    rec, (field, T, rows, packed, air, boundary), stark, host, resident = wide(10)
    one = FieldElement(1, field)

    def bend(cycle, register):
        bent = [list(row) for row in rows]
        bent[cycle][register] = bent[cycle][register] + one
        return bent
    wrong = list(boundary)
    wrong[3] = (wrong[3][0], wrong[3][1], wrong[3][2] + one)

    def outcomes(trace, conditions):
        seen = []
        for batch_min in (4, LOOP):
            monkeypatch.setattr(FastStark, "COLUMN_BATCH_MIN", batch_min)
            for device_resident in (False, True):
                seeded(rec["urandom_seed"])
                try:
                    if device_resident:
                        proof = stark.prove(DeviceTrace.from_rows(trace, field), air, conditions, resident[0], resident[1])
                    else:
                        proof = stark.prove(trace, air, conditions, host[0], host[1])
                    seen.append(("proof", hashlib.sha256(proof).hexdigest(), stark.verify(proof, air, conditions, host[2])))
                except AssertionError as raised:
                    seen.append(("raised", str(raised)))
        assert len(set(seen)) == 1, seen
        return seen[0]
    for trace, conditions in ((bend(0, 5), boundary), (bend(T - 1, 0), boundary), (rows, wrong)):
        assert outcomes(trace, conditions) == ("raised", "cannot perform polynomial division because remainder is not zero")
    middle = outcomes(bend(T // 2, 5), boundary)
    assert middle[0] == "raised" or middle[2] is False

"""FastStark.prove on wide traces with the two further column steps of the batch path (FastStark.COLUMN_DIVIDE: the boundary quotients
of all registers as one combination and one columns-form coset division with ONE pending verdict; FastStark.COLUMN_COMBINE: the
nonlinear combination as one pass): the proofs are the reference's byte for byte with the switches in every setting, the library
calls are counted, a false boundary raises the per-register loop's message, and a prover that finds no pinned slot free still
produces the golden proof."""
import ctypes
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

SETTINGS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.fixture
def seeded(monkeypatch):
    """os.urandom -> the generator the golden runs were drawn with"""
    def seed(value):
        rng = random.Random(value)
        monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    return seed


@pytest.fixture
def switches(monkeypatch):
    def switch(divide, combine):
        monkeypatch.setattr(FastStark, "COLUMN_DIVIDE", divide)
        monkeypatch.setattr(FastStark, "COLUMN_COMBINE", combine)
    return switch


@functools.lru_cache(maxsize=None)
def wide(log_fri):
    """(record, instance, prover, preprocessing from host lists, preprocessing on the device) of one golden record, made once"""
    rec = [r for r in load_golden("fast_stark_wide.json")["runs"] if r["log_fri"] == log_fri][0]
    instance = workloads.synthetic_wide_instance(log_fri, rec["registers"], rec["num_colinearity_checks"])
    field, T = instance[0], instance[1]
    stark = FastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"], rec["registers"], T)
    host, resident = stark.preprocess(), stark.preprocess(device_resident=True)
    assert host[2].hex() == resident[2].hex() == rec["zerofier_root"]
    return rec, instance, stark, host, resident


@pytest.mark.parametrize("divide,combine", SETTINGS)
@pytest.mark.parametrize("how", ["host rows", "device trace"])
@pytest.mark.parametrize("log_fri", [10, 12])
def test_wide_golden_proofs_with_the_switches(log_fri, how, divide, combine, seeded, switches):
    rec, (field, T, rows, packed, air, boundary), stark, host, resident = wide(log_fri)
    assert FastStark.COLUMN_BATCH_MIN <= rec["registers"]
    switches(divide, combine)
    seeded(rec["urandom_seed"])
    if how == "device trace":
        proof = stark.prove(DeviceTrace.from_packed(packed, field), air, boundary, resident[0], resident[1])
    else:
        proof = stark.prove(rows, air, boundary, host[0], host[1])
    assert len(proof) == rec["proof_len"]
    assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]                # byte-identical to the reference


def test_rescue_prime_goldens_with_both_switches(seeded, switches, monkeypatch):
    """the Rescue-Prime proofs of tests/golden/fast_stark.json (two registers, boundary zerofiers of different degrees) with the batch
    path forced and both switches on"""
    monkeypatch.setattr(FastStark, "COLUMN_BATCH_MIN", 2)
    switches(True, True)
    field, rp = Field.main(), RescuePrime()
    for rec in load_golden("fast_stark.json")["runs"]:
        seeded(rec["urandom_seed"])
        input_element = FieldElement(int(rec["input"]), field)
        output_element = rp.hash(input_element)
        stark = FastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"], rp.m, rp.N + 1)
        tz, tz_codeword, tz_root = stark.preprocess()
        air, boundary = rp.transition_constraints(stark.omicron), rp.boundary_constraints(output_element)
        proof = stark.prove(rp.trace(input_element), air, boundary, tz, tz_codeword)
        assert len(proof) == rec["proof_len"] and hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]
        assert stark.verify(proof, air, boundary, tz_root) is True


@pytest.mark.parametrize("log_fri", [10, 12])
def test_synthetic_goldens_with_both_switches(log_fri, seeded, switches, monkeypatch):
    """the two-register workload of tests/golden/fast_stark_synth.json with the batch path forced and both switches on"""
    import synth
    monkeypatch.setattr(FastStark, "COLUMN_BATCH_MIN", 2)
    switches(True, True)
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


def test_call_census_with_both_switches(seeded, switches, monkeypatch):
    """16 registers at FRI 2^10: no division and no axpy per register or per term -- ONE columns-form division, and two combinations
    (the boundary numerators, the nonlinear combination)"""
    rec, (field, T, rows, packed, air, boundary), stark, host, resident = wide(10)
    switches(True, True)
    seeded(rec["urandom_seed"])
    trace = DeviceTrace.from_packed(packed, field)
    census = Census(sc.lib())
    monkeypatch.setattr(sc, "lib", lambda: census)
    proof = stark.prove(trace, air, boundary, resident[0], resident[1])
    monkeypatch.undo()
    assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]
    calls = census.calls
    assert calls.get("sc_coset_divide_later_dev", 0) == 0
    assert calls.get("sc_coset_divide_columns_later_dev", 0) == 1
    assert calls.get("sc_axpy_shift_dev", 0) == 0
    assert calls.get("sc_combine_columns_dev", 0) == 2


def test_false_boundary_raises_the_same_with_the_switches(seeded, switches):
    """a perturbed boundary value leaves a remainder in that register's boundary division: the one verdict of the columns-form
    division raises the per-register loop's assertion, word for word, from host rows and from a device trace"""
    rec, (field, T, rows, packed, air, boundary), stark, host, resident = wide(10)
    one = FieldElement(1, field)
    wrong = list(boundary)
    wrong[3] = (wrong[3][0], wrong[3][1], wrong[3][2] + one)
    seen = []
    for divide, combine in ((False, False), (True, True)):
        switches(divide, combine)
        for device_resident in (False, True):
            seeded(rec["urandom_seed"])
            with pytest.raises(AssertionError) as raised:
                if device_resident:
                    stark.prove(DeviceTrace.from_rows(rows, field), air, wrong, resident[0], resident[1])
                else:
                    stark.prove(rows, air, wrong, host[0], host[1])
            seen.append(str(raised.value))
    assert set(seen) == {"cannot perform polynomial division because remainder is not zero"}, seen


class Drained:
    """Every pinned slot taken, by 1-element out-of-place deferred divisions, until sc_pointwise_div_later_dev says
    SC_ERR_UNSUPPORTED.  Does not assume the pool's size: other live objects may hold slots.  `release()` waits for all."""

    def __init__(self):
        self.a, self.b, self.out = sc.DeviceVector.from_ints([6]), sc.DeviceVector.from_ints([3]), sc.DeviceVector(1)
        self.handles = []
        lib = sc.lib()
        while True:
            h = ctypes.c_void_p()
            rc = lib.sc_pointwise_div_later_dev(self.a.ptr, self.b.ptr, self.out.ptr, 1, ctypes.byref(h), None)
            if rc == sc.SC_ERR_UNSUPPORTED:
                break
            sc._check(rc)
            self.handles.append(sc.Later(h))
            assert len(self.handles) <= 1 << 16, "the slot pool never ran out"

    def release(self):
        for h in self.handles:
            assert h.wait() == (False, False)
        self.handles = []


def test_a_prove_without_a_free_slot_is_still_the_golden_proof(seeded, switches):
    rec, (field, T, rows, packed, air, boundary), stark, host, resident = wide(10)
    switches(True, True)
    seeded(rec["urandom_seed"])
    drained = Drained()
    try:
        assert len(drained.handles) > 0
        proof = stark.prove(DeviceTrace.from_packed(packed, field), air, boundary, resident[0], resident[1])
    finally:
        drained.release()
    assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]

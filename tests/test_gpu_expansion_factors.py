"""Proofs at expansion factors other than 4 on the GPU, byte for byte against the reference's own (tests/golden/expansion.json, made by
tests/golden/make_golden.py --expansion; instances: tests/expansion_cases.py).  Every other test of the suite runs at expansion
factor 4, so a 4 baked into the companion openings at index + ef, into the successor row of verify_batch's combination check, into
the shape of the FRI commit phase (the expansion factor, not 4 s, ends the folding: the last codeword is 2 ef long, degree bound 1),
into the last codeword's degree bound or into the FRI-to-trace domain ratio would pass there and fails here.

Fri: the three forms of Fri.prove with the persistent tail kernel on and off, from device codewords and lists; verify and
verify_batch on an honest codeword and on one of N / ef + 1 coefficients; prove_batch.  A last codeword of 8192 elements, beyond
the 4096 that travel through the tail kernel's pinned block.  FastStark: both data flows, host rows and device traces, both forms
of the preprocessing; verify and verify_batch on the proof, a false boundary claim and altered proofs; prove_batch; the sharded
prover at one rank.  N = 64 lies below the 256 leaves of the fused fold (the fold is its own launch there): only the bytes show it."""
import functools
import hashlib
import os
import pickle
import random
from types import SimpleNamespace

import pytest

from conftest import load_golden
from workload_rescue_prime import RescuePrime
import expansion_cases
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import starkcore as sc                              # noqa: E402
import fri as fri_module                            # noqa: E402
from algebra import Field, FieldElement             # noqa: E402
from fast_rpsss import SignatureProofStream         # noqa: E402
from fast_stark import DeviceTrace, FastStark       # noqa: E402
from fri import Fri                                 # noqa: E402
from ip import ProofStream                          # noqa: E402
from ntt import fast_coset_evaluate_device          # noqa: E402
from starkcore import DeviceCodeword, DeviceVector  # noqa: E402
from univariate import Polynomial                   # noqa: E402

field = Field.main()
G = load_golden("expansion.json")
FRI = G["fri"]
STARK = G["stark"]
TAIL_LAST_MAX = 4096                                # csrc/fri_tail.cuh


def fri_id(rec):
    return "2^%d-ef%d-s%d-%s" % (rec["logN"], rec["expansion_factor"], rec["num_colinearity_tests"], "honest" if rec["honest"] else "one-more")


def stark_id(rec):
    return "%s-2^%d-ef%d-s%d" % (rec["kind"], rec["fri_domain_length"].bit_length() - 1, rec["expansion_factor"], rec["num_colinearity_checks"])


def fri_of(rec):
    N = 1 << rec["logN"]
    fr = Fri(field.generator(), field.primitive_nth_root(N), N, rec["expansion_factor"], rec["num_colinearity_tests"])
    assert fr.num_rounds() == rec["num_rounds"]
    return fr


def codeword(seed, count, N):
    """the coset evaluation of `count` seeded coefficients, in HBM"""
    coeffs = [FieldElement(v, field) for v in synth.synth_ints(seed, count)]
    return fast_coset_evaluate_device(Polynomial(coeffs), field.generator(), field.primitive_nth_root(N), N)


@functools.lru_cache(maxsize=None)
def codeword_bytes(index):
    rec = FRI[index]
    raw = codeword(rec["coeff_seed"], rec["num_coeffs"], 1 << rec["logN"]).vec.to_bytes()
    assert hashlib.sha256(raw).hexdigest() == rec["codeword_sha256"]
    return raw


def fresh(index):
    """the record's codeword in a vector of its own: no tree, no cached objects"""
    return DeviceCodeword(DeviceVector.from_bytes(codeword_bytes(index)), field)


def is_recorded(rec, top, stream):
    ser = stream.serialize()
    assert top == rec["top_level_indices"]
    assert [o.hex() for o in stream.objects[:rec["num_rounds"]]] == rec["roots"]
    assert (len(stream.objects), len(ser)) == (rec["num_objects"], rec["serialized_len"])
    assert hashlib.sha256(ser).hexdigest() == rec["serialized_sha256"]
    return ser


@functools.lru_cache(maxsize=None)
def proof_of(index):
    stream = ProofStream()
    fri_of(FRI[index]).prove(fresh(index), stream)
    return stream.serialize()


def host_verdict(fn, *args):
    try:
        return fn(*args) == True          # noqa: E712
    except Exception:
        return False


# ---- Fri -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("index", range(len(FRI)), ids=[fri_id(r) for r in FRI])
def test_fri_prove_in_every_form_is_the_references_proof(index, monkeypatch):
    """one library call, commit in the library with the query phase in Python, the Python round loop -- forced as
    tests/test_gpu_host.py forces them -- each with the tail kernel on and off, from a device codeword and (up to 2^10) a list"""
    rec, fr = FRI[index], fri_of(FRI[index])
    N, s = 1 << rec["logN"], rec["num_colinearity_tests"]
    assert rec["last_codeword_len"] == N >> (fr.num_rounds() - 1)
    one_calls, commits = [], []
    real_one, real_commit = Fri._prove_in_library, Fri._commit_in_library
    serialized = set()
    for form in ("one call", "commit in library", "python"):
        for tail in (1, 0):
            for as_list in ([False, True] if rec["logN"] <= 10 else [False]):
                source = fresh(index)
                if as_list:
                    source = source.tolist()
                stream = ProofStream()
                sc.set_tuning("fri_tail", tail)
                try:
                    with monkeypatch.context() as m:
                        if form == "one call":
                            m.setattr(Fri, "_prove_in_library", lambda self, *a: (lambda out: (one_calls.append(out is not None), out)[1])(real_one(self, *a)))
                        else:
                            m.setattr(Fri, "_prove_in_library", lambda self, *a: None)
                        if form == "python":
                            m.setattr(Fri, "_commit_in_library", lambda self, cw, ps, rounds: self._commit_rounds(cw, ps, rounds))
                        else:
                            m.setattr(Fri, "_commit_in_library", lambda self, *a: (lambda out: (commits.append(out is not None), out)[1])(real_commit(self, *a)))
                        top = fr.prove(source, stream)
                finally:
                    sc.set_tuning("fri_tail", 1)
                serialized.add(is_recorded(rec, top, stream))
    assert len(serialized) == 1
    # the one-call prover serves device codewords of every recorded shape: at least two rounds and s <= the last codeword's length
    assert fr.num_rounds() >= 2 and s <= rec["last_codeword_len"]
    lists = 1 if rec["logN"] <= 10 else 0
    assert one_calls == ([True] + [False] * lists) * 2
    assert commits == [True] * ((2 + 2 * lists) + 2 * lists)      # the second form always, the first form's lists (no one call for a list)


@pytest.mark.parametrize("index", range(len(FRI)), ids=[fri_id(r) for r in FRI])
def test_fri_verify_and_verify_batch_give_the_references_verdict(index):
    rec, fr = FRI[index], fri_of(FRI[index])
    want = rec["verifies"]
    if want is None:
        # (the reference's verifier interpolates the 8192-element last codeword by Lagrange's formula: no verdict recorded; the
        # honest proof must verify, the other one has a polynomial of degree N / ef: one too many)
        want = rec["honest"]
    proof = proof_of(index)
    values, batch_values = [], []
    assert fr.verify(ProofStream().deserialize(proof), values) is want
    assert fr.verify_batch([ProofStream().deserialize(proof)], [batch_values]) == [want]
    if want:
        assert values == batch_values and len(values) == 2 * rec["num_colinearity_tests"]


def test_fri_verify_batch_on_a_mixed_batch_agrees_proof_by_proof():
    """both proofs of one shape and the honest proofs of two more, in one batch: every member is verified with the Fri of the
    first shape's expansion factor only where it is that shape -- so the batch is per shape, and within it proof by proof"""
    by_shape = {}
    for index, rec in enumerate(FRI):
        by_shape.setdefault((rec["logN"], rec["expansion_factor"], rec["num_colinearity_tests"]), {})[rec["honest"]] = index
    shape = (10, 8, 5)
    fr = fri_of(FRI[by_shape[shape][True]])
    others = [codeword(7000 + k, (1 << 10) // 8, 1 << 10) for k in range(2)]
    proofs = [proof_of(by_shape[shape][True]), proof_of(by_shape[shape][False])]
    for cw in others:
        stream = ProofStream()
        fr.prove(cw, stream)
        proofs.append(stream.serialize())
    # a proof of another shape read with this one's parameters: the host verifier's verdict, whatever it is
    proofs.append(proof_of(by_shape[(10, 16, 2)][True]))
    proofs.append(proof_of(by_shape[(8, 2, 3)][True]))
    want = [host_verdict(fr.verify, ProofStream().deserialize(p), []) for p in proofs]
    assert want[:4] == [True, False, True, True] and not any(want[4:])
    assert fr.verify_batch([ProofStream().deserialize(p) for p in proofs], [[] for _ in proofs]) == want
    # ... and each shape's own verifier on its own honest proof, in one go per shape
    for other in ((10, 16, 2), (8, 2, 3)):
        index = by_shape[other][True]
        assert fri_of(FRI[index]).verify_batch([ProofStream().deserialize(proof_of(index)) for _ in range(2)], [[], []]) == [True, True]


@pytest.fixture
def row_counts(monkeypatch):
    """rows each device entry received, UNDECIDED colinearity verdicts, and calls of the host functions rows fall back to
    (tests/test_gpu_verify_batch.py)"""
    counts = {"merkle": 0, "colinearity": 0, "undecided": 0, "host_merkle": 0, "host_colinearity": 0}
    merkle_batch, colinearity_batch = sc.merkle_verify_batch, sc.colinearity_batch
    host_merkle, host_colinearity = fri_module.Merkle.verify, fri_module.test_colinearity

    def spy_merkle(rows, *a):
        counts["merkle"] += len(rows)
        return merkle_batch(rows, *a)

    def spy_colinearity(rows, *a):
        counts["colinearity"] += len(rows)
        out = colinearity_batch(rows, *a)
        counts["undecided"] += int((out == sc.UNDECIDED).sum())
        return out

    def spy_host_merkle(*a):
        counts["host_merkle"] += 1
        return host_merkle(*a)

    def spy_host_colinearity(*a):
        counts["host_colinearity"] += 1
        return host_colinearity(*a)

    monkeypatch.setattr(sc, "merkle_verify_batch", spy_merkle)
    monkeypatch.setattr(sc, "colinearity_batch", spy_colinearity)
    monkeypatch.setattr(fri_module.Merkle, "verify", staticmethod(spy_host_merkle))
    monkeypatch.setattr(fri_module, "test_colinearity", spy_host_colinearity)
    return counts


def test_honest_fri_proofs_check_every_row_on_the_device(row_counts):
    index = [i for i, r in enumerate(FRI) if (r["logN"], r["expansion_factor"], r["honest"]) == (11, 32, True)][0]
    rec, fr = FRI[index], fri_of(FRI[index])
    s, rounds = rec["num_colinearity_tests"], rec["num_rounds"]
    proofs = [proof_of(index)]
    for seed in range(2):
        stream = ProofStream()
        fr.prove(codeword(7100 + seed, rec["num_coeffs"], 1 << rec["logN"]), stream)
        proofs.append(stream.serialize())
    assert fr.verify_batch([ProofStream().deserialize(p) for p in proofs], [[] for _ in proofs]) == [True] * 3
    assert row_counts["merkle"] == 3 * 3 * s * (rounds - 1)
    assert row_counts["colinearity"] == 3 * s * (rounds - 1)
    assert row_counts["undecided"] == row_counts["host_merkle"] == row_counts["host_colinearity"] == 0


HONEST = [i for i, r in enumerate(FRI) if r["honest"]]


@pytest.mark.parametrize("kind", ["plain", "signature"])
@pytest.mark.parametrize("index", HONEST, ids=[fri_id(FRI[i]) for i in HONEST])
def test_fri_prove_batch_members_are_the_single_proofs_and_member_0_the_references(index, kind):
    rec, fr = FRI[index], fri_of(FRI[index])
    N = 1 << rec["logN"]
    raws = [codeword_bytes(index)] + [codeword(rec["coeff_seed"] + 10 * k, rec["num_coeffs"], N).vec.to_bytes() for k in range(1, 5)]
    assert len(set(raws)) == 5
    make = (lambda m: ProofStream()) if kind == "plain" else (lambda m: SignatureProofStream(b"document %d" % m))
    singles = []
    for m, raw in enumerate(raws):
        stream = make(m)
        singles.append((fr.prove(DeviceCodeword(DeviceVector.from_bytes(raw), field), stream), stream.serialize()))
    if kind == "plain":
        assert hashlib.sha256(singles[0][1]).hexdigest() == rec["serialized_sha256"]
    for K in (1, 2, 5):
        before = sc.forest_stats()
        streams = [make(m) for m in range(K)]
        tops = fr.prove_batch([DeviceCodeword(DeviceVector.from_bytes(raw), field) for raw in raws[:K]], streams)
        after = sc.forest_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (fr.num_rounds(), K * fr.num_rounds())      # one forest of K trees per round
        assert [(top, stream.serialize()) for top, stream in zip(tops, streams)] == singles[:K]
        if kind == "plain":
            is_recorded(rec, tops[0], streams[0])
            assert fr.verify_batch(streams, [[] for _ in streams]) == [True] * K


def test_a_last_codeword_longer_than_the_tail_kernels_pinned_block():
    """N = 2^15, ef = 2^12, s = 2: three rounds, a last codeword of 8192 elements (csrc/fri_tail.cuh: TAIL_LAST_MAX = 4096 go
    through the pinned block).  The bytes are the reference's (test_fri_prove_in_every_form_...); here, as
    tests/test_gpu_host.py does for the tail kernel: the first two roots against the oracle's commitment to its own coset
    evaluation and to its own first fold."""
    from oracle import py_oracle as po
    index = [i for i, r in enumerate(FRI) if r["last_codeword_len"] > TAIL_LAST_MAX and r["honest"]][0]
    rec = FRI[index]
    N, ef, s = 1 << rec["logN"], rec["expansion_factor"], rec["num_colinearity_tests"]
    assert (N, ef, s) == (1 << 15, 1 << 12, 2)
    fr = Fri(field.generator(), field.primitive_nth_root(N), N, ef, s)           # the host class first
    assert fr.num_rounds() == 3 and N >> (fr.num_rounds() - 1) == 8192 > TAIL_LAST_MAX
    proofs = []
    for tail in (1, 0):
        sc.set_tuning("fri_tail", tail)
        try:
            stream = ProofStream()
            top = fr.prove(fresh(index), stream)
            proofs.append((top, stream.serialize()))
        finally:
            sc.set_tuning("fri_tail", 1)
    assert proofs[0] == proofs[1]
    assert hashlib.sha256(proofs[0][1]).hexdigest() == rec["serialized_sha256"]
    assert fr.verify(ProofStream().deserialize(proofs[0][1]), []) is True
    objects = ProofStream().deserialize(proofs[0][1]).objects
    assert len(objects[fr.num_rounds()]) == 8192
    coeffs = synth.synth_packed(rec["coeff_seed"], rec["num_coeffs"]).tobytes()
    om = field.primitive_nth_root(N)
    cw0 = po.C.coset_evaluate(coeffs, rec["num_coeffs"], po.GENERATOR, om.value, N)
    assert objects[0] == po.C.merkle_commit(cw0, N)
    stream = ProofStream()
    stream.push(objects[0])
    alpha = field.sample(stream.prover_fiat_shamir())
    cw1 = po.C.fold(cw0, N, alpha.value, po.GENERATOR, om.value)
    assert objects[1] == po.C.merkle_commit(cw1, N // 2)


# ---- FastStark -------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def seeded(monkeypatch):
    """os.urandom -> the generator the golden runs were drawn with"""
    def seed(value):
        rng = random.Random(value)
        monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    return seed


def rows_and_constraints(rec, make_stark):
    ef, s = rec["expansion_factor"], rec["num_colinearity_checks"]
    if rec["kind"] == "rescue_prime":
        rp = RescuePrime()
        input_element = FieldElement(int(rec["input"]), field)
        output_element = rp.hash(input_element)
        assert str(output_element.value) == rec["output"]
        stark = make_stark(rp.m, rp.N + 1)
        return stark, None, rp.trace(input_element), rp.transition_constraints(stark.omicron), rp.boundary_constraints(output_element)
    if rec["kind"] == "synthetic":
        _, T, packed, rows, air, boundary = expansion_cases.synthetic_instance(rec["log_fri"], ef, s)
    else:
        _, T, packed, rows, air, boundary = expansion_cases.wide_instance(rec["log_fri"], rec["registers"], ef, s)
    assert T == rec["original_trace_length"]
    return make_stark(rec["registers"], T), packed, rows, air, boundary


@functools.lru_cache(maxsize=None)
def instance(index):
    rec = STARK[index]
    make = lambda registers, cycles: FastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"], registers, cycles)
    stark, packed, rows, air, boundary = rows_and_constraints(rec, make)
    assert (stark.omicron_domain_length, stark.fri_domain_length) == (rec["omicron_domain_length"], rec["fri_domain_length"])
    assert stark.fri.expansion_factor == rec["expansion_factor"] and stark.num_registers == rec["registers"]
    host, resident = stark.preprocess(), stark.preprocess(device_resident=True)
    assert host[2].hex() == resident[2].hex() == rec["zerofier_root"]
    return SimpleNamespace(rec=rec, stark=stark, packed=packed, rows=rows, air=air, boundary=boundary, host=host, resident=resident, root=host[2])


def device_trace(inst):
    return DeviceTrace.from_packed(inst.packed, field) if inst.packed is not None else DeviceTrace.from_rows(inst.rows, field)


def is_recorded_proof(rec, proof):
    objects = pickle.loads(proof)
    assert [o.hex() for o in objects[:rec["registers"] + 1]] == rec.get("first_roots", [o.hex() for o in objects[:rec["registers"] + 1]])
    assert (len(objects), len(proof)) == (rec["num_objects"], rec["proof_len"])
    assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]                # byte-identical to the reference


@functools.lru_cache(maxsize=None)
def golden_proof(index):
    """the record's proof as this package makes it (checked against the record by the tests that call this)"""
    inst = instance(index)
    rng = random.Random(inst.rec["urandom_seed"])
    genuine = os.urandom
    os.urandom = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
    try:
        proof = inst.stark.prove(device_trace(inst), inst.air, inst.boundary, inst.resident[0], inst.resident[1])
    finally:
        os.urandom = genuine
    is_recorded_proof(inst.rec, proof)
    return proof


@pytest.mark.parametrize("device_min", [32, 10 ** 9])
@pytest.mark.parametrize("index", range(len(STARK)), ids=[stark_id(r) for r in STARK])
def test_stark_prove_is_the_references_proof(index, device_min, seeded, monkeypatch):
    """DEVICE_MIN = 32: every polynomial in HBM; 10^9: the reference's host-list data flow (up to a FRI domain of 2^12) -- from host
    rows and from a DeviceTrace, with the preprocessing from host lists and device-resident"""
    rec = STARK[index]
    if device_min > 32 and rec["fri_domain_length"] > 1 << 12:
        return                                             # (the host-list data flow at 2^14: seconds of Python lists, nothing new)
    monkeypatch.setattr(FastStark, "DEVICE_MIN", device_min)
    instance.cache_clear()                                 # (preprocess() reads DEVICE_MIN)
    try:
        inst = instance(index)
        for trace_on_device in (False, True):
            for pre in (inst.host, inst.resident):
                seeded(rec["urandom_seed"])
                trace = device_trace(inst) if trace_on_device else list(inst.rows)
                proof = inst.stark.prove(trace, inst.air, inst.boundary, pre[0], pre[1])
                is_recorded_proof(rec, proof)
    finally:
        instance.cache_clear()


@pytest.mark.parametrize("divide,combine", [(True, True), (False, False), (True, False), (False, True)])
def test_wide_trace_with_the_column_steps_on_and_off(divide, combine, seeded, monkeypatch):
    index = [i for i, r in enumerate(STARK) if r["kind"] == "wide"][0]
    rec = STARK[index]
    assert rec["registers"] >= FastStark.COLUMN_BATCH_MIN and rec["expansion_factor"] == 8
    monkeypatch.setattr(FastStark, "COLUMN_DIVIDE", divide)
    monkeypatch.setattr(FastStark, "COLUMN_COMBINE", combine)
    inst = instance(index)
    for trace_on_device in (False, True):
        seeded(rec["urandom_seed"])
        pre = inst.resident if trace_on_device else inst.host
        proof = inst.stark.prove(device_trace(inst) if trace_on_device else list(inst.rows), inst.air, inst.boundary, pre[0], pre[1])
        is_recorded_proof(rec, proof)


@pytest.mark.parametrize("index", range(len(STARK)), ids=[stark_id(r) for r in STARK])
def test_stark_verify_and_verify_batch_give_the_references_verdicts(index):
    """the proof, the false boundary claim and every recorded alteration, re-applied to the proof made here: `verify` one by one,
    `verify_batch` all of them in one batch with the combination check on the GPU (the default)"""
    inst = instance(index)
    rec, stark = inst.rec, inst.stark
    assert FastStark.COMBINATION_ON_DEVICE is True
    proof = golden_proof(index)
    objects = pickle.loads(proof)
    N, ef = stark.fri_domain_length, rec["expansion_factor"]
    places = expansion_cases.alteration_places(len(objects), rec["registers"], ef, N, rec["top_level_indices"])
    assert [{k: v for k, v in a.items() if k != "verifies"} for a in rec["alterations"]] == places
    assert any(a["position"] == (a["companion_of"] + ef) % N and a["how"] == "add one" for a in places if "companion_of" in a)
    wrong = expansion_cases.false_claim(inst.boundary, field.one())
    cases = [(proof, inst.boundary, rec["verifies"]), (proof, wrong, rec["false_claim_verifies"])]
    for place in rec["alterations"]:
        cases.append((pickle.dumps(expansion_cases.altered(objects, place, field.one())), inst.boundary, place["verifies"]))
    want = [w for _, _, w in cases]
    assert want[:2] == [True, False] and len(want) >= 6
    assert [host_verdict(stark.verify, p, inst.air, b, inst.root) for p, b, _ in cases] == want
    assert stark.verify_batch([p for p, _, _ in cases], inst.air, [b for _, b, _ in cases], inst.root) == want
    # the honest proof twice and a false claim between them: a rejection moves no other member
    assert stark.verify_batch([proof, proof, proof], inst.air, [inst.boundary, wrong, inst.boundary], inst.root) == [True, False, True]


def test_honest_stark_proofs_check_every_row_on_the_device(row_counts):
    index = [i for i, r in enumerate(STARK) if r["kind"] == "rescue_prime" and r["expansion_factor"] == 16][0]
    inst = instance(index)
    stark = inst.stark
    proofs = [golden_proof(index)] * 3
    assert stark.verify_batch(proofs, inst.air, [inst.boundary] * 3, inst.root) == [True] * 3
    s, rounds = stark.fri.num_colinearity_tests, stark.fri.num_rounds()
    fri_rows = 3 * s * (rounds - 1)
    opened_rows = (stark.num_registers + 2) * 4 * s          # every committed codeword at 2 s opened points and their successors at + ef
    assert row_counts["merkle"] == len(proofs) * (fri_rows + opened_rows)
    assert row_counts["colinearity"] == len(proofs) * s * (rounds - 1)
    assert row_counts["undecided"] == row_counts["host_merkle"] == row_counts["host_colinearity"] == 0


@pytest.mark.parametrize("how", ["host rows", "device traces"])
def test_stark_prove_batch_is_three_sequential_proofs_and_member_0_the_references(how, seeded, monkeypatch):
    index = [i for i, r in enumerate(STARK) if r["kind"] == "synthetic" and r["log_fri"] == 11][0]
    inst = instance(index)
    rec, stark, T = inst.rec, inst.stark, inst.rec["original_trace_length"]
    rows, boundaries = [], []
    for m in range(3):                                     # the AIR's trace from different starting rows; member 0 is the golden's
        a, b = synth.synthetic_air_columns(T, 3 + 2 * m, 5 + m)
        rows.append([[FieldElement(x, field), FieldElement(y, field)] for x, y in zip(a, b)])
        boundaries.append([(0, 0, FieldElement(a[0], field)), (0, 1, FieldElement(b[0], field)), (T - 1, 1, FieldElement(b[T - 1], field))])
    assert [[e.value for e in row] for row in rows[0]] == [[e.value for e in row] for row in inst.rows]
    pre = inst.resident if how == "device traces" else inst.host
    traces = lambda: [DeviceTrace.from_rows(r, field) for r in rows] if how == "device traces" else [list(r) for r in rows]
    seeded(rec["urandom_seed"])
    want = [stark.prove(trace, inst.air, boundary, pre[0], pre[1]) for trace, boundary in zip(traces(), boundaries)]
    calls = []
    real = FastStark.transition_quotients_batch
    monkeypatch.setattr(FastStark, "transition_quotients_batch", lambda self, constraints, points, *a, **k: (calls.append(len(points)), real(self, constraints, points, *a, **k))[1])
    seeded(rec["urandom_seed"])
    got = stark.prove_batch(traces(), inst.air, boundaries, pre[0], pre[1])
    assert calls == [3]                                    # the members' transition quotients in one batched call
    assert got == want and len(set(got)) == 3
    is_recorded_proof(rec, got[0])
    assert stark.verify_batch(got, inst.air, boundaries, inst.root) == [True] * 3


def test_sharded_fast_stark_at_one_rank_is_the_references_proof(seeded, monkeypatch):
    """sharded_stark.ShardedFastStark(rank 0, world 1) with the HIP engine on the Rescue-Prime record at expansion factor 8: the
    FRI-to-trace domain ratio of the sharded LDEs and the sharded prover's own companion openings"""
    import torch
    import sharded_stark
    monkeypatch.setattr(sharded_stark.ShardedFastStark, "MIN_SHARDED_LOG2", 4)
    rec = [r for r in STARK if r["kind"] == "rescue_prime" and r["expansion_factor"] == 8][0]
    dev = torch.device("cuda", 0)
    make = lambda registers, cycles: sharded_stark.ShardedFastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"],
                                                                  registers, cycles, 0, 1, dev)
    stark, _, rows, air, boundary = rows_and_constraints(rec, make)
    seeded(rec["urandom_seed"])
    tz, layer, root = stark.preprocess()
    assert root.hex() == rec["zerofier_root"]
    proof = stark.prove(rows, air, boundary, tz, layer)
    is_recorded_proof(rec, proof)

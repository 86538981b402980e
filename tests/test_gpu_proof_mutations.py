"""Every single change of a proof (tests/proof_mutations.py) at the library's verifiers: Fri.verify / Fri.verify_batch and
FastStark.verify / FastStark.verify_batch (csrc/merkle_verify.cuh, csrc/combination.cuh) must reject every mutant, agree with each
other member by member, and -- for FRI -- agree with the plain verifier of tests/plain_fri_verifier.py.

Fri: n = 256, expansion 4, s = 3 (five codewords, four queried rounds), over pair leaves on / off, grinding_bits 0 / 4 and a plain or
a document-bound stream.  The library's proof is the plain prover's, byte for byte, in BOTH leaf forms.  One verify_batch call per case
holds every mutant and the honest proof at the first, a middle and the last place; its verdicts and every member's polynomial_values
are `verify`'s.  The mutants that keep every type, every length and every value below p are rejected by device rows alone (no
UNDECIDED verdict, no host fall-back); with 16 KiB staging chunks the verdicts are the same.

FastStark: the 2-register synthetic AIR on the FRI domain 2^10 with s = 8 (the instance of test_gpu_fri_pairs.py::test_fast_stark; the
security level 16 = 2 s allows no smaller s without grinding, and the one instance serves all eight cases), under all eight
combinations of pair_leaves, row_commitments and grinding_bits in {0, 4}; the combination with all three on is proved from a
DeviceTrace, the others from host rows.  The 16-register wide instance once, all three on.  There is no independent STARK verifier:
the check is the absolute property (honest accepted, every single change rejected) and the agreement of verify and verify_batch.
The leaf and row value changes alone, in a batch of their own with the combination on the device: all rejected, and no opened point
of a mutant whose values stayed canonical is decided by the host.

Measured on an MI355X machine (one honest verify; objects; mutants; the whole case).  Fri.verify takes 0.3 - 0.6 ms and a Fri case
under a second: decimal leaves 54 / 55 objects (without / with the nonce) and 729 - 738 mutants, pair leaves 30 / 31 objects and
367 - 376 mutants.  FastStark.verify takes 1.9 - 2.8 ms (16 registers: 5.2 ms); a case is the verify of every mutant, the batch of all
of them and the batch of the leaf and row changes:

    pair_leaves  row_commitments  bits   objects   mutants    case
    off          off              0 / 4  393 / 394  4084 / 4098   15 s     thinned (the full sweep: 4609 mutants, 15 s)
    off          on               0 / 4  263 / 264  3009 / 3014   10 s     thinned (3474 / 3480, 11 s)
    on           off              0 / 4  329 / 330  3318 / 3327   11 s     thinned
    on           on               0 / 4  199 / 200  2501 / 2512    7 s     the full sweep
    on           on (16 registers)    4  200        2246          15 s     thinned (2516, 15 s)

Thinned, as the cases above ten seconds are: of a sequence (a triple, a row, the last codeword, a path) the first and the last member or
depth are changed, not the first, the middle and the last.  No object, round, class of change or option combination is left out, and
the Fri cases and the smallest FastStark case keep the middle places.  Thinning takes a tenth of the mutants, so those cases stay
above ten seconds: the time is the host walk of FastStark.verify (about a millisecond per mutant) and of verify_batch's collection
(under two), thousands of times."""
import functools
import os
import pickle
import random
import time
from hashlib import blake2s, shake_256

import pytest

import fri_pairs_cases as cases
import plain_fri_verifier as plain
import proof_mutations
from fri_pairs_cases import G
from proof_mutations import label_class, label_index, mutants
from verify_spies import combination_hosts, host_verdict, row_counts           # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N, EXPANSION, S = 256, 4, 3
ROUNDS = 5
STARK_S = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()


def new_stream(document=None):
    from ip import ProofStream

    class DocumentStream(ProofStream):
        """challenges prefixed by a document's digest, as the signature scheme's are"""

        def __init__(self):
            ProofStream.__init__(self)
            self.prefix = blake2s(bytes(document)).digest()

        def prover_fiat_shamir(self, num_bytes=32):
            return shake_256(self.prefix + self.serialize()).digest(num_bytes)

        def verifier_fiat_shamir(self, num_bytes=32):
            return shake_256(self.prefix + pickle.dumps(self.objects[:self.read_index])).digest(num_bytes)

        def deserialize(self, bb):
            stream = DocumentStream()
            stream.objects = pickle.loads(bb)
            return stream

    return ProofStream() if document is None else DocumentStream()


def interleaved(honest, changed, labels):
    """the honest proof at the first, a middle and the last place of the batch -> (members, the honest places, the members' names)"""
    middle = len(changed) // 2
    members = [honest] + changed[:middle] + [honest] + changed[middle:] + [honest]
    names = ["honest"] + labels[:middle] + ["honest"] + labels[middle:] + ["honest"]
    return members, (0, middle + 1, len(members) - 1), names


def plain_values(values):
    return [(index, element.value) for index, element in values]


# ---- Fri -------------------------------------------------------------------------------------------------------------------------------
FRI_CASES = [(pair_leaves, bits, document) for pair_leaves in (False, True) for bits in (0, 4) for document in (None, b"a document")]


def fri_object_count(pair_leaves, grinding_bits):
    """the roots, the last codeword, the nonce if any; per queried round s pairs and s paths, or s triples and 3 s paths"""
    return ROUNDS + 1 + (1 if grinding_bits else 0) + (2 if pair_leaves else 4) * S * (ROUNDS - 1)


@functools.lru_cache(maxsize=None)
def fri_sweep(pair_leaves, grinding_bits, document):
    """one case's proof, mutants and `verify`'s answers, made once; callers leave them unchanged"""
    import starkcore
    from algebra import Field, FieldElement
    from fri import Fri
    field = Field.main()
    fri = Fri(field.generator(), field.primitive_nth_root(N), N, EXPANSION, S, grinding_bits=grinding_bits, pair_leaves=pair_leaves)
    assert fri.num_rounds() == ROUNDS == cases.num_rounds(N, EXPANSION, S)
    ints = cases.codeword(N, EXPANSION)
    stream = new_stream(document)
    fri.prove(starkcore.DeviceCodeword.from_list([FieldElement(v, field) for v in ints], field), stream)
    honest = stream.serialize()
    labels, changed = [], []
    for label, objects in mutants(pickle.loads(honest)):
        labels.append(label)
        changed.append(pickle.dumps(objects))
    want, want_values = [], []
    for proof in changed:
        values = []
        want.append(host_verdict(fri.verify, new_stream(document).deserialize(proof), values))
        want_values.append(values)
    return fri, ints, honest, labels, changed, want, want_values


def fri_batch(fri, document, members):
    values = [[] for _ in members]
    return fri.verify_batch([new_stream(document).deserialize(proof) for proof in members], values), values


@pytest.mark.parametrize("pair_leaves,grinding_bits,document", FRI_CASES)
def test_fri(pair_leaves, grinding_bits, document, row_counts, capsys):
    from algebra import Field, FieldElement
    field = Field.main()
    fri, ints, honest, labels, changed, want, want_values = fri_sweep(pair_leaves, grinding_bits, document)
    # the library's proof is the plain prover's: the option-off plain prover is tied to the library, which the goldens tie to the reference
    model = new_stream(document)
    prove = cases.prove if pair_leaves else plain.prove_decimal
    prove(ints, G, cases.root_of_unity(N), EXPANSION, S, model, lambda v: FieldElement(v, field), grinding_bits)
    assert honest == model.serialize()
    assert len(pickle.loads(honest)) == fri_object_count(pair_leaves, grinding_bits)
    assert {label_index(label) for label in labels} == set(range(fri_object_count(pair_leaves, grinding_bits)))
    prefix = b"" if document is None else blake2s(document).digest()
    started = time.perf_counter()
    honest_values = []
    assert fri.verify(new_stream(document).deserialize(honest), honest_values) is True
    seconds = time.perf_counter() - started
    assert plain.verify(pickle.loads(honest), N, EXPANSION, S, G, cases.root_of_unity(N), pair_leaves, grinding_bits, prefix) == (True, None)
    # every mutant: rejected by verify, and by the plain verifier
    assert [label for label, verdict in zip(labels, want) if verdict is not False] == []
    plain_verdicts = [plain.verify(pickle.loads(proof), N, EXPANSION, S, G, cases.root_of_unity(N), pair_leaves, grinding_bits, prefix)[0] for proof in changed]
    assert [label for label, verdict in zip(labels, plain_verdicts) if verdict is not False] == []
    # one batch of all of them and the honest proof three times
    members, honest_at, names = interleaved(honest, changed, labels)
    expected = [False] * len(members)
    expected_values = list(want_values)
    for place in honest_at:
        expected[place] = True
        expected_values.insert(place, honest_values)
    got, got_values = fri_batch(fri, document, members)
    assert [names[k] for k in range(len(members)) if got[k] is not expected[k]] == []
    assert [names[k] for k in range(len(members)) if plain_values(got_values[k]) != plain_values(expected_values[k])] == []
    # the changes that keep every type, length and value below p: device rows decide, nothing falls back to the host
    canonical = [proof for label, proof in zip(labels, changed) if label_class(label) in proof_mutations.CANONICAL_CLASSES]
    assert len(canonical) > len(changed) // 4
    for key in row_counts:
        row_counts[key] = 0
    verdicts, _ = fri_batch(fri, document, canonical)
    assert verdicts == [False] * len(canonical)
    assert row_counts["merkle"] > 0 and row_counts["colinearity"] > 0
    assert row_counts["undecided"] == row_counts["host_merkle"] == row_counts["host_colinearity"] == 0
    capsys.readouterr()                            # (the verifier prints a line per rejection)
    with capsys.disabled():
        print("\nMEASURED fri pair_leaves=%s bits=%d document=%s: %d objects, %d mutants, honest verify %.1f ms"
              % (pair_leaves, grinding_bits, document is not None, len(pickle.loads(honest)), len(changed), 1e3 * seconds))


@pytest.mark.parametrize("pair_leaves", (False, True))
def test_fri_batch_in_small_staging_chunks(pair_leaves):
    """16 KiB of staging (about 25 decimal-leaf rows a chunk): the rejecting rows spread over many chunks, the verdicts stay"""
    import starkcore as sc
    fri, _, honest, labels, changed, want, _ = fri_sweep(pair_leaves, 0, None)
    members, honest_at, _ = interleaved(honest, changed, labels)
    first, _ = fri_batch(fri, None, members)
    sc._check(sc.lib().sc_set_tuning(b"verify_stage_kb", 16))
    try:
        again, _ = fri_batch(fri, None, members)
    finally:
        sc._check(sc.lib().sc_set_tuning(b"verify_stage_kb", 65536))
    assert again == first
    assert [k for k, verdict in enumerate(again) if verdict] == list(honest_at)


# ---- FastStark -------------------------------------------------------------------------------------------------------------------------
STARK_CASES = [(pair_leaves, row_commitments, bits) for pair_leaves in (False, True) for row_commitments in (False, True) for bits in (0, 4)]


@functools.lru_cache(maxsize=None)
def stark_instance(registers):
    import synth
    import workloads
    from algebra import FieldElement
    if registers == 2:
        field, T, _, air, boundary = workloads.synthetic_stark_instance(10, STARK_S)
        rows = [[FieldElement(a, field), FieldElement(b, field)] for a, b in zip(*synth.synthetic_air_columns(T))]
    else:
        field, T, rows, _, air, boundary = workloads.synthetic_wide_instance(10, registers, STARK_S)
    return field, T, rows, air, boundary


def stark_object_count(stark, registers):
    """the commitments' roots, FRI's objects, then per committed tree 4 s openings of two objects each: a leaf or a row, and a path"""
    rounds, s = stark.fri.num_rounds(), STARK_S
    fri_objects = rounds + 1 + (1 if stark.grinding_bits else 0) + (2 if stark.pair_leaves else 4) * s * (rounds - 1)
    trees = 2 if stark.row_commitments else registers + 2              # (the transition zerofier's comes last, in either form)
    return (1 if stark.row_commitments else registers + 1) + fri_objects, 2 * 4 * s * trees


@functools.lru_cache(maxsize=None)
def stark_sweep(pair_leaves, row_commitments, grinding_bits, registers=2):
    """one case's prover, proof and mutants, made once.  Every case but the smallest (two registers, pair leaves and row commitments
    on) passed ten seconds with the full sweep: their sequences are thinned to the first and the last member or depth (see the module's
    docstring)"""
    from fast_stark import DeviceTrace, FastStark
    field, T, rows, air, boundary = stark_instance(registers)
    stark = FastStark(field, 4, STARK_S, 2 * STARK_S, registers, T, grinding_bits=grinding_bits, row_commitments=row_commitments, pair_leaves=pair_leaves)
    assert stark.fri_domain_length == 1 << 10
    tz, tz_codeword, root = stark.preprocess()
    trace = [list(r) for r in rows]
    if registers == 2 and pair_leaves and row_commitments and grinding_bits:
        trace = DeviceTrace.from_rows(trace, field)
    genuine, rng = os.urandom, random.Random(83)
    os.urandom = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
    try:
        honest = stark.prove(trace, air, boundary, tz, tz_codeword)
    finally:
        os.urandom = genuine
    labels, changed = [], []
    for label, objects in mutants(pickle.loads(honest), thin=not (registers == 2 and pair_leaves and row_commitments)):
        labels.append(label)
        changed.append(pickle.dumps(objects))
    return stark, air, boundary, root, honest, labels, changed


def run_stark_case(pair_leaves, row_commitments, grinding_bits, registers, combination_hosts, capsys):
    stark, air, boundary, root, honest, labels, changed = stark_sweep(pair_leaves, row_commitments, grinding_bits, registers)
    objects = pickle.loads(honest)
    head, tail = stark_object_count(stark, registers)
    assert len(objects) == head + tail
    assert {label_index(label) for label in labels} == set(range(len(objects)))
    started = time.perf_counter()
    assert stark.verify(honest, air, boundary, root) is True
    seconds = time.perf_counter() - started
    started = time.perf_counter()
    want = [host_verdict(stark.verify, proof, air, boundary, root) for proof in changed]
    sweep_seconds = time.perf_counter() - started
    assert [label for label, verdict in zip(labels, want) if verdict is not False] == []
    members, honest_at, names = interleaved(honest, changed, labels)
    started = time.perf_counter()
    got = stark.verify_batch(members, air, [boundary] * len(members), root)
    batch_seconds = time.perf_counter() - started
    assert [names[k] for k, verdict in enumerate(got) if verdict is not (k in honest_at)] == []
    # the opened leaves and rows alone: every value change of them is rejected, the canonical ones without the host's `holds`
    from fast_stark import FastStark
    assert FastStark.COMBINATION_ON_DEVICE is True
    chosen = [(label, proof) for label, proof in zip(labels, changed) if label_index(label) >= head
              and proof_mutations.kind_of(objects[label_index(label)]) in ("element", "elements") and label_class(label) in proof_mutations.VALUE_CLASSES]
    assert len({label_index(label) for label, _ in chosen}) == tail // 2
    combination_hosts["checks"].clear()
    del combination_hosts["host_owners"][:]
    verdicts = stark.verify_batch([proof for _, proof in chosen], air, [boundary] * len(chosen), root)
    assert verdicts == [False] * len(chosen)
    checks, = combination_hosts["checks"]
    canonical = {k for k, (label, _) in enumerate(chosen) if label_class(label) in proof_mutations.CANONICAL_CLASSES}
    assert len(canonical) >= tail // 2                                  # (plus_one of every leaf, and of a row's first and last member)
    assert checks.combination_device_rows >= 2 * STARK_S * len(canonical)
    assert canonical & set(combination_hosts["host_owners"]) == set()
    capsys.readouterr()
    with capsys.disabled():
        print("\nMEASURED stark registers=%d pair_leaves=%s row_commitments=%s bits=%d: %d objects, %d mutants, honest verify %.1f ms, "
              "verify of all mutants %.1f s, the batch %.1f s" % (registers, pair_leaves, row_commitments, grinding_bits, len(objects), len(changed),
                                                                    1e3 * seconds, sweep_seconds, batch_seconds))


@pytest.mark.parametrize("pair_leaves,row_commitments,grinding_bits", STARK_CASES)
def test_fast_stark(pair_leaves, row_commitments, grinding_bits, combination_hosts, capsys):
    run_stark_case(pair_leaves, row_commitments, grinding_bits, 2, combination_hosts, capsys)


def test_fast_stark_wide(combination_hosts, capsys):
    """16 registers (the column-batched prover), all three options on: rows of 17 values"""
    run_stark_case(True, True, 4, 16, combination_hosts, capsys)

"""FastStark and FastRPSSS with row_commitments=True on the GPU (fast_stark.py; the kernels and entries underneath:
tests/test_gpu_merkle_rows.py): proofs verify and are shorter, one commitment stands in front of FRI's objects, the opened rows are
the committed columns, verify_batch agrees with verify on altered proofs, the host-list data flow, the default unchanged,
prove_batch / sign_batch member by member, the sharded prover's refusal.
A file of its own, named to run behind tests/test_gpu_prove_batch.py: one test there counts the device copies of DeviceTraces whose
columns are separate allocations and so depends on where the library's pool hands those allocations out; provers that take vectors
from the pool and give them back in front of it change that."""
import functools
import os
import pickle
import random

import pytest

import merkle_rows_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


@pytest.fixture
def seeded(monkeypatch):
    def seed(value):
        rng = random.Random(value)
        monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    return seed


S = 8                                              # colinearity checks: 4 S = 32 opened positions


@functools.lru_cache(maxsize=None)
def instance(registers):
    """the smallest FRI domain (2^10) at which the 16-register workload is legal with 8 colinearity checks, and the 2-register
    workload at the same size: (field, trace rows as lists, air, boundary, prover with the option off, with it on, preprocessing)"""
    import synth
    import workloads
    from algebra import FieldElement
    from fast_stark import FastStark
    if registers == 2:
        field, T, _, air, boundary = workloads.synthetic_stark_instance(10, S)
        rows = [[FieldElement(a, field), FieldElement(b, field)] for a, b in zip(*synth.synthetic_air_columns(T))]
    else:
        field, T, rows, _, air, boundary = workloads.synthetic_wide_instance(10, registers, S)
    off = FastStark(field, 4, S, 2 * S, registers, T)
    on = FastStark(field, 4, S, 2 * S, registers, T, row_commitments=True)
    assert on.fri_domain_length == 1 << 10 and on.row_commitments is True and off.row_commitments is False
    return field, rows, air, boundary, off, on, off.preprocess()


def prove(stark, registers, device_trace=False):
    from fast_stark import DeviceTrace
    field, rows, air, boundary, _, _, (tz, tz_codeword, _) = instance(registers)
    trace = [list(r) for r in rows]
    if device_trace:
        trace = DeviceTrace.from_rows(trace, field)
    return stark.prove(trace, air, boundary, tz, tz_codeword)


def layout_of(stark, proof):
    """(objects, place of the first opened row): behind the commitments come FRI's roots, its last codeword and its query triples;
    the committed openings are the proof's tail -- with the option on 4 S (row, path) pairs, then the zerofier's 4 S (leaf, path) pairs"""
    objects = pickle.loads(proof)
    return objects, len(objects) - 4 * (4 * S)


@pytest.mark.parametrize("registers", (16, 2))
@pytest.mark.parametrize("device_trace", (False, True))
def test_proofs_verify_and_are_shorter(sc, seeded, registers, device_trace):
    field, rows, air, boundary, off, on, (_, _, root) = instance(registers)
    seeded(41)
    proof = prove(on, registers, device_trace)
    seeded(41)
    default = prove(off, registers, device_trace)
    assert on.verify(proof, air, boundary, root) is True
    assert off.verify(default, air, boundary, root) is True
    assert len(proof) < len(default)
    # exactly one commitment in front of FRI's objects; one row and one path per position instead of registers + 1 of each
    objects, first = layout_of(on, proof)
    rounds = on.fri.num_rounds()
    assert all(type(o) is bytes and len(o) == 64 for o in objects[:1 + rounds]) and type(objects[1 + rounds]) is list
    defaults = pickle.loads(default)
    assert all(type(o) is bytes and len(o) == 64 for o in defaults[:registers + 1 + rounds]) and type(defaults[registers + 1 + rounds]) is list
    assert len(defaults) - len(objects) == registers + 2 * (4 * S) * registers
    for j in range(4 * S):
        row, path = objects[first + 2 * j], objects[first + 2 * j + 1]
        assert type(row) is list and len(row) == registers + 1 and type(path) is list and len(path) == 10


def test_row_openings_travel_as_a_description(sc, seeded):
    """on a plain ProofStream the opened rows are pushed as the device answered them (proof_objects.RowOpenings) and pickled by the
    library from their description: the same bytes as pickle.dumps of the objects they stand for"""
    import proof_objects
    from ip import ProofStream
    registers = 16
    field, rows, air, boundary, off, on, (tz, tz_codeword, root) = instance(registers)
    stream = ProofStream()
    seeded(67)
    proof = on.prove([list(r) for r in rows], air, boundary, tz, tz_codeword, stream)
    assert sum(isinstance(segment, proof_objects.RowOpenings) for segment in stream.objects._segments) == 1
    assert proof == pickle.dumps(stream.objects.materialized())
    assert on.verify(proof, air, boundary, root) is True


def test_opened_rows_are_the_committed_columns(sc, seeded, monkeypatch):
    """the same seeded os.urandom gives both modes the same boundary-quotient and randomizer codewords (the root differs, hence the
    sampled positions): the rows the option opens, and the values the default proof opens column by column, are those codewords'"""
    registers = 16
    field, rows, air, boundary, off, on, _ = instance(registers)
    captured, start = [], sc.RowTree.start
    monkeypatch.setattr(sc.RowTree, "start", classmethod(lambda cls, columns: captured.append(start(columns)) or captured[-1]))
    seeded(43)
    proof = prove(on, registers)
    seeded(43)
    default = prove(off, registers)
    (tree,) = captured
    columns = [sc.unpack(v.to_bytes()) for v in tree.vectors]
    assert len(columns) == registers + 1
    objects, first = layout_of(on, proof)
    assert objects[0] == tree.root
    opened = []
    on.fri.verify(_stream_behind(objects, 1), opened)
    positions = sorted([i for i, _ in opened] + [(i + 4) % 1024 for i, _ in opened])
    assert len(positions) == 4 * S
    for j, position in enumerate(positions):
        row, path = objects[first + 2 * j], objects[first + 2 * j + 1]
        assert [v.value for v in row] == [column[position] for column in columns]
        assert cases.verify(tree.root, position, path, [v.value for v in row])
    defaults = pickle.loads(default)
    opened = []
    off.fri.verify(_stream_behind(defaults, registers + 1), opened)
    positions = sorted([i for i, _ in opened] + [(i + 4) % 1024 for i, _ in opened])
    tail = len(defaults) - (registers + 2) * 2 * (4 * S)
    for c in range(registers + 1):
        for j, position in enumerate(positions):
            assert defaults[tail + c * 2 * (4 * S) + 2 * j].value == columns[c][position]


def _stream_behind(objects, commitments):
    """a proof stream read up to FRI's first object"""
    from ip import ProofStream
    stream = ProofStream()
    stream.objects = list(objects)
    stream.read_index = commitments
    return stream


def test_verify_batch_agrees_with_verify(sc, seeded):
    registers = 16
    field, rows, air, boundary, off, on, (_, _, root) = instance(registers)
    from algebra import FieldElement
    seeded(47)
    proof = prove(on, registers)
    objects, first = layout_of(on, proof)

    def altered(change):
        changed = pickle.loads(proof)
        change(changed)
        return pickle.dumps(changed)

    def bump_value(o):
        o[first][3] = FieldElement((o[first][3].value + 1) % field.p, field)

    def bump_digest(o):
        o[first + 1][2] = bytes([o[first + 1][2][0] ^ 1]) + o[first + 1][2][1:]

    def shorten_row(o):
        o[first + 2] = o[first + 2][:-1]

    def bump_root(o):
        o[0] = bytes([o[0][0] ^ 1]) + o[0][1:]

    def shorten_path(o):
        o[first + 5] = o[first + 5][:-1]

    def foreign_value(o):
        o[first + 4][0] = FieldElement(field.p, field)          # not below p

    proofs = [proof] + [altered(change) for change in (bump_value, bump_digest, shorten_row, bump_root, shorten_path, foreign_value)]
    expected = [True] + [False] * 6
    assert [on.verify(p, air, boundary, root) for p in proofs] == expected
    assert on.verify_batch(proofs, air, [boundary] * len(proofs), root) == expected


@pytest.mark.parametrize("rows_device_min", (256, 10 ** 9))
def test_host_list_flow(sc, seeded, monkeypatch, rows_device_min):
    """a prover kept off the device data flow (DEVICE_MIN out of reach: host lists, Merkle.commit_rows / open_rows -- with the row tree
    built on the GPU from the lists, and with the pure-host bodies) gives the proof of the device data flow, object for object, and it
    verifies"""
    from fast_stark import FastStark
    from merkle import Merkle
    monkeypatch.setattr(Merkle, "ROWS_DEVICE_MIN", rows_device_min)
    registers = 2
    field, rows, air, boundary, off, on, (_, _, root) = instance(registers)
    seeded(53)
    resident_flow = prove(on, registers)
    monkeypatch.setattr(FastStark, "DEVICE_MIN", 10 ** 9)
    seeded(53)
    host_flow = prove(on, registers)
    assert on.verify(host_flow, air, boundary, root) is True
    assert pickle.loads(host_flow) == pickle.loads(resident_flow)
    objects = pickle.loads(host_flow)
    rounds = on.fri.num_rounds()
    assert all(type(o) is bytes for o in objects[:1 + rounds]) and type(objects[1 + rounds]) is list


def test_default_is_unchanged(sc, seeded):
    """row_commitments=False is the prover with the keyword omitted, byte for byte (the golden proofs are the real guard)"""
    from fast_stark import FastStark
    registers = 2
    field, rows, air, boundary, off, on, _ = instance(registers)
    explicit = FastStark(field, 4, S, 2 * S, registers, off.original_trace_length, row_commitments=False)
    seeded(59)
    first = prove(off, registers, device_trace=True)
    seeded(59)
    assert prove(explicit, registers, device_trace=True) == first


def test_prove_batch_goes_member_by_member(sc, seeded):
    registers = 2
    field, rows, air, boundary, off, on, (tz, tz_codeword, root) = instance(registers)
    traces = [[list(r) for r in rows] for _ in range(2)]
    assert off._batch_served(traces, [boundary] * 2) is True and on._batch_served(traces, [boundary] * 2) is False
    seeded(61)
    alone = [prove(on, registers) for _ in range(2)]
    seeded(61)
    assert on.prove_batch(traces, air, [boundary] * 2, tz, tz_codeword) == alone
    assert on.verify_batch(alone, air, [boundary] * 2, root) == [True, True]


@functools.lru_cache(maxsize=None)
def signer():
    from fast_rpsss import FastRPSSS
    return FastRPSSS(row_commitments=True)


def test_signature(sc):
    scheme = signer()
    assert scheme.stark.row_commitments is True
    sk = scheme.field.sample(b"a key for a row-committed signature")
    pk = scheme.rp.hash(sk)
    signature = scheme.sign(sk, b"a document")
    assert scheme.verify(pk, b"a document", signature) is True
    assert scheme.verify(pk, b"another document", signature) is False


def test_sign_batch(sc):
    scheme = signer()
    sks = [scheme.field.sample(b"key %d of a row-committed batch" % k) for k in range(2)]
    pks = scheme.rp.hash_batch(sks)
    documents = [b"document %d" % k for k in range(2)]
    signatures = scheme.sign_batch(sks, documents)
    assert [scheme.verify(pk, d, s) for pk, d, s in zip(pks, documents, signatures)] == [True, True]
    assert scheme.verify_batch(pks, documents, signatures) == [True, True]
    assert scheme.verify_batch(pks, documents, signatures[::-1]) == [False, False]


def test_sharded_prover_refuses():
    from algebra import Field
    from sharded_stark import ShardedFastStark
    with pytest.raises(AssertionError, match="row_commitments is not supported"):
        ShardedFastStark(Field.main(), 4, S, 2 * S, 2, 32, 0, 1, None, row_commitments=True)

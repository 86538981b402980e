"""FastStark(row_commitments=True).prove_batch and FastRPSSS(row_commitments=True).sign_batch on the batched path (fast_stark.py
_rows_batch_served / _prove_chunk; the row forest underneath: tests/test_gpu_row_forest.py): under a seeded os.urandom
the proofs are those of sequential `prove` / `sign` calls byte for byte and every stream holds the same objects, they verify, an
altered row is rejected, the forests built are the row-committed path's (ONE row forest per chunk, none over single codewords), chunks,
batches that are not served, a false witness, signatures with and without grinding, the default unchanged.
The instances are those of tests/test_gpu_row_commitment_proofs.py (FRI domain 2^10, 8 colinearity checks), K members each; the file
is named to run behind that one."""
import functools
import os
import pickle
import random

import pytest

pytestmark = pytest.mark.gpu

S = 8                                              # colinearity checks: 4 S = 32 opened positions


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


class Instance:
    """three members of one AIR at FRI 2^10: host rows, boundaries, the provers with the option on and off, the preprocessing"""

    def __init__(self, registers):
        import synth
        import workloads
        from algebra import FieldElement
        from fast_stark import FastStark
        self.registers = registers
        if registers == 2:
            field, T, _, self.air, _ = workloads.synthetic_stark_instance(10, S)
        else:
            field, T, _, _, self.air, _ = workloads.synthetic_wide_instance(10, registers, S)
        self.field, self.rows, self.boundaries = field, [], []
        for m in range(3):
            if registers == 2:
                a, b = synth.synthetic_air_columns(T, 3 + 2 * m, 5 + m)
                mine = [list(pair) for pair in zip(a, b)]
                named = [(0, 0), (0, 1), (T - 1, 1)]
            else:
                row = [7 * i + 3 + m for i in range(registers)]
                mine = [row]
                for _ in range(T - 1):
                    row = [(row[i] * row[i] + row[(i + 1) % registers]) % field.p for i in range(registers)]
                    mine.append(row)
                named = [(0, i) for i in range(registers)] + [(T - 1, 0)]
            self.rows.append([[FieldElement(v, field) for v in row] for row in mine])
            self.boundaries.append([(cycle, register, FieldElement(mine[cycle][register], field)) for cycle, register in named])
        self.off = FastStark(field, 4, S, 2 * S, registers, T)
        self.on = FastStark(field, 4, S, 2 * S, registers, T, row_commitments=True)
        assert self.on.fri_domain_length == 1 << 10
        self.tz, self.tz_codeword, self.root = self.off.preprocess()

    def traces(self, K, device=False, rows=None):
        from fast_stark import DeviceTrace
        rows = self.rows[:K] if rows is None else rows
        return [DeviceTrace.from_rows([list(r) for r in member], self.field) if device else [list(r) for r in member] for member in rows]

    def sequential(self, stark, seeded, seed, K, device=False, streams=None, rows=None, boundaries=None):
        seeded(seed)
        streams = [None] * K if streams is None else streams
        boundaries = self.boundaries[:K] if boundaries is None else boundaries
        return [stark.prove(trace, self.air, boundary, self.tz, self.tz_codeword, stream)
                for trace, boundary, stream in zip(self.traces(K, device, rows), boundaries, streams)]

    def batch(self, stark, seeded, seed, K, device=False, streams=None, rows=None, boundaries=None):
        seeded(seed)
        return stark.prove_batch(self.traces(K, device, rows), self.air, self.boundaries[:K] if boundaries is None else boundaries, self.tz, self.tz_codeword, streams)


@functools.lru_cache(maxsize=None)
def instance(registers):
    return Instance(registers)


# ---- prove_batch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", (False, True), ids=("host-rows", "device-traces"))
@pytest.mark.parametrize("registers", (2, 16))
@pytest.mark.parametrize("K", (1, 2, 3))
def test_batch_is_the_sequential_proofs(sc, seeded, K, registers, device):
    """the proofs and the streams' objects of K `prove` calls; R = 16: a row of 17 values crosses two blocks.  The batch is served by
    ONE row forest of K trees (and FRI's forest per round): no forest over the boundary-quotient or the randomizer codewords."""
    from ip import ProofStream
    import proof_objects
    inst = instance(registers)
    on = inst.on
    traces = inst.traces(K, device)
    assert on._rows_batch_served(traces, inst.boundaries[:K]) is True and on._batch_served(traces, inst.boundaries[:K]) is False
    assert inst.off._rows_batch_served(traces, inst.boundaries[:K]) is False
    alone_streams, streams = [ProofStream() for _ in range(K)], [ProofStream() for _ in range(K)]
    want = inst.sequential(on, seeded, 71, K, device, alone_streams)
    inst.batch(on, seeded, 71, K, device)              # (the zerofier's forest exists from here on)
    before = sc.forest_stats()
    got = inst.batch(on, seeded, 71, K, device, streams)
    after = sc.forest_stats()
    assert got == want and len(set(got)) == K
    rounds = on.fri.num_rounds()
    assert (after[0] - before[0], after[1] - before[1]) == (1 + rounds, K + K * rounds)
    for mine, alone in zip(streams, alone_streams):
        assert list(mine.objects) == list(alone.objects)
        # on a plain ProofStream the rows travel as a description
        assert sum(isinstance(segment, proof_objects.RowOpenings) for segment in mine.objects._segments) == 1
    assert [on.verify(proof, inst.air, boundary, inst.root) for proof, boundary in zip(got, inst.boundaries)] == [True] * K
    assert on.verify_batch(got, inst.air, inst.boundaries[:K], inst.root) == [True] * K


def test_an_altered_row_is_rejected(sc, seeded):
    from algebra import FieldElement
    inst = instance(16)
    on, field = inst.on, inst.field
    proofs = inst.batch(on, seeded, 73, 3)
    altered = []
    for m, proof in enumerate(proofs):
        objects = pickle.loads(proof)
        first = len(objects) - 4 * (4 * S)             # 4 S (row, path) pairs, then the zerofier's 4 S (leaf, path) pairs
        row = objects[first + 2 * m]
        assert type(row) is list and len(row) == 17 and len(objects[first + 2 * m + 1]) == 10
        row[5 * m] = FieldElement((row[5 * m].value + 1) % field.p, field)
        altered.append(pickle.dumps(objects))
    assert [on.verify(proof, inst.air, boundary, inst.root) for proof, boundary in zip(altered, inst.boundaries)] == [False] * 3
    mixed = [proofs[0], altered[1], proofs[2]]
    assert on.verify_batch(mixed, inst.air, inst.boundaries, inst.root) == [True, False, True]


def test_chunks(sc, seeded, monkeypatch):
    """FOREST_MAX_LEAVES = the leaves of two members' boundary-quotient codewords: three members go as 2 + 1 -- two row forests, of two
    trees and of one -- and the bytes do not move"""
    inst = instance(2)
    on = inst.on
    want = inst.sequential(on, seeded, 79, 3)
    inst.batch(on, seeded, 79, 3)
    rounds, R, N = on.fri.num_rounds(), on.num_registers, on.fri_domain_length
    monkeypatch.setattr(sc, "FOREST_MAX_LEAVES", 2 * R * N)
    built = []
    build = sc.RowForest.build.__func__
    monkeypatch.setattr(sc.RowForest, "build", classmethod(lambda cls, segments, n, count: built.append(count) or build(cls, segments, n, count)))
    before = sc.forest_stats()
    got = inst.batch(on, seeded, 79, 3)
    after = sc.forest_stats()
    assert got == want and built == [2, 1]
    assert (after[0] - before[0], after[1] - before[1]) == (2 * (1 + rounds), 3 * (1 + rounds))


def test_another_boundary_layout_goes_member_by_member(sc, seeded):
    """member 1 names one pair less: not served, decided before any draw -- K calls of `prove`, no forest"""
    inst = instance(2)
    on = inst.on
    boundaries = [inst.boundaries[0], [inst.boundaries[1][0], inst.boundaries[1][2]], inst.boundaries[2]]
    assert on._rows_batch_served(inst.traces(3), boundaries) is False
    want = inst.sequential(on, seeded, 83, 3, boundaries=boundaries)
    before = sc.forest_stats()
    got = inst.batch(on, seeded, 83, 3, boundaries=boundaries)
    assert sc.forest_stats() == before and got == want
    assert on.verify_batch(got, inst.air, boundaries, inst.root) == [True] * 3


def outcome(fn):
    try:
        return ("ok", fn())
    except AssertionError as e:
        return ("raised", str(e))


def test_false_witness(sc, seeded):
    """member 1 of 3 with a bent cell that a boundary condition pins: the batch raises `prove`'s assertion and returns no proofs, every
    stream holds a prefix of `prove`'s pushes, and every check was read -- correct batches run afterwards, more of them than a leaked
    pinned slot per failure would leave room for"""
    from algebra import FieldElement
    from ip import ProofStream
    inst = instance(2)
    on = inst.on
    bent = [list(row) for row in inst.rows[1]]
    bent[0][1] = bent[0][1] + FieldElement(1, inst.field)
    rows = [inst.rows[0], bent, inst.rows[2]]
    seeded(89)
    alone = outcome(lambda: on.prove([list(r) for r in bent], inst.air, inst.boundaries[1], inst.tz, inst.tz_codeword))
    assert alone == ("raised", "cannot perform polynomial division because remainder is not zero")
    honest = [ProofStream() for _ in range(3)]
    inst.batch(on, seeded, 89, 3, streams=honest)
    for _ in range(3):
        streams = [ProofStream() for _ in range(3)]
        assert outcome(lambda: inst.batch(on, seeded, 89, 3, streams=streams, rows=rows)) == alone
        for m, (bad, good) in enumerate(zip(streams, honest)):
            assert m == 1 or list(bad.objects) == list(good.objects)[:len(bad.objects)]
            assert len(bad.objects) <= 1                # at most the row root: nothing behind the collected checks
    assert inst.batch(on, seeded, 89, 3) == inst.sequential(on, seeded, 89, 3)


def test_option_off_is_unchanged(sc, seeded):
    """the default prover's batch is still the sequential proofs (which the golden proofs pin), served by the per-codeword forests"""
    inst = instance(2)
    off = inst.off
    assert off._batch_served(inst.traces(3), inst.boundaries) is True
    want = inst.sequential(off, seeded, 97, 3)
    inst.batch(off, seeded, 97, 3)
    before = sc.forest_stats()
    got = inst.batch(off, seeded, 97, 3)
    after = sc.forest_stats()
    rounds, R = off.fri.num_rounds(), off.num_registers
    assert got == want
    assert (after[0] - before[0], after[1] - before[1]) == (2 + rounds, 3 * R + 3 + 3 * rounds)


# ---- signatures ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signer(grinding_bits=0):
    from fast_rpsss import FastRPSSS
    return FastRPSSS(num_colinearity_checks=64 - grinding_bits // 2, grinding_bits=grinding_bits, row_commitments=True)


@pytest.mark.parametrize("K,grinding_bits", [(1, 0), (3, 0), (3, 8)])
def test_sign_batch(sc, seeded, K, grinding_bits):
    """sign_batch is K `sign` calls under the same draws, served by one row forest; on a SignatureProofStream the rows travel as
    objects; verify_batch accepts the signatures and rejects them in another order"""
    from fast_rpsss import SignatureProofStream
    scheme = signer(grinding_bits)
    stark = scheme.stark
    assert stark.row_commitments is True and stark.grinding_bits == grinding_bits
    sks = [scheme.field.sample(b"key %d of a row-forest batch" % k) for k in range(K)]
    pks = scheme.rp.hash_batch(sks)
    documents = [b"document %d" % k for k in range(K)]
    seeded(101)
    alone = [scheme.sign(sk, document) for sk, document in zip(sks, documents)]
    seeded(101)
    scheme.sign_batch(sks, documents)
    rounds = stark.fri.num_rounds()
    streams = [SignatureProofStream(document) for document in documents]
    before = sc.forest_stats()
    seeded(101)
    together = scheme.stark_prove_batch(sks, streams)
    after = sc.forest_stats()
    assert together == alone
    assert (after[0] - before[0], after[1] - before[1]) == (1 + rounds, K + K * rounds)
    checks = stark.num_colinearity_checks
    for stream in streams:                             # objects, not a description: a list of FieldElements and a list of digests per position
        assert type(stream.objects) is list
        first = len(stream.objects) - 4 * (4 * checks)
        assert type(stream.objects[first]) is list and len(stream.objects[first]) == scheme.rp.m + 1
        assert all(type(digest) is bytes for digest in stream.objects[first + 1])
    assert scheme.verify_batch(pks, documents, together) == [True] * K
    assert [scheme.verify(pk, d, s) for pk, d, s in zip(pks, documents, together)] == [True] * K
    if K > 1:
        assert scheme.verify_batch(pks, documents, together[1:] + together[:1]) == [False] * K

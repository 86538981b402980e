"""Every prover route with a proof of work in it, beyond the N = 32 proofs of tests/test_gpu_grind_proofs.py: Fri.prove where all rounds
run inside the persistent tail kernel (2^10) and where classic rounds come first (2^18), with the tail kernel on and off and from a
host list; Fri.prove with further codewords opened in the same call (the extra_trees of sc_fri_prove_grind_dev); Fri.prove_batch with
further forests, whole and split into chunks; FastStark.prove_batch on a trace wide enough for column batches; FastRPSSS.sign_batch /
verify_batch; ShardedFri's refusal.  The nonce moves every later object of a stream one place on, so of every proof made here the
same four things are asserted as at N = 32: the nonce is the hashlib loop's, the indices are sampled over the stream with it,
verify and verify_batch accept, and an altered nonce is rejected for that member only."""
import ctypes
import os
import pickle
import random

import pytest

import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()


import grinding                                    # noqa: E402
import starkcore as sc                             # noqa: E402
from algebra import Field, FieldElement            # noqa: E402
from fri import AlsoOpen, AlsoOpenForests, Fri     # noqa: E402
from ip import ProofStream                         # noqa: E402
from merkle import Merkle                          # noqa: E402
from starkcore import CodewordMatrix, DeviceCodeword, DeviceVector, MerkleForest   # noqa: E402

field = Field.main()
BITS = 10                                          # a hashlib search of a thousand trials or so
N2, S2, SHIFT = 1 << 10, 10, 4                     # the batched shape of tests/test_gpu_fri_batch_also_open.py


@pytest.fixture
def seeded(monkeypatch):
    def seed(value):
        rng = random.Random(value)
        monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    return seed


def codeword(seed, N):
    """the coset evaluation of N / 4 synthetic coefficients on the FRI domain of length N, on the device"""
    vec, src = DeviceVector(N), DeviceVector.from_bytes(synth.synth_packed(seed, N // 4).tobytes())
    sc._check(sc.lib().sc_coset_evaluate_dev(src.ptr, N // 4, sc.fe_bytes(field.generator().value), sc.fe_bytes(field.primitive_nth_root(N).value), N, vec.ptr, None))
    return DeviceCodeword(vec, field)


def fresh(cw):
    return DeviceCodeword(DeviceVector.from_bytes(cw.vec.to_bytes()), field)


def make_fri(N, s, bits=BITS):
    return Fri(field.generator(), field.primitive_nth_root(N), N, 4, s, grinding_bits=bits)


def stream_of(objects):
    ps = ProofStream()
    ps.objects = list(objects)
    return ps


def tail_stats():
    out = (ctypes.c_uint64 * 2)()
    sc._check(sc.lib().sc_fri_tail_stats(out))
    return out[0], out[1]                          # launches, launches that gave up


def nonce_and_seed(fri, objects):
    """the nonce behind the roots and the last codeword, checked against the hashlib loop over the seed of the objects in front of it"""
    rounds = fri.num_rounds()
    nonce = objects[rounds + 1]
    seed = stream_of(objects[:rounds + 1]).prover_fiat_shamir()
    assert type(nonce) is int and nonce == grinding.grind_host(seed, fri.grinding_bits)
    return nonce, seed


def the_four_things(fri, objects, top):
    """(1) the nonce, (2) the indices, (3) acceptance, (4) rejection of nonce + 1 and of the next accepted nonce, for that member only"""
    objects = list(objects)
    rounds, N, s = fri.num_rounds(), fri.domain_length, fri.num_colinearity_tests
    nonce, seed = nonce_and_seed(fri, objects)
    assert list(top) == fri.sample_indices(stream_of(objects[:rounds + 2]).prover_fiat_shamir(), N // 2, N >> (rounds - 1), s)
    assert len(objects) == rounds + 2 + 4 * s * (rounds - 1)
    assert fri.verify(stream_of(objects), []) is True
    assert fri.verify_batch([stream_of(objects)], [[]]) == [True]
    for other in (nonce + 1, grinding.grind_host(seed, fri.grinding_bits, nonce + 1)):
        altered = objects[:rounds + 1] + [other] + objects[rounds + 2:]
        assert fri.verify(stream_of(altered), []) is False
        assert fri.verify_batch([stream_of(objects), stream_of(altered), stream_of(objects)], [[], [], []]) == [True, False, True]
    return nonce


# ---- Fri.prove ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN,s", [(10, 10), (18, 10)])
def test_fri_prove_with_the_tail_kernel_and_without(logN, s, monkeypatch, capsys):
    """2^10: every round inside the tail kernel; 2^18: the rounds at 2^18 and 2^17 are classic launches, the tail kernel takes over
    from 2^16 down.  fri_tail 1 and 0 write the same bytes; so does the route through a host list (2^10)."""
    N = 1 << logN
    fri = make_fri(N, s)
    cw = codeword(700 + logN, N)
    taken = []
    real = Fri._prove_in_library

    def watched(self, *args):
        result = real(self, *args)
        taken.append(result is not None)
        return result
    monkeypatch.setattr(Fri, "_prove_in_library", watched)
    made = []
    for tail in (1, 0):
        sc.set_tuning("fri_tail", tail)
        try:
            before = tail_stats()
            ps = ProofStream()
            top = fri.prove(fresh(cw), ps)
            after = tail_stats()
        finally:
            sc.set_tuning("fri_tail", 1)
        assert after == (before[0] + tail, before[1]), tail           # launched when it should be, and did not give up
        made.append((top, ps.serialize()))
    assert taken == [True, True]
    assert made[0] == made[1]
    if logN == 10:
        before = tail_stats()
        by_phases = ProofStream()
        assert fri.prove(cw.tolist(), by_phases) == made[0][0]
        assert taken == [True, True, False]
        assert tail_stats() == (before[0] + 1, before[1])              # (its commit phase is sc_fri_commit_dev: the tail kernel again)
        assert by_phases.serialize() == made[0][1]
    the_four_things(fri, pickle.loads(made[0][1]), made[0][0])
    capsys.readouterr()                                                # (verify prints its reason for a rejection)


def expected_positions(indices, N):
    """opened_positions of FastStark.prove (fast_stark.py:154-158)"""
    duplicated = [i for i in indices] + [(i + SHIFT) % N for i in indices]
    return sorted(duplicated + [(i + (N // 2)) % N for i in duplicated])


def test_fri_prove_with_further_codewords_opened_in_the_call(monkeypatch, capsys):
    """also_open: two committed codewords opened by sc_fri_prove_grind_dev itself at the positions of the indices sampled WITH the
    nonce; the stream is the one without the keyword"""
    fri = make_fri(N2, S2)
    cw = codeword(9000, N2)
    committed = [codeword(5000, N2), codeword(5001, N2)]
    roots = [Merkle.commit(c) for c in committed]
    plain = ProofStream()
    top = fri.prove(fresh(cw), plain)
    also = AlsoOpen(lambda indices: (committed, [expected_positions(indices, N2)] * len(committed)), codewords=committed, shift=SHIFT)
    taken = []
    real = Fri._prove_in_library

    def watched(self, *args):
        result = real(self, *args)
        taken.append(result is not None)
        return result
    monkeypatch.setattr(Fri, "_prove_in_library", watched)
    ps = ProofStream()
    assert fri.prove(fresh(cw), ps, also) == top
    assert taken == [True]                                             # one library call, the search and the further openings inside it
    assert ps.serialize() == plain.serialize()
    the_four_things(fri, pickle.loads(ps.serialize()), top)
    positions = expected_positions(top, N2)
    assert len(also.answers) == len(also.position_arrays) == 2
    for root, (values, paths), where in zip(roots, also.answers, also.position_arrays):
        assert [int(w) for w in where] == positions
        residues = sc.unpack(bytes(values))
        assert len(residues) == len(paths) == 4 * S2
        for index, value, path in zip(positions, residues, paths):
            digests = [bytes(path[64 * k:64 * k + 64]) for k in range(len(path) // 64)]
            assert len(digests) == 10 and Merkle.verify(root, index, digests, FieldElement(value, field)), index
    # the same request served phase by phase (a host list): the same stream, answers at the same positions
    phased = AlsoOpen(lambda indices: (committed, [expected_positions(indices, N2)] * len(committed)), codewords=committed, shift=SHIFT)
    by_phases = ProofStream()
    assert fri.prove(cw.tolist(), by_phases, phased) == top and by_phases.serialize() == plain.serialize()
    capsys.readouterr()


# ---- Fri.prove_batch ---------------------------------------------------------------------------------------------------------------
def further_forests(K, N):
    """(forests, owners): two trees per member in one forest, one tree for everybody in the other"""
    pairs = [codeword(5000 + k, N) for k in range(2 * K)]
    forests = [MerkleForest.build(CodewordMatrix.from_members(pairs)), MerkleForest.build(CodewordMatrix.from_members([codeword(4999, N)]))]
    return forests, [[[2 * m, 2 * m + 1] for m in range(K)], [[0] for _ in range(K)]]


def check_answers(also, forests, owners, tops, N):
    K = len(tops)
    assert len(also.answers) == len(also.positions) == K
    for m in range(K):
        assert also.positions[m] == expected_positions(tops[m], N)
        pairs = [(p, tree) for p in range(len(forests)) for tree in owners[p][m]]
        assert len(also.answers[m]) == len(pairs)
        for (p, tree), (values, paths) in zip(pairs, also.answers[m]):
            want_values, want_paths = forests[p].query([(tree, i) for i in also.positions[m]])
            assert list(values) == list(want_values) and [list(path) for path in paths] == [list(path) for path in want_paths], (m, p, tree)
            for index, value, path in zip(also.positions[m], values, paths):
                assert Merkle.verify(forests[p].roots[tree], index, path, FieldElement(value, field)), (m, p, tree, index)


@pytest.mark.parametrize("split", [False, True])
def test_fri_prove_batch_with_further_forests(split, monkeypatch, capsys):
    """5 members with also_open against 5 single calls, byte for byte; split: FOREST_MAX_LEAVES = 2 rows, chunks of 2, 2 and 1 (one
    sc_grind_batch per chunk).  Every member's nonce is its own stream's minimum."""
    K = 5
    fri = make_fri(N2, S2)
    base = [codeword(9000 + k, N2) for k in range(K)]
    forests, owners = further_forests(K, N2)
    single = [ProofStream() for _ in range(K)]
    want = [fri.prove(fresh(cw), ps) for cw, ps in zip(base, single)]
    also = AlsoOpenForests(forests, owners, SHIFT)
    together = [ProofStream() for _ in range(K)]
    before = sc.forest_stats()
    with monkeypatch.context() as mp:
        if split:
            mp.setattr(sc, "FOREST_MAX_LEAVES", 2 * N2)
        got = fri.prove_batch([fresh(cw) for cw in base], together, also)
    assert sc.forest_stats()[0] - before[0] == (3 if split else 1) * fri.num_rounds()
    assert got == want
    assert [s.serialize() for s in together] == [s.serialize() for s in single]
    check_answers(also, forests, owners, got, N2)
    nonces = [the_four_things(fri, pickle.loads(s.serialize()), top) for s, top in zip(together, got)]
    assert len(set(nonces)) == K
    assert fri.verify_batch([stream_of(pickle.loads(s.serialize())) for s in together], [[] for _ in together]) == [True] * K
    capsys.readouterr()


# ---- FastStark.prove_batch on a wide trace ------------------------------------------------------------------------------------------
def nonce_place(proof):
    (k,) = [k for k, o in enumerate(pickle.loads(proof)) if type(o) is int]
    return k


def nonce_and_indices_in_a_stark_proof(fri, proof, first_root, front):
    """the first two of the four things on a STARK proof, whose top-level indices no call returns: the nonce is the hashlib loop's over
    the objects in front of it, and the first round's `a` openings -- triple t's first element with the path at k + 1 + s + 3 t --
    lead to FRI's first root at the indices sampled over the stream WITH the nonce.  front(objects): a stream of the proof's kind."""
    objects = pickle.loads(proof)
    k, rounds, N, s = nonce_place(proof), fri.num_rounds(), fri.domain_length, fri.num_colinearity_tests
    assert k == first_root + rounds + 1
    seed = front(objects[:k]).prover_fiat_shamir()
    assert objects[k] == grinding.grind_host(seed, fri.grinding_bits)
    indices = fri.sample_indices(front(objects[:k + 1]).prover_fiat_shamir(), N // 2, N >> (rounds - 1), s)
    for t, index in enumerate(indices):
        assert Merkle.verify(objects[first_root], index, objects[k + 1 + s + 3 * t], objects[k + 1 + t][0]), t
    return objects[k], grinding.grind_host(seed, fri.grinding_bits, objects[k] + 1)


def with_object(proof, place, change):
    objects = pickle.loads(proof)
    objects[place] = change(objects[place])
    return pickle.dumps(objects)


def test_fast_stark_prove_batch_on_a_wide_trace(seeded):
    """16 registers at a FRI domain of 2^10 (the smallest shape of tests/test_gpu_wide_stark_columns.py: `prove` takes the column
    batches), 8 colinearity checks and 8 grinding bits: prove_batch equals prove member by member, and verify_batch rejects exactly
    the member whose nonce is altered -- or whose nonce is kept while one opened element BEHIND it is altered, which only device
    checks that read the shifted positions can tell"""
    import workloads
    from fast_stark import FastStark
    registers, s, bits = 16, 8, 8
    _, T, rows, packed, air, boundary = workloads.synthetic_wide_instance(10, registers, s)
    assert FastStark.COLUMN_BATCH_MIN <= registers
    stark = FastStark(field, 4, s, 2 * s + bits, registers, T, grinding_bits=bits)
    assert stark.fri_domain_length == 1 << 10 and stark.fri.grinding_bits == bits
    tz, tz_codeword, root = stark.preprocess()
    seeded(31)
    alone = [stark.prove([list(r) for r in rows], air, boundary, tz, tz_codeword) for _ in range(3)]
    seeded(31)
    proofs = stark.prove_batch([[list(r) for r in rows] for _ in range(3)], air, [boundary] * 3, tz, tz_codeword)
    assert proofs == alone and len(set(proofs)) == 3
    # the nonce of each proof: behind R + 1 roots, FRI's roots and the last codeword; the hashlib loop's over the stream in front of it
    found = [nonce_and_indices_in_a_stark_proof(stark.fri, proof, registers + 1, stream_of) for proof in proofs]
    assert len(set(nonce for nonce, _ in found)) == 3
    assert stark.verify(proofs[1], air, boundary, root) is True
    assert stark.verify_batch(proofs, air, [boundary] * 3, root) == [True] * 3
    k = nonce_place(proofs[1])
    bump = lambda element: FieldElement((element.value + 1) % field.p, field)
    objects = pickle.loads(proofs[1])
    assert type(objects[k + 1]) is tuple and len(objects[k + 1]) == 3 and type(objects[-2]) is FieldElement and type(objects[-1]) is list
    altered = [with_object(proofs[1], k, lambda nonce: nonce + 1),                                     # the nonce
               with_object(proofs[1], k, lambda nonce: found[1][1]),                                   # the next accepted nonce
               with_object(proofs[1], k + 1, lambda triple: (bump(triple[0]),) + triple[1:]),          # the first opened element behind it
               with_object(proofs[1], k + s, lambda triple: triple[:2] + (bump(triple[2]),)),          # the last triple of the first round
               with_object(proofs[1], len(objects) - 2, bump)]                                         # the last opened leaf of the proof
    for bad in altered:
        assert stark.verify_batch([proofs[0], bad, proofs[2]], air, [boundary] * 3, root) == [True, False, True]
    assert stark.verify(altered[1], air, boundary, root) is False and stark.verify(altered[2], air, boundary, root) is False


# ---- FastRPSSS ---------------------------------------------------------------------------------------------------------------------
def test_sign_batch_and_verify_batch_with_grinding(seeded):
    """FastRPSSS at 56 colinearity checks and 16 grinding bits: sign_batch of three documents equals three sign calls under the same
    seeded randomness; verify_batch accepts them and rejects exactly the one whose nonce is bumped"""
    from fast_rpsss import FastRPSSS, SignatureProofStream
    scheme = FastRPSSS(num_colinearity_checks=56, grinding_bits=16)
    sks = [scheme.field.sample(b"key %d of a ground batch" % k) for k in range(3)]
    pks = scheme.rp.hash_batch(sks)
    documents = [b"document %d" % k for k in range(3)]
    seeded(77)
    alone = [scheme.sign(sk, document) for sk, document in zip(sks, documents)]
    seeded(77)
    together = scheme.sign_batch(sks, documents)
    assert together == alone and len(set(together)) == 3
    def front_of(document):
        def front(objects):
            stream = SignatureProofStream(document)
            stream.objects = list(objects)
            return stream
        return front
    found = [nonce_and_indices_in_a_stark_proof(scheme.stark.fri, signature, scheme.rp.m + 1, front_of(document)) for document, signature in zip(documents, together)]
    assert len(set(nonce for nonce, _ in found)) == 3
    assert scheme.verify_batch(pks, documents, together) == [True] * 3
    assert [scheme.verify(pk, document, signature) for pk, document, signature in zip(pks, documents, together)] == [True] * 3
    for m in range(3):
        for other in (found[m][0] + 1, found[m][1]):                   # nonce + 1, the next accepted nonce
            bumped = list(together)
            bumped[m] = with_object(together[m], nonce_place(together[m]), lambda nonce: other)
            assert scheme.verify_batch(pks, documents, bumped) == [k != m for k in range(3)]


# ---- the sharded prover ------------------------------------------------------------------------------------------------------------
def test_sharded_fri_refuses_grinding_bits():
    from sharded_fri import ShardedFri
    with pytest.raises(AssertionError, match="sharded provers do not grind"):
        ShardedFri(make_fri(32, 2, 8), 4, 0, 1, None, engine=object())

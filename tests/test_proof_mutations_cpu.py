"""The enumerator of single changes (tests/proof_mutations.py) and the plain FRI verifier (tests/plain_fri_verifier.py) pinned against
each other without a GPU: both plain provers at n = 256, expansion 4, s = 3 -- five codewords of 256 .. 16 values, so FOUR queried
rounds: a first, two middle ones and a last -- with grinding_bits 0 and 4.  The verifier accepts the four honest proofs and rejects every
mutant of them; every object index has mutants; and the sweep reaches the rounds after round 0 with both kinds of query-phase check.

Which of `colinearity` and `merkle` a class of change can fail at all in a round after round 0 follows from the protocol, not from what
the verifier says, and is written down in LATER_ROUND_CHECKS:

    bit0, bit7last                  a path digest fails its path; a root r > 0 moves alpha_r, which fails round r's tests: both
    plus_one, swap_members          the values of a test and the leaves of its paths: both
    literal_p                       decimal leaves: p is the residue 0 and the string "p": both (pair leaves refuse it by shape)
    plus_p                          decimal leaves: the SAME residue, so the tests hold, under another decimal string: the paths alone
                                    (pair leaves refuse it by shape)
    drop_digest, append_digest,     decimal leaves: the path alone (pair leaves refuse the first two by shape)
    swap_digests
    drop_member, repeat_member,     a shape failure in the round the object belongs to: neither
    as_str

The table is asserted as an equality over failures(), which lists every failed check, not only the first."""
import functools
import pickle
from hashlib import blake2s

import pytest

import fri_pairs_cases as cases
import plain_fri_verifier as plain
import proof_mutations
from fri_pairs_cases import G, P
from proof_mutations import label_class, label_index, mutants

N, EXPANSION, S = 256, 4, 3
ROUNDS = 5
FORMS = [(pair_leaves, bits) for pair_leaves in (False, True) for bits in (0, 4)]
LATER_ROUND_CHECKS = {
    "bit0": {"colinearity", "merkle"}, "bit7last": {"colinearity", "merkle"},
    "plus_one": {"colinearity", "merkle"}, "swap_members": {"colinearity", "merkle"}, "literal_p": {"colinearity", "merkle"},
    "plus_p": {"merkle"}, "drop_digest": {"merkle"}, "append_digest": {"merkle"}, "swap_digests": {"merkle"},
    "drop_member": set(), "repeat_member": set(), "as_str": set(),
}


def object_count(pair_leaves, grinding_bits, rounds=ROUNDS, s=S):
    """the roots, the last codeword, the nonce if any; per queried round s pairs and s paths, or s triples and 3 s paths"""
    return rounds + 1 + (1 if grinding_bits else 0) + (2 if pair_leaves else 4) * s * (rounds - 1)


def honest_proof(pair_leaves, grinding_bits, document=None):
    """the plain prover's proof as bytes; the stream is ip.ProofStream's, whose Fiat-Shamir step is the protocol's"""
    from algebra import Field, FieldElement
    from ip import ProofStream
    field = Field.main()

    class Bound(ProofStream):
        def prover_fiat_shamir(self, num_bytes=32):
            from hashlib import shake_256
            return shake_256(blake2s(bytes(document)).digest() + self.serialize()).digest(num_bytes)

    stream = ProofStream() if document is None else Bound()
    prove = cases.prove if pair_leaves else plain.prove_decimal
    prove(cases.codeword(N, EXPANSION), G, cases.root_of_unity(N), EXPANSION, S, stream, lambda v: FieldElement(v, field), grinding_bits)
    return stream.serialize()


def plain_verdict(proof, pair_leaves, grinding_bits, prefix=b""):
    return plain.verify(pickle.loads(proof), N, EXPANSION, S, G, cases.root_of_unity(N), pair_leaves, grinding_bits, prefix)


@functools.lru_cache(maxsize=None)
def sweep(pair_leaves, grinding_bits):
    """(the honest objects, [(label, the mutant as a proof, (verdict, reason), failures)]), computed once; callers leave it unchanged"""
    objects = pickle.loads(honest_proof(pair_leaves, grinding_bits))
    rows = []
    for label, changed in mutants(objects):
        proof = pickle.dumps(changed)
        found = plain.failures(pickle.loads(proof), N, EXPANSION, S, G, cases.root_of_unity(N), pair_leaves, grinding_bits)
        rows.append((label, proof, plain_verdict(proof, pair_leaves, grinding_bits), found))
    return objects, rows


@pytest.mark.parametrize("pair_leaves,grinding_bits", FORMS)
def test_object_count(pair_leaves, grinding_bits):
    assert cases.num_rounds(N, EXPANSION, S) == ROUNDS
    objects = pickle.loads(honest_proof(pair_leaves, grinding_bits))
    assert len(objects) == object_count(pair_leaves, grinding_bits)
    assert len(objects) == {(False, 0): 54, (False, 4): 55, (True, 0): 30, (True, 4): 31}[(pair_leaves, grinding_bits)]
    assert len(objects[ROUNDS]) == N >> (ROUNDS - 1) == 16


@pytest.mark.parametrize("pair_leaves,grinding_bits", FORMS)
def test_honest_accepted_every_mutant_rejected(pair_leaves, grinding_bits):
    proof = honest_proof(pair_leaves, grinding_bits)
    assert plain_verdict(proof, pair_leaves, grinding_bits) == (True, None)
    objects, rows = sweep(pair_leaves, grinding_bits)
    accepted = [label for label, _, (verdict, _), _ in rows if verdict is not False]
    assert accepted == []
    assert all(reason in plain.REASONS for _, _, (_, reason), _ in rows)
    # the honest proof of the other form, and of the other bit count, is no proof here
    assert plain_verdict(honest_proof(not pair_leaves, grinding_bits), pair_leaves, grinding_bits)[0] is False
    assert plain_verdict(honest_proof(pair_leaves, 4 - grinding_bits), pair_leaves, grinding_bits)[0] is False


def test_document_bound_transcript():
    """a proof made under a document's prefix verifies under that prefix and under no other"""
    for pair_leaves in (False, True):
        proof = honest_proof(pair_leaves, 4, b"a document")
        assert plain_verdict(proof, pair_leaves, 4, blake2s(b"a document").digest()) == (True, None)
        assert plain_verdict(proof, pair_leaves, 4, blake2s(b"another document").digest())[0] is False
        assert plain_verdict(proof, pair_leaves, 4)[0] is False


@pytest.mark.parametrize("pair_leaves,grinding_bits", FORMS)
def test_every_object_has_mutants_of_one_change(pair_leaves, grinding_bits):
    objects, rows = sweep(pair_leaves, grinding_bits)
    before = [pickle.dumps(o) for o in objects]
    assert {label_index(label) for label, _, _, _ in rows} == set(range(len(objects)))
    assert len({label for label, _, _, _ in rows}) == len(rows)
    # a digest, the object with the fewest: two flips, as_str, delete, and where objects follow duplicate and truncate
    per_index = [sum(1 for label, _, _, _ in rows if label_index(label) == i) for i in range(len(objects))]
    assert min(per_index) >= 6
    for label, proof, _, _ in rows:
        i, name = label_index(label), label_class(label)
        after = [pickle.dumps(o) for o in pickle.loads(proof)]
        assert after != before, label
        if name in proof_mutations.VALUE_CLASSES:
            assert len(after) == len(before) and [k for k in range(len(before)) if after[k] != before[k]] == [i], label
        elif name == "delete":
            assert after == before[:i] + before[i + 1:], label
        elif name == "duplicate":
            assert after == before[:i + 1] + before[i:] and i + 1 < len(before), label
        elif name == "exchange":
            assert after == before[:i] + [before[i + 1], before[i]] + before[i + 2:], label
        else:
            assert name == "truncate" and after == before[:i + 1] and i + 1 < len(before), label
    assert [pickle.dumps(o) for o in objects] == before            # the enumerator left its input alone
    assert not any(label_class(label) == "duplicate" and label_index(label) == len(objects) - 1 for label, _, _, _ in rows)
    # the thinned sweep drops the middle places and nothing else
    thin = {label for label, _ in mutants(objects, thin=True)}
    full = {label for label, _, _, _ in rows}
    assert thin < full and {label_index(label) for label in thin} == set(range(len(objects)))
    assert {label_class(label) for label in thin} == {label_class(label) for label in full}


def test_an_unknown_object_is_an_error():
    objects = pickle.loads(honest_proof(True, 0))
    for stranger in (3.5, None, [], ["a string"], [objects[0], objects[ROUNDS][0]], {"a": 1}, True):
        with pytest.raises(TypeError):
            list(mutants(objects[:2] + [stranger] + objects[2:]))


def test_classes_reach_the_later_rounds():
    """per class of value change: the query-phase checks that fail in some round after round 0, over the four proofs together, are
    exactly those of LATER_ROUND_CHECKS -- and they are met in the middle rounds and in the last queried round"""
    reached, rounds_met = {}, {}
    for pair_leaves, grinding_bits in FORMS:
        _, rows = sweep(pair_leaves, grinding_bits)
        for label, _, _, found in rows:
            name = label_class(label)
            if name not in LATER_ROUND_CHECKS:
                continue
            for reason, r in found:
                if r is not None and r > 0:
                    rounds_met.setdefault(name, set()).add(r)
                    if reason in ("colinearity", "merkle"):
                        reached.setdefault(name, set()).add(reason)
    for name, expected in LATER_ROUND_CHECKS.items():
        assert reached.get(name, set()) == expected, name
        assert rounds_met[name] == {1, 2, 3}, name
    assert set(LATER_ROUND_CHECKS) == set(proof_mutations.VALUE_CLASSES) - set(proof_mutations.NONCE_CLASSES)


def test_first_reasons():
    """every reason is some mutant's first reason, and the nonce's mutants fail the proof of work or, where the changed nonce happens to
    be accepted (one in sixteen), the query phase it re-samples"""
    seen = set()
    for pair_leaves, grinding_bits in FORMS:
        _, rows = sweep(pair_leaves, grinding_bits)
        seen |= {reason for _, _, (_, reason), _ in rows}
        for label, _, (_, reason), _ in rows:
            if label_class(label) in ("nonce_2_64", "nonce_as_element"):
                assert reason == "proof of work", label
            elif label_class(label) in proof_mutations.NONCE_CLASSES:
                assert reason in ("proof of work", "colinearity", "merkle"), label
    assert seen == set(plain.REASONS) - {"degree"}
    # `degree` needs a last codeword that is committed yet not of low degree: a prover that folds a codeword of full degree
    from algebra import Field, FieldElement
    from ip import ProofStream
    import random
    field, rng, stream = Field.main(), random.Random(1), ProofStream()
    cases.prove([rng.randrange(P) for _ in range(N)], G, cases.root_of_unity(N), EXPANSION, S, stream, lambda v: FieldElement(v, field))
    assert plain_verdict(stream.serialize(), True, 0) == (False, "degree")

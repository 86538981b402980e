"""Proofs with a proof of work in them (Fri / FastStark / FastRPSSS with grinding_bits > 0) on the GPU: the nonce on the stream is the
smallest one the hashlib loop accepts, the indices come from the transcript with it, every prover route writes the same bytes, an
altered nonce is rejected, and at grinding_bits = 0 the bytes are the golden ones."""
import hashlib
import pickle

import pytest

from conftest import load_golden
import synth

pytestmark = pytest.mark.gpu

N, S = 32, 2                      # the smallest domain at which Fri(expansion factor 4, 2 tests) has two rounds


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


@pytest.fixture(scope="module")
def field(sc):
    from algebra import Field
    return Field.main()


def codeword(field, seed, n=N):
    from algebra import FieldElement
    from ntt import fast_coset_evaluate_device
    from univariate import Polynomial
    return fast_coset_evaluate_device(Polynomial([FieldElement(v, field) for v in synth.synth_ints(seed, n // 4)]), field.generator(), field.primitive_nth_root(n), n)


def make_fri(field, bits, n=N, s=S):
    from fri import Fri
    return Fri(field.generator(), field.primitive_nth_root(n), n, 4, s, grinding_bits=bits)


def stream_of(objects):
    from ip import ProofStream
    ps = ProofStream()
    ps.objects = list(objects)
    return ps


@pytest.mark.parametrize("bits", [8, 16])
def test_fri_prove_pushes_the_smallest_nonce(field, bits):
    import grinding
    from ip import ProofStream
    fri = make_fri(field, bits)
    rounds = fri.num_rounds()
    assert rounds == 2
    ps = ProofStream()
    top = fri.prove(codeword(field, 5), ps)
    objects = list(ps.objects)
    nonce = objects[rounds + 1]                         # behind the roots and the last codeword
    seed = stream_of(objects[:rounds + 1]).prover_fiat_shamir()
    assert type(nonce) is int and nonce == grinding.grind_host(seed, bits)
    assert top == fri.sample_indices(stream_of(objects[:rounds + 2]).prover_fiat_shamir(), N // 2, N >> (rounds - 1), S)
    assert len(objects) == rounds + 2 + 4 * S * (rounds - 1)
    assert fri.verify(ps, []) is True
    assert fri.verify(stream_of(pickle.loads(ps.serialize())), []) is True
    assert fri.verify_batch([stream_of(objects)], [[]]) == [True]
    # another accepted nonce moves the indices (the openings no longer answer them); a nonce that is not accepted fails at once
    following = grinding.grind_host(seed, bits, nonce + 1)
    for other in (following, nonce + 1):
        altered = objects[:rounds + 1] + [other] + objects[rounds + 2:]
        assert fri.verify(stream_of(altered), []) is False
        assert fri.verify_batch([stream_of(altered), stream_of(objects)], [[], []]) == [False, True]
    # a Fri without grinding does not take the proof (it reads the nonce as a triple), nor the other way round
    assert make_fri(field, 0).verify_batch([stream_of(objects)], [[]]) == [False]
    plain = ProofStream()
    make_fri(field, 0).prove(codeword(field, 5), plain)
    assert fri.verify_batch([stream_of(list(plain.objects))], [[]]) == [False]


@pytest.mark.parametrize("bits", [8, 16])
def test_every_route_writes_the_same_bytes(field, monkeypatch, bits):
    from fri import Fri
    from ip import ProofStream
    fri = make_fri(field, bits)
    taken = []
    real = Fri._prove_in_library

    def watched(self, *args):
        result = real(self, *args)
        taken.append(result is not None)
        return result
    monkeypatch.setattr(Fri, "_prove_in_library", watched)
    in_library, by_phases = ProofStream(), ProofStream()
    top = fri.prove(codeword(field, 7), in_library)                     # a device codeword: one library call, the search inside it
    assert fri.prove(codeword(field, 7).tolist(), by_phases) == top     # a list: phase by phase, the search between commit and sampling
    assert taken == [True, False]
    assert in_library.serialize() == by_phases.serialize()
    # three members in one batch (the searches ride one grid) against three calls
    members = [codeword(field, 7 + 10 * k) for k in range(3)]
    alone = [ProofStream() for _ in members]
    tops = [fri.prove(codeword(field, 7 + 10 * k), stream) for k, stream in enumerate(alone)]
    together = [ProofStream() for _ in members]
    assert fri.prove_batch(members, together) == tops
    assert [s.serialize() for s in together] == [s.serialize() for s in alone]
    assert together[0].serialize() == in_library.serialize() and len(set(s.serialize() for s in together)) == 3
    assert fri.verify_batch(together, [[] for _ in together]) == [True] * 3


def test_zero_bits_is_the_golden_proof(field):
    """Fri(..., grinding_bits=0) writes the bytes recorded before grinding existed (tests/golden/fri.json, as tests/test_gpu_host.py reads it)"""
    from ip import ProofStream
    rec = min(load_golden("fri.json")["prove_synth"], key=lambda r: r["logN"])
    n = 1 << rec["logN"]
    cw = codeword(field, rec["coeff_seed"], n)
    assert hashlib.sha256(cw.vec.to_bytes()).hexdigest() == rec["codeword_sha256"]
    from fri import Fri
    fri = Fri(field.generator(), field.primitive_nth_root(n), n, rec["expansion_factor"], rec["num_colinearity_tests"], grinding_bits=0)
    ps = ProofStream()
    assert fri.prove(cw, ps) == rec["top_level_indices"]
    ser = ps.serialize()
    assert len(ps.objects) == rec["num_objects"] and hashlib.sha256(ser).hexdigest() == rec["serialized_sha256"]


def nonce_places(proof):
    return [k for k, o in enumerate(pickle.loads(proof)) if type(o) is int]


def with_nonce_plus_one(proof):
    objects = pickle.loads(proof)
    (k,) = nonce_places(proof)
    objects[k] += 1
    return pickle.dumps(objects)


def test_fast_stark_round_trips(sc):
    """FastStark at 4 colinearity checks and 8 grinding bits for a security level of 16 (2 * 4 + 8): prove / verify, prove_batch /
    verify_batch, and verify_batch's verdicts when one member's nonce is altered"""
    import workloads
    from algebra import FieldElement
    from fast_stark import FastStark
    s, bits = 4, 8
    field, T, _, air, boundary = workloads.synthetic_stark_instance(9, s)
    col_a, col_b = synth.synthetic_air_columns(T)
    rows = [[FieldElement(a, field), FieldElement(b, field)] for a, b in zip(col_a, col_b)]
    stark = FastStark(field, 4, s, 16, 2, T, grinding_bits=bits)
    assert stark.fri_domain_length == 1 << 9 and stark.num_randomizers == 4 * s and stark.fri.num_rounds() >= 2
    zerofier, zerofier_codeword, root = stark.preprocess()
    proof = stark.prove([list(r) for r in rows], air, boundary, zerofier, zerofier_codeword)
    assert len(nonce_places(proof)) == 1
    assert stark.verify(proof, air, boundary, root) is True
    assert stark.verify(with_nonce_plus_one(proof), air, boundary, root) is False
    proofs = stark.prove_batch([[list(r) for r in rows] for _ in range(3)], air, [boundary] * 3, zerofier, zerofier_codeword)
    assert all(len(nonce_places(p)) == 1 for p in proofs)
    assert [stark.verify(p, air, boundary, root) for p in proofs] == [True] * 3
    assert stark.verify_batch(proofs, air, [boundary] * 3, root) == [True] * 3
    assert stark.verify_batch([proofs[0], with_nonce_plus_one(proofs[1]), proofs[2]], air, [boundary] * 3, root) == [True, False, True]
    # the same parameters without the proof of work do not reach the security level
    with pytest.raises(AssertionError):
        FastStark(field, 4, s, 16, 2, T)


def test_signature_with_grinding(sc):
    """FastRPSSS at 56 colinearity checks and 16 grinding bits (2 * 56 + 16 = 128): one document signed and verified"""
    from fast_rpsss import FastRPSSS
    scheme = FastRPSSS(num_colinearity_checks=56, grinding_bits=16)
    assert scheme.stark.num_colinearity_checks == 56 and scheme.stark.fri.grinding_bits == 16 and scheme.stark.num_randomizers == 224
    sk = scheme.field.sample(b"a key for a ground signature")
    pk = scheme.rp.hash(sk)
    signature = scheme.sign(sk, b"a document")
    assert len(nonce_places(signature)) == 1
    assert scheme.verify(pk, b"a document", signature) is True
    assert scheme.verify(pk, b"another document", signature) is False
    assert scheme.verify(pk, b"a document", with_nonce_plus_one(signature)) is False
    assert scheme.verify_batch([pk, pk], [b"a document"] * 2, [signature, with_nonce_plus_one(signature)]) == [True, False]

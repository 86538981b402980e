"""Fri.verify's complete observable behaviour, pinned without a GPU: over every single change (tests/proof_mutations.py) of the plain
provers' proofs at n = 256, expansion 4, s = 3 -- five codewords, four queried rounds -- in both leaf forms and with grinding_bits 0 and
4, what `verify` returns or raises, every line it prints, the `polynomial_values` it leaves and how far it read the stream.  The two
device steps of the last codeword are answered by the plain verifier's host versions (the decimal tree's root, the interpolant's
degree), as tests/test_grind_cpu.py::fri_by_hand answers them by hand; everything else is the library's own walk.

The verdict (an exception is a rejection) must be the plain verifier's on every mutant, and the digest over the per-mutant records is
a constant: a change to the verifier's walk that moves a verdict, a printed line, an exception's kind, the reported values or the read
position of ANY mutant moves it.  The constants were taken before the verifiers of fri.py became one walk, and hold after it."""
import hashlib
import pickle

import pytest

import fri_pairs_cases as cases
import plain_fri_verifier as plain
from fri_pairs_cases import G
from proof_mutations import mutants

N, EXPANSION, S = 256, 4, 3
DIGESTS = {
    (False, 0): "aca059a351fba7c52d6d66673c0bfac2f11e012edb282b082819a00eaf79fa1c",
    (False, 4): "6ba78c2090f4c039b075f5f0299733cd1bbae3b2c58308baade53fe05a12cc98",
    (True, 0): "312269b572d23e14a1ada90b67746a245e2e39fcaf121b565304202e36c153ca",
    (True, 4): "b49ed6f4b65891b3d60093443caaf71612642fff1a667921c0cb211cf8e4ec6c",
}
MUTANTS = {(False, 0): (729, 206), (False, 4): (735, 206), (True, 0): (370, 35), (True, 4): (376, 36)}      # (mutants, of them raising)


@pytest.fixture()
def host_fri(monkeypatch):
    """make(pair_leaves, grinding_bits) -> a Fri on the cases' domain whose last-codeword checks need no device"""
    import fri as fri_module
    from algebra import Field, FieldElement
    field = Field.main()
    monkeypatch.setattr(fri_module.Merkle, "commit", lambda values: plain.decimal_levels([v.value for v in values])[-1][0])
    monkeypatch.setattr(fri_module.Fri, "_last_codeword_degree",
                        lambda self, values, omega, offset: plain._degree([v.value for v in values], omega.value))

    def make(pair_leaves, grinding_bits):
        return fri_module.Fri(FieldElement(G, field), FieldElement(cases.root_of_unity(N), field), N, EXPANSION, S,
                              grinding_bits=grinding_bits, pair_leaves=pair_leaves)
    return make


def honest_objects(pair_leaves, grinding_bits):
    from algebra import Field, FieldElement
    from ip import ProofStream
    field, stream = Field.main(), ProofStream()
    prove = cases.prove if pair_leaves else plain.prove_decimal
    prove(cases.codeword(N, EXPANSION), G, cases.root_of_unity(N), EXPANSION, S, stream, lambda v: FieldElement(v, field), grinding_bits)
    return pickle.loads(stream.serialize())


def observe(fri, objects, capsys):
    """(True / False / the exception's class name, the printed lines, polynomial_values as (index, value), the stream's read_index)"""
    from ip import ProofStream
    stream, values = ProofStream(), []
    stream.objects = list(objects)
    try:
        outcome = fri.verify(stream, values)
        assert outcome is True or outcome is False
    except Exception as error:
        outcome = type(error).__name__
    printed = capsys.readouterr().out.splitlines()
    return outcome, printed, [(index, getattr(value, "value", value)) for index, value in values], stream.read_index


@pytest.mark.parametrize("pair_leaves,grinding_bits", sorted(DIGESTS))
def test_verify_is_pinned_on_every_mutant(host_fri, capsys, pair_leaves, grinding_bits):
    fri = host_fri(pair_leaves, grinding_bits)
    omega = cases.root_of_unity(N)
    objects = honest_objects(pair_leaves, grinding_bits)
    outcome, printed, values, read_index = observe(fri, objects, capsys)
    assert outcome is True and printed == [] and read_index == len(objects)
    assert len(values) == 2 * S == 6
    record, accepted, disagreeing, raising = hashlib.sha256(), [], [], 0
    count = 0
    for label, changed in mutants(objects):
        count += 1
        observed = observe(fri, changed, capsys)
        if observed[0] is True:
            accepted.append(label)
        if (observed[0] is True) != plain.verify(changed, N, EXPANSION, S, G, omega, pair_leaves, grinding_bits)[0]:
            disagreeing.append(label)
        raising += type(observed[0]) is str
        record.update(repr((label,) + observed).encode())
    print("mutants %d, raising %d, digest %s" % (count, raising, record.hexdigest()))
    assert (count, raising) == MUTANTS[(pair_leaves, grinding_bits)]
    assert accepted == []
    assert disagreeing == []
    assert record.hexdigest() == DIGESTS[(pair_leaves, grinding_bits)]

"""FastRPSSS.sign_batch at the signature scheme's own shape (284 trace rows, FRI 2^12, 64 colinearity checks): with the seed of the
reference's golden run (tests/golden/rpsss.json) and its key draws made first, two signatures in one call -- the golden key and
document as member 0 -- are the two of sequential `sign` calls, member 0's is the reference's, and both pass verify_batch."""
import hashlib
import os
import random

import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


from fast_rpsss import FastRPSSS, SignatureProofStream     # noqa: E402


@pytest.fixture(scope="module")
def rpsss():
    return FastRPSSS()


def keys_then(rpsss, g, monkeypatch, sign):
    """the golden run's stream: its key draws first, then whatever `sign` draws"""
    rng = random.Random(g["seed"])
    monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    pairs = [rpsss.keygen() for _ in range(len(g["keys"]))]
    assert [[str(sk.value), str(pk.value)] for sk, pk in pairs] == g["keys"]
    return pairs, sign(pairs)


def test_two_signatures_are_the_sequential_ones_and_member_0_is_the_reference(rpsss, monkeypatch):
    g = load_golden("rpsss.json")
    documents = [g["document"].encode(), b"a second document, signed with the second key"]
    members = [g["signed_key"], 1]
    pairs, together = keys_then(rpsss, g, monkeypatch, lambda pairs: rpsss.sign_batch([pairs[k][0] for k in members], documents))
    _, one_by_one = keys_then(rpsss, g, monkeypatch, lambda pairs: [rpsss.sign(pairs[k][0], document) for k, document in zip(members, documents)])
    assert len(together) == 2 and together[0] != together[1]
    assert len(together[0]) == g["signature_len"] and hashlib.sha256(together[0]).hexdigest() == g["signature_sha256"]
    assert together[0] == one_by_one[0] and together[1] == one_by_one[1]
    assert rpsss.verify_batch([pairs[k][1] for k in members], documents, together) == [True, True]
    assert rpsss.verify_batch([pairs[k][1] for k in members], documents[::-1], together) == [False, False]


def test_stark_prove_batch_takes_the_callers_streams(rpsss, monkeypatch):
    g = load_golden("rpsss.json")
    document = g["document"].encode()
    stream = SignatureProofStream(document)
    _, proofs = keys_then(rpsss, g, monkeypatch, lambda pairs: rpsss.stark_prove_batch([pairs[g["signed_key"]][0]], [stream]))
    assert len(proofs) == 1 and proofs[0] == stream.serialize()
    assert hashlib.sha256(proofs[0]).hexdigest() == g["signature_sha256"]


def test_empty_batch_and_lengths(rpsss):
    assert rpsss.sign_batch([], []) == []
    assert rpsss.stark_prove_batch([], []) == []
    with pytest.raises(AssertionError):
        rpsss.sign_batch([rpsss.field.one()], [])
    with pytest.raises(AssertionError):
        rpsss.stark_prove_batch([rpsss.field.one()], [])

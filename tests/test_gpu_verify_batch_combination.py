"""FastStark.verify_batch with the combination at the opened points checked on the device (BatchChecks.combination,
sc_stark_combination_batch) against FastStark.verify: honest proofs of the synthetic AIR, a wide AIR and FastRPSSS signatures; inputs
on which ONLY the combination can fail (every Merkle path and colinearity test still passes); a bad member among good ones; the row
counter with the switch on and off; a leaf that is not a canonical residue."""
import pickle
import random

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import starkcore as sc                             # noqa: E402
import fast_stark                                  # noqa: E402
import fri                                         # noqa: E402
import workloads                                   # noqa: E402
from fast_stark import DeviceTrace, FastStark      # noqa: E402
from algebra import Field, FieldElement            # noqa: E402
from multivariate import MPolynomial               # noqa: E402

P = Field.P_MAIN
S = 16                                             # colinearity tests: 2 S opened points per proof


def host_verdict(fn, *args):
    try:
        return fn(*args) == True          # noqa: E712
    except Exception:
        return False


@pytest.fixture
def watched(monkeypatch):
    """the BatchChecks of every verify_batch call, and whether any Merkle or colinearity row failed on the device"""
    seen = {"checks": [], "other_rows_failed": False}

    class Watched(fri.BatchChecks):
        def __init__(self, count):
            fri.BatchChecks.__init__(self, count)
            seen["checks"].append(self)

    merkle_batch, colinearity_batch = sc.merkle_verify_batch, sc.colinearity_batch

    def spy(batch):
        def run(rows, *a):
            out = batch(rows, *a)
            seen["other_rows_failed"] |= bool((out != 1).any())
            return out
        return run

    monkeypatch.setattr(fast_stark, "BatchChecks", Watched)
    monkeypatch.setattr(sc, "merkle_verify_batch", spy(merkle_batch))
    monkeypatch.setattr(sc, "colinearity_batch", spy(colinearity_batch))
    return seen


def device_rows(seen):
    return sum(checks.combination_device_rows for checks in seen["checks"])


def seeded(seed):
    rng = random.Random(seed)
    return lambda k: bytes(rng.getrandbits(8) for _ in range(k))


@pytest.fixture(scope="module")
def synthetic():
    field, T, packed, air, boundary = workloads.synthetic_stark_instance(12, S)
    stark = FastStark(field, 4, S, 2 * S, 2, T)
    tz, committed, tz_root = stark.preprocess(device_resident=True)
    genuine = fast_stark.os.urandom
    try:
        fast_stark.os.urandom = seeded(12)
        proofs = [stark.prove(DeviceTrace.from_packed(packed, field), air, boundary, tz, committed) for _ in range(3)]
    finally:
        fast_stark.os.urandom = genuine
    return stark, air, boundary, tz_root, proofs


@pytest.fixture(scope="module")
def wide():
    field, T, rows, packed, air, boundary = workloads.synthetic_wide_instance(12, 5, S)
    stark = FastStark(field, 4, S, 2 * S, 5, T)
    tz, committed, tz_root = stark.preprocess(device_resident=True)
    proofs = [stark.prove(DeviceTrace.from_packed(packed, field), air, boundary, tz, committed) for _ in range(2)]
    return stark, air, boundary, tz_root, proofs


@pytest.fixture(scope="module")
def signed():
    from fast_rpsss import FastRPSSS
    scheme = FastRPSSS()
    field = scheme.field
    sks = [field.sample(b"key %d" % k) for k in range(2)]
    pks = [scheme.rp.hash(sk) for sk in sks]
    documents = [b"document %d" % k for k in range(2)]
    return scheme, pks, documents, scheme.sign_batch(sks, documents)


@pytest.mark.parametrize("instance", ["synthetic", "wide"])
def test_honest_proofs_match_verify_and_every_point_is_a_device_row(request, watched, instance):
    stark, air, boundary, tz_root, proofs = request.getfixturevalue(instance)
    want = [host_verdict(stark.verify, p, air, boundary, tz_root) for p in proofs]
    assert want == [True] * len(proofs)
    assert stark.verify_batch(proofs, air, [boundary] * len(proofs), tz_root) == want
    assert device_rows(watched) == 2 * S * len(proofs) and len(watched["checks"][-1].combinations) == 1


def test_honest_signatures_match_verify_and_every_point_is_a_device_row(watched, signed):
    scheme, pks, documents, signatures = signed
    want = [scheme.verify(pk, d, s) for pk, d, s in zip(pks, documents, signatures)]
    assert want == [True, True]
    assert scheme.verify_batch(pks, documents, signatures) == want
    assert device_rows(watched) == 2 * scheme.stark.num_colinearity_checks * 2


def test_generic_constraints_give_the_same_verdicts(watched, signed):
    """the same AIR as plain MPolynomials (no hand-written evaluator): the device rows are the same"""
    scheme, pks, documents, signatures = signed
    air = [MPolynomial(dict(a.dictionary)) for a in scheme.rp.transition_constraints(scheme.stark.omicron)]
    boundaries = [scheme.rp.boundary_constraints(pk) for pk in pks]
    from fast_rpsss import SignatureProofStream
    streams = [SignatureProofStream(d) for d in documents]
    assert scheme.stark.verify_batch(signatures, air, boundaries, scheme.transition_zerofier_root, streams) == [True, True]
    assert device_rows(watched) == 2 * scheme.stark.num_colinearity_checks * 2


def test_only_the_combination_rejects_a_boundary_with_another_value(watched, synthetic):
    stark, air, boundary, tz_root, proofs = synthetic
    field = Field.main()
    for k in range(len(boundary)):
        wrong = [(c, r, v + field.one()) if j == k else (c, r, v) for j, (c, r, v) in enumerate(boundary)]
        assert host_verdict(stark.verify, proofs[0], air, wrong, tz_root) is False
        # one bad member must not move the others
        assert stark.verify_batch(proofs, air, [boundary, wrong, boundary], tz_root) == [True, False, True]
    assert not watched["other_rows_failed"]
    assert device_rows(watched) == len(boundary) * 2 * S * 3


@pytest.mark.parametrize("instance", ["synthetic", "wide"])
def test_only_the_combination_rejects_constraints_with_one_coefficient_changed(request, watched, instance):
    stark, air, boundary, tz_root, proofs = request.getfixturevalue(instance)
    field = Field.main()
    changed = list(air)
    dictionary = dict(air[-1].dictionary)
    key = next(iter(dictionary))
    dictionary[key] = dictionary[key] + field.one()
    changed[-1] = MPolynomial(dictionary)
    assert stark.max_degree(changed) == stark.max_degree(air)
    want = [host_verdict(stark.verify, p, changed, boundary, tz_root) for p in proofs]
    assert want == [False] * len(proofs)
    assert stark.verify_batch(proofs, changed, [boundary] * len(proofs), tz_root) == want
    assert not watched["other_rows_failed"] and device_rows(watched) == 2 * S * len(proofs)


def test_only_the_combination_rejects_another_members_proof(watched, signed):
    scheme, pks, documents, signatures = signed
    # member 1's signature of member 0's document under member 0's public key: the stream is bound to the document, so sign it anew
    other = scheme.sign_batch([scheme.field.sample(b"key 1")], [documents[0]])[0]
    assert scheme.verify(pks[1], documents[0], other) is True
    assert scheme.verify(pks[0], documents[0], other) is False
    assert scheme.verify_batch([pks[0], pks[0], pks[1]], [documents[0], documents[0], documents[1]], [signatures[0], other, signatures[1]]) == [True, False, True]
    assert not watched["other_rows_failed"]


def test_switch_off_runs_the_host_loop_with_the_same_verdicts(watched, synthetic, monkeypatch):
    stark, air, boundary, tz_root, proofs = synthetic
    field = Field.main()
    wrong = [(c, r, v + field.one()) if j == 0 else (c, r, v) for j, (c, r, v) in enumerate(boundary)]
    objects = pickle.loads(proofs[2])
    objects[-2] = objects[-2] + field.one()
    cases = [(proofs[0], boundary), (proofs[1], wrong), (pickle.dumps(objects), boundary), (proofs[2], boundary)]
    want = [host_verdict(stark.verify, p, air, b, tz_root) for p, b in cases]
    assert want == [True, False, False, True]
    run = lambda: stark.verify_batch([p for p, _ in cases], air, [b for _, b in cases], tz_root)
    assert run() == want
    assert device_rows(watched) == 2 * S * len(cases)
    monkeypatch.setattr(FastStark, "COMBINATION_ON_DEVICE", False)
    assert run() == want
    assert watched["checks"][-1].combination_device_rows == 0 and not watched["checks"][-1].combinations
    monkeypatch.setattr(FastStark, "COMBINATION_ON_DEVICE", True)
    monkeypatch.setattr(FastStark, "COMBINATION_DEVICE_MIN_ROWS", 2 * S * len(cases) + 1)        # one row short of the threshold: the host loop
    assert run() == want
    assert watched["checks"][-1].combination_device_rows == 0
    monkeypatch.setattr(FastStark, "COMBINATION_DEVICE_MIN_ROWS", 2 * S * len(cases))
    assert run() == want
    assert watched["checks"][-1].combination_device_rows == 2 * S * len(cases)


def test_a_leaf_that_is_no_canonical_residue_takes_the_host_path(watched, synthetic):
    stark, air, boundary, tz_root, proofs = synthetic
    field = Field.main()
    objects = pickle.loads(proofs[0])
    # the last opening of the last boundary quotient's codeword (behind it: 4 S openings each of the randomizer's and the transition
    # zerofier's, a leaf and a path each); its position is an opened point or a successor, so one or two rows read the leaf
    leaf_at = len(objects) - 2 - 2 * 2 * 4 * S
    same = list(objects)
    same[leaf_at] = FieldElement(objects[leaf_at].value + P, field)       # the same residue, not canonical
    other = list(objects)
    other[leaf_at] = FieldElement(-1, field)
    for changed in (same, other):
        proof = pickle.dumps(changed)
        want = host_verdict(stark.verify, proof, air, boundary, tz_root)
        assert stark.verify_batch([proof, proofs[1]], air, [boundary] * 2, tz_root) == [want, True]
        checks = watched["checks"][-1]
        group = next(iter(checks.combinations.values()))
        assert 1 <= len(group.host_only) <= 2 and checks.combination_device_rows == 2 * 2 * S - len(group.host_only)

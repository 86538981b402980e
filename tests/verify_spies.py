"""What the tests of the batched verifiers share: the verdict of a host verifier that may raise, and the spies that count what a
verify_batch call sent to the device and what fell back to the host (tests/test_gpu_verify_batch.py, tests/test_gpu_proof_mutations.py).
A test module imports the fixtures by name."""
import pytest


def host_verdict(fn, *args):
    try:
        return fn(*args) == True          # noqa: E712  (the verifiers return bools; anything else is not an acceptance)
    except Exception:
        return False


@pytest.fixture
def row_counts(monkeypatch):
    """rows each device entry received, UNDECIDED colinearity verdicts, and calls of the host functions rows fall back to"""
    import fri
    import starkcore as sc
    counts = {"merkle": 0, "colinearity": 0, "undecided": 0, "host_merkle": 0, "host_colinearity": 0}
    merkle_batch, colinearity_batch = sc.merkle_verify_batch, sc.colinearity_batch
    host_merkle, host_colinearity = fri.Merkle.verify, fri.test_colinearity

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
    monkeypatch.setattr(fri.Merkle, "verify", staticmethod(spy_host_merkle))
    monkeypatch.setattr(fri, "test_colinearity", spy_host_colinearity)
    return counts


@pytest.fixture
def combination_hosts(monkeypatch):
    """the BatchChecks of every FastStark.verify_batch call, and the owners (members of the batch) for which the host decided an opened
    point of the combination (the `holds` of FastStark._walk, which every row carries for the case that the device cannot
    hold or decide it), one entry per call"""
    import fast_stark
    import fri
    seen = {"checks": [], "host_owners": []}

    class Watched(fri.BatchChecks):
        def __init__(self, count):
            fri.BatchChecks.__init__(self, count)
            seen["checks"].append(self)

        def combination(self, owner, group, member, index, claimed, randomizer, zerofier, current, following, host):
            def counted():
                seen["host_owners"].append(owner)
                return host()
            fri.BatchChecks.combination(self, owner, group, member, index, claimed, randomizer, zerofier, current, following, counted)

    monkeypatch.setattr(fast_stark, "BatchChecks", Watched)
    return seen

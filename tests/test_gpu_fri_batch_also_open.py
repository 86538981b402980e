"""Fri.prove_batch(..., also_open=AlsoOpenForests(...)): committed codewords in forests of their own -- one with two trees per member,
one over a single codeword that all members share -- opened at each member's positions in the launch that fetches the FRI openings.
The streams and indices are those of prove_batch without the keyword and of K calls of prove; the answers are those of a separate
MerkleForest.query and pass Merkle.verify; one sc_merkle_forest_query_dev per chunk, also when FOREST_MAX_LEAVES splits the batch;
the member-by-member fallback fills the answers; the argument errors come before any work."""
import pytest

import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import starkcore as sc                             # noqa: E402
from algebra import Field, FieldElement            # noqa: E402
from fast_rpsss import SignatureProofStream        # noqa: E402
from fri import AlsoOpenForests, Fri               # noqa: E402
from ip import ProofStream                         # noqa: E402
from merkle import Merkle                          # noqa: E402
from ntt import fast_coset_evaluate_device         # noqa: E402
from starkcore import CodewordMatrix, DeviceCodeword, DeviceVector, MerkleForest   # noqa: E402
from univariate import Polynomial                  # noqa: E402

field = Field.main()
N2, S2 = 1 << 10, 10
SHAPE2 = (field.generator(), field.primitive_nth_root(N2), N2, 4, S2)       # the batched shape of tests/test_gpu_fri_batch.py
SHIFT = 4                                                                    # the expansion factor, as FastStark.prove passes it


def codeword(seed, N):
    om = field.primitive_nth_root(N)
    coeffs = [FieldElement(v, field) for v in synth.synth_ints(seed, N // 4)]
    return fast_coset_evaluate_device(Polynomial(coeffs), field.generator(), om, N)


def fresh(cw):
    return DeviceCodeword(DeviceVector.from_bytes(cw.vec.to_bytes()), field)


def streams_of(kind, K):
    return [ProofStream() if kind == "plain" else SignatureProofStream(b"document %d" % m) for m in range(K)]


def further_forests(K, N):
    """(forests, owners, the shared codeword): two trees per member in one forest, one tree for everybody in the other"""
    pairs = [codeword(5000 + k, N) for k in range(2 * K)]
    shared = codeword(4999, N)
    forests = [MerkleForest.build(CodewordMatrix.from_members(pairs)), MerkleForest.build(CodewordMatrix.from_members([shared]))]
    owners = [[[2 * m, 2 * m + 1] for m in range(K)], [[0] for _ in range(K)]]
    return forests, owners, shared


def expected_positions(indices, N):
    """opened_positions of FastStark.prove (fast_stark.py:154-158)"""
    duplicated = [i for i in indices] + [(i + SHIFT) % N for i in indices]
    quadrupled = [i for i in duplicated] + [(i + (N // 2)) % N for i in duplicated]
    quadrupled.sort()
    return quadrupled


def check_answers(also, forests, owners, tops, N):
    K = len(tops)
    assert len(also.answers) == len(also.positions) == K
    for m in range(K):
        assert also.positions[m] == expected_positions(tops[m], N)
        assert len(also.positions[m]) == 4 * len(tops[m])
        pairs = [(p, tree) for p in range(len(forests)) for tree in owners[p][m]]
        assert len(also.answers[m]) == len(pairs)
        for (p, tree), (values, paths) in zip(pairs, also.answers[m]):
            want_values, want_paths = forests[p].query([(tree, i) for i in also.positions[m]])
            assert list(values) == list(want_values) and [list(path) for path in paths] == [list(path) for path in want_paths], (m, p, tree)
            for index, value, path in zip(also.positions[m], values, paths):
                assert Merkle.verify(forests[p].roots[tree], index, path, FieldElement(value, field)), (m, p, tree, index)


class Census:
    """the bound library with every call counted by name"""

    def __init__(self, lib):
        self.lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("sc_"):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("kind", ["plain", "signature"])
def test_openings_travel_with_the_batch(K, kind, monkeypatch):
    fr = Fri(*SHAPE2)
    base = [codeword(9000 + k, N2) for k in range(K)]
    forests, owners, shared = further_forests(K, N2)
    assert forests[1].count == 1 and forests[1].roots[0] == Merkle.commit(shared)
    single, without, with_ = streams_of(kind, K), streams_of(kind, K), streams_of(kind, K)
    want = [fr.prove(fresh(cw), ps) for cw, ps in zip(base, single)]
    assert fr.prove_batch([fresh(cw) for cw in base], without) == want
    also = AlsoOpenForests(forests, owners, SHIFT)
    census = Census(sc.lib())
    with monkeypatch.context() as mp:
        mp.setattr(sc, "lib", lambda: census)
        got = fr.prove_batch([fresh(cw) for cw in base], with_, also)
    assert census.calls.get("sc_merkle_forest_query_dev", 0) == 1
    assert got == want
    for m in range(K):
        assert with_[m].serialize() == without[m].serialize() == single[m].serialize(), m
    check_answers(also, forests, owners, got, N2)


def test_one_query_per_chunk_when_the_batch_is_split(monkeypatch):
    """FOREST_MAX_LEAVES = 2 rows: 5 members go in chunks of 2, 2 and 1; the further forests' tree numbers stay those of the batch"""
    K = 5
    fr = Fri(*SHAPE2)
    base = [codeword(9000 + k, N2) for k in range(K)]
    forests, owners, _ = further_forests(K, N2)
    without, with_ = streams_of("plain", K), streams_of("plain", K)
    want = fr.prove_batch([fresh(cw) for cw in base], without)
    also = AlsoOpenForests(forests, owners, SHIFT)
    census = Census(sc.lib())
    before = sc.forest_stats()
    with monkeypatch.context() as mp:
        mp.setattr(sc, "FOREST_MAX_LEAVES", 2 * N2)
        mp.setattr(sc, "lib", lambda: census)
        got = fr.prove_batch([fresh(cw) for cw in base], with_, also)
    after = sc.forest_stats()
    assert after[0] - before[0] == 3 * fr.num_rounds()                   # three chunks, one forest per round each
    assert census.calls.get("sc_merkle_forest_query_dev", 0) == 3
    assert got == want
    assert [s.serialize() for s in with_] == [s.serialize() for s in without]
    check_answers(also, forests, owners, got, N2)


def test_the_member_by_member_fallback_fills_the_answers(monkeypatch):
    """one round: the forest path does not serve it, the members go through prove, and ONE separate query fetches the openings"""
    N, K = 32, 3
    fr = Fri(field.generator(), field.primitive_nth_root(N), N, 4, 4)
    assert fr.num_rounds() == 1
    base = [codeword(300 + k, N) for k in range(K)]
    forests, owners, _ = further_forests(K, N)
    single, with_ = streams_of("plain", K), streams_of("plain", K)
    want = [fr.prove(fresh(cw), ps) for cw, ps in zip(base, single)]
    also = AlsoOpenForests(forests, owners, SHIFT)
    census = Census(sc.lib())
    before = sc.forest_stats()
    with monkeypatch.context() as mp:
        mp.setattr(sc, "lib", lambda: census)
        got = fr.prove_batch([fresh(cw) for cw in base], with_, also)
    assert sc.forest_stats() == before                                   # no forest of the prover's own
    assert census.calls.get("sc_merkle_forest_query_dev", 0) == 1
    assert got == want
    assert [s.serialize() for s in with_] == [s.serialize() for s in single]
    check_answers(also, forests, owners, got, N)


def test_argument_errors_come_before_any_work():
    K = 3
    fr = Fri(*SHAPE2)
    base = [codeword(9000 + k, N2) for k in range(K)]
    forests, owners, _ = further_forests(K, N2)
    short = MerkleForest.build(CodewordMatrix.from_members([codeword(77, N2 // 2)]))
    wrong = [AlsoOpenForests(forests + [short], owners + [[[0]] * K], SHIFT),             # a forest of another row length
             AlsoOpenForests(forests, [owners[0][:-1], owners[1]], SHIFT),                # a member without owners
             AlsoOpenForests(forests, [owners[0], [0] * K], SHIFT),                       # tree numbers, not lists of them
             AlsoOpenForests(forests, [owners[0]], SHIFT)]                                # a forest without owners
    before = sc.forest_stats()
    for also in wrong:
        streams = streams_of("plain", K)
        with pytest.raises(AssertionError):
            fr.prove_batch([fresh(cw) for cw in base], streams, also)
        assert all(s.objects == [] for s in streams)
        assert also.answers is None and also.positions is None
    assert sc.forest_stats() == before

"""The batched verifier (FastStark.verify_batch, Fri.verify_batch; csrc/merkle_verify.cuh through sc_merkle_verify_batch and
sc_fri_colinearity_batch) against the host functions it replaces: Merkle.verify / verify_, test_colinearity, Fri.verify and
FastStark.verify.  Where the host function raises, the batch must say False; one malformed proof must not move the others."""
import pickle
import random
from hashlib import blake2b, shake_256

import numpy as np
import pytest

from verify_spies import host_verdict, row_counts           # noqa: F401  (row_counts: a fixture)
from workload_rescue_prime import RescuePrime

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import starkcore as sc                             # noqa: E402
import fast_stark                                  # noqa: E402
import workloads                                   # noqa: E402
from fast_stark import DeviceTrace, FastStark      # noqa: E402
from fri import BatchChecks, Fri                   # noqa: E402
from algebra import Field, FieldElement            # noqa: E402
from ip import ProofStream                         # noqa: E402
from merkle import Merkle                          # noqa: E402
from ntt import fast_coset_evaluate_device         # noqa: E402
from starkcore import DeviceCodeword, MerkleTree   # noqa: E402
from univariate import Polynomial, test_colinearity  # noqa: E402

P = Field.P_MAIN


def _seed_urandom(seed):
    rng = random.Random(seed)
    fast_stark.os.urandom = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
    return rng


@pytest.fixture
def seeded_urandom():
    genuine = fast_stark.os.urandom
    yield _seed_urandom
    fast_stark.os.urandom = genuine


def flipped(digest, at=0):
    return digest[:at] + bytes([digest[at] ^ 1]) + digest[at + 1:]


# ---- Merkle rows ---------------------------------------------------------------------------------------------------------------

def merkle_batch(cases):
    checks = BatchChecks(len(cases))
    for owner, case in enumerate(cases):
        checks.merkle(owner, *case)
    return checks.run()


@pytest.mark.parametrize("logn", [1, 2, 3, 7, 12, 16, 20])
def test_merkle_rows_match_merkle_verify(logn):
    field = Field.main()
    rng = random.Random(900 + logn)
    n = 1 << logn
    values = [rng.randrange(P) for _ in range(n)]
    tree = MerkleTree.from_bytes(b"".join(v.to_bytes(16, "little") for v in values))
    root = tree.root
    cases = []
    for _ in range(16):
        i = rng.randrange(n)
        path = tree.open(i)
        leaf = FieldElement(values[i], field)
        cases.append((root, i, path, leaf))                                             # honest
        cases.append((root, i, path, leaf + field.one()))                               # the leaf
        for d in range(logn):                                                           # each digest position of the path
            cases.append((root, i, [flipped(p, d % 64) if k == d else p for k, p in enumerate(path)], leaf))
        cases.append((root, i ^ 1, path, leaf))                                         # the wrong index
        cases.append((flipped(root, 63), i, path, leaf))                                # the wrong root
        cases.append((root, i, path[:-1], leaf))                                        # one level short
        cases.append((root, i, path + [path[-1]], leaf))                                # one level long
        cases.append((root, i, path, FieldElement(values[i] + P, field)))               # a leaf value >= p
        cases.append((root, i, path, FieldElement(-values[i] - 1, field)))              # a negative value
        cases.append((root, i, path, FieldElement(values[i] + (1 << 200), field)))      # beyond 16 bytes
        cases.append((root, i, path, b"%d" % values[i]))                                # a leaf of another type that hashes the same
        cases.append((root, i, path, values[i]))                                        # a leaf of the wrong type (bytes(int))
        cases.append((root, -1, path, leaf))                                            # a negative index
        cases.append((root[:32], i, path, leaf))                                        # a root of the wrong length
        cases.append((root, i, [p[:32] for p in path], leaf))                           # digests of the wrong length
    want = [host_verdict(Merkle.verify, *case) for case in cases]
    assert merkle_batch(cases) == want
    assert sum(want) >= 16


def test_merkle_digest_leaves_match_verify_():
    """Merkle.verify_ (a raw leaf digest) through the C entry's rows directly; also a batch split into many staging chunks"""
    rng = random.Random(5)
    leafs = [blake2b(i.to_bytes(2, "little")).digest() for i in range(1 << 9)]
    root = Merkle.commit_(leafs)
    rows, digests, roots, want, nd = [], [], [root, flipped(root)], [], 0
    for t in range(3000):
        i = rng.randrange(len(leafs))
        path = Merkle.open_(i, leafs)
        leaf = leafs[i] if t % 3 else leafs[(i + 1) % len(leafs)]
        r = t % 7 == 0
        digests.append(leaf)
        rows.append((i, nd + 1, int(r), len(path), sc.LEAF_DIGEST, nd.to_bytes(16, "little")))
        digests += path
        nd += 1 + len(path)
        want.append(Merkle.verify_(roots[r], i, path, leaf))
    arr = sc.merkle_rows(*[[r[k] for r in rows] for k in range(5)], b"".join(r[5] for r in rows))
    got = sc.merkle_verify_batch(arr, b"".join(digests), b"".join(roots))
    assert [bool(v) for v in got] == want
    sc._check(sc.lib().sc_set_tuning(b"verify_stage_kb", 16))           # ~25 rows per chunk
    try:
        assert [bool(v) for v in sc.merkle_verify_batch(arr, b"".join(digests), b"".join(roots))] == want
        # rows out of order: the chunks' digest ranges grow, the verdicts do not change
        perm = np.random.default_rng(3).permutation(len(arr))
        got = sc.merkle_verify_batch(arr[perm], b"".join(digests), b"".join(roots))
        assert [bool(v) for v in got] == [want[k] for k in perm]
    finally:
        sc._check(sc.lib().sc_set_tuning(b"verify_stage_kb", 65536))


def test_merkle_leaf_digests_far_from_their_paths():
    """leaf digests kept in a table of their own, far from the paths (each row's leaf is staged on its own): correct verdicts at the
    smallest staging buffer and at the default one"""
    rng = random.Random(6)
    leafs = [blake2b(i.to_bytes(2, "little")).digest() for i in range(1 << 10)]
    root = Merkle.commit_(leafs)
    rows, paths, want = [], [], []
    nd = len(leafs)                                   # digests = [the leaf table][paths ...]
    for t in range(2000):
        i = rng.randrange(len(leafs))
        path = Merkle.open_(i, leafs)
        leaf_index = i if t % 4 else (i + 1) % len(leafs)
        rows.append((i, nd, 0, len(path), sc.LEAF_DIGEST, leaf_index.to_bytes(16, "little")))
        paths += path
        nd += len(path)
        want.append(Merkle.verify_(root, i, path, leafs[leaf_index]))
    arr = sc.merkle_rows(*[[r[k] for r in rows] for k in range(5)], b"".join(r[5] for r in rows))
    digests = b"".join(leafs) + b"".join(paths)
    rev = arr[::-1].copy()                            # the leaf table stays at the front while the paths run backwards
    sc._check(sc.lib().sc_set_tuning(b"verify_stage_kb", 16))
    try:
        assert [bool(v) for v in sc.merkle_verify_batch(arr, digests, root)] == want
        assert [bool(v) for v in sc.merkle_verify_batch(rev, digests, root)] == want[::-1]
    finally:
        sc._check(sc.lib().sc_set_tuning(b"verify_stage_kb", 65536))
    assert [bool(v) for v in sc.merkle_verify_batch(arr, digests, root)] == want
    assert 0 < sum(want) < len(want)


def test_merkle_rows_outside_their_tables_are_refused():
    arr = sc.merkle_rows([0], [0], [1], [1], [sc.LEAF_RESIDUE], bytes(16))
    with pytest.raises(sc.StarkCoreError):
        sc.merkle_verify_batch(arr, bytes(64), bytes(64))              # root 1 of a table of one
    arr = sc.merkle_rows([0], [0], [0], [2], [sc.LEAF_RESIDUE], bytes(16))
    with pytest.raises(sc.StarkCoreError):
        sc.merkle_verify_batch(arr, bytes(64), bytes(64))              # a path of two digests in a table of one


# ---- colinearity rows ----------------------------------------------------------------------------------------------------------

def test_colinearity_rows_match_test_colinearity():
    field = Field.main()
    rng = random.Random(11)
    cases = []
    for log_n in (3, 10, 20, 30):
        omega, offset = field.primitive_nth_root(1 << log_n), field.generator() ^ rng.randrange(1, 5)
        alpha = FieldElement(rng.randrange(P), field)
        half = 1 << (log_n - 1)
        for t in range(60):
            a = rng.randrange(half)
            b = a + half
            xa, xb = offset * (omega ^ a), offset * (omega ^ b)
            ya, yb = FieldElement(rng.randrange(P), field), FieldElement(rng.randrange(P), field)
            kind = t % 6
            if kind == 0:              # honest: the fold's value at alpha
                yc = ya + (yb - ya) / (xb - xa) * (alpha - xa)
            elif kind == 1:
                yc = FieldElement(rng.randrange(P), field)
            elif kind == 2:            # y_a == y_b
                yb, yc = ya, ya
            elif kind == 3:            # coinciding abscissas: decided on the host
                b = a
                yc = ya
            elif kind == 4:            # alpha on the domain
                cases.append((offset, omega, a, b, xa, ya, yb, ya + (yb - ya) / (xb - xa) * (xa - xa)))
                continue
            else:                      # a value that is not a canonical residue
                yc = FieldElement(P + 3, field)
            cases.append((offset, omega, a, b, alpha, ya, yb, yc))
    checks = BatchChecks(len(cases))
    for owner, (offset, omega, a, b, alpha, ya, yb, yc) in enumerate(cases):
        checks.colinearity(owner, checks.round(offset, omega, alpha), offset, omega, a, b, alpha, ya, yb, yc)
    want = [host_verdict(test_colinearity, [(offset * (omega ^ a), ya), (offset * (omega ^ b), yb), (alpha, yc)])
            for offset, omega, a, b, alpha, ya, yb, yc in cases]
    assert checks.run() == want
    assert 0 < sum(want) < len(want)


# ---- Fri.verify_batch ----------------------------------------------------------------------------------------------------------

def fri_proof(field, N, s, seed, zero_stretch=None):
    om = field.primitive_nth_root(N)
    rng = random.Random(seed)
    poly = Polynomial([FieldElement(rng.randrange(P), field) for _ in range(N // 4)])
    cw = fast_coset_evaluate_device(poly, field.generator(), om, N)
    if zero_stretch is not None:      # a dishonest prover: its codeword is not of low degree
        values = cw.tolist()
        lo, hi = zero_stretch
        values[lo:hi] = [field.zero()] * (hi - lo)
        cw = DeviceCodeword.from_list(values, field)
    fr = Fri(field.generator(), om, N, 4, s)
    ps = ProofStream()
    fr.prove(cw, ps)
    return fr, ps.serialize()


@pytest.mark.parametrize("N,s", [(1 << 8, 4), (1 << 10, 10), (1 << 13, 16), (1 << 16, 40)])
def test_fri_verify_batch_matches_fri_verify(N, s):
    field = Field.main()
    fr, proof = fri_proof(field, N, s, N + s)
    _, other = fri_proof(field, N, s, N + s + 1)
    _, dishonest = fri_proof(field, N, s, N + s + 2, zero_stretch=(N // 3, N // 3 + N // 8))
    objects = pickle.loads(proof)
    rounds = fr.num_rounds()
    variants = [proof, other, dishonest]

    def changed(at, value):
        o = list(objects)
        o[at] = value
        variants.append(pickle.dumps(o))

    changed(0, flipped(objects[0]))                                                          # a root
    last = objects[rounds]
    changed(rounds, [last[0] + field.one()] + last[1:])                                      # the last codeword
    a, b, c = objects[rounds + 1]
    changed(rounds + 1, (a, b, c + field.one()))                                             # a triple value (round 0)
    a, b, c = objects[rounds + 3]
    changed(rounds + 3, (a + field.one(), b, c))                                             # a leaf of round 0, third test
    later = rounds + 1 + 4 * s                                                               # the first triple of round 1
    if rounds > 2:
        a, b, c = objects[later]
        changed(later, (a, b + field.one(), c))
    path_at = rounds + 1 + s
    changed(path_at, [flipped(objects[path_at][0])] + objects[path_at][1:])                  # a path digest
    changed(path_at + 2, objects[path_at + 2][:-1])                                          # a path one level short
    changed(path_at + 1, "not a path")                                                       # an object of the wrong type
    variants.append(pickle.dumps(objects[:len(objects) // 2]))                               # a truncated stream
    variants.append(proof)
    want_values, want = [], []
    for v in variants:
        values = []
        want.append(host_verdict(fr.verify, ProofStream().deserialize(v), values))
        want_values.append(values)
    streams = [ProofStream().deserialize(v) for v in variants]
    got_values = [[] for _ in variants]
    got = fr.verify_batch(streams, got_values)
    assert got == want
    assert want[0] and want[1] and want[-1] and not want[2] and sum(want) == 3
    for k, (w, g) in enumerate(zip(want_values, got_values)):
        if k < len(variants) - 2:         # (Fri.verify raises on the truncated stream: its list is not part of the contract)
            assert g == w, k


def test_fri_verify_batch_empty_and_single():
    field = Field.main()
    fr, proof = fri_proof(field, 1 << 10, 8, 3)
    assert fr.verify_batch([], []) == []
    values = []
    assert fr.verify_batch([ProofStream().deserialize(proof)], [values]) == [True]
    host = []
    assert fr.verify(ProofStream().deserialize(proof), host) is True
    assert values == host and len(values) == 2 * 8


# ---- FastStark.verify_batch ----------------------------------------------------------------------------------------------------

class DocumentProofStream(ProofStream):
    """the tutorial's signature scheme: the transcript is prefixed with the document, so a proof is bound to it"""

    def __init__(self, document):
        ProofStream.__init__(self)
        self.prefix = shake_256(document).digest(32)

    def prover_fiat_shamir(self, num_bytes=32):
        return shake_256(self.prefix + self.serialize()).digest(num_bytes)

    def verifier_fiat_shamir(self, num_bytes=32):
        return shake_256(self.prefix + pickle.dumps(self.objects[:self.read_index])).digest(num_bytes)

    def deserialize(self, bb):
        ps = DocumentProofStream(b"")
        ps.prefix = self.prefix
        ps.objects = pickle.loads(bb)
        return ps


@pytest.fixture(scope="module")
def rescue_instance():
    field = Field.main()
    genuine = fast_stark.os.urandom
    try:
        _seed_urandom(77)
        rp = RescuePrime()
        stark = FastStark(field, 4, 4, 4, rp.m, rp.N + 1)
        tz, tz_codeword, tz_root = stark.preprocess()
        proofs, boundaries = [], []
        for k in range(3):
            inp = field.sample(b"batch %d" % k)
            air, boundary = rp.transition_constraints(stark.omicron), rp.boundary_constraints(rp.hash(inp))
            proofs.append(stark.prove(rp.trace(inp), air, boundary, tz, tz_codeword))
            boundaries.append(boundary)
        signed = {}
        for doc in (b"document one", b"document two"):
            inp = field.sample(b"key")
            boundary = rp.boundary_constraints(rp.hash(inp))
            signed[doc] = (stark.prove(rp.trace(inp), air, boundary, tz, tz_codeword, DocumentProofStream(doc)), boundary)
    finally:
        fast_stark.os.urandom = genuine
    return stark, air, tz_root, proofs, boundaries, signed, rp


def test_stark_verify_batch_rescue_prime_and_alterations(rescue_instance):
    stark, air, tz_root, proofs, boundaries, _, rp = rescue_instance
    field = Field.main()
    objects = pickle.loads(proofs[0])
    cases = [(p, b) for p, b in zip(proofs, boundaries)]
    cases.append((proofs[1], boundaries[0]))                                              # the wrong boundary

    def changed(at, value):
        o = list(objects)
        o[at] = value
        cases.append((pickle.dumps(o), boundaries[0]))

    leaf_at, path_at = len(objects) - 2, len(objects) - 1                                 # the alteration classes of
    changed(leaf_at, objects[leaf_at] + field.one())                                      # test_verifier_rejects_tampered_proofs
    changed(path_at, [flipped(objects[path_at][0])] + objects[path_at][1:])
    first_fri = rp.m + 1
    rounds = stark.fri.num_rounds()
    last_at = first_fri + rounds
    changed(last_at, [objects[last_at][0] + field.one()] + objects[last_at][1:])
    triple_at = last_at + 1
    a, b, c = objects[triple_at]
    changed(triple_at, (a, b, c + field.one()))
    fri_path_at = triple_at + stark.fri.num_colinearity_tests
    changed(fri_path_at, [flipped(objects[fri_path_at][0])] + objects[fri_path_at][1:])
    changed(first_fri, flipped(objects[first_fri]))
    changed(0, flipped(objects[0]))                                                       # a register's root
    changed(leaf_at, "a leaf of the wrong type")
    cases.insert(2, (pickle.dumps([]), boundaries[0]))                                    # an emptied stream in the middle
    cases.insert(4, (pickle.dumps(objects[:len(objects) // 3]), boundaries[0]))           # a truncated one
    want = [host_verdict(stark.verify, p, air, b, tz_root) for p, b in cases]
    got = stark.verify_batch([p for p, _ in cases], air, [b for _, b in cases], tz_root)
    assert got == want
    assert want[:2] == [True, True] and want[2] is False and want[3] is True and want[4] is False and sum(want) == 3
    # each proof alone gives the same verdict as in the batch
    for (p, b), w in zip(cases[:6], want[:6]):
        assert stark.verify_batch([p], air, [b], tz_root) == [w]
    assert stark.verify_batch([], air, [], tz_root) == []


def test_stark_verify_batch_document_bound_streams(rescue_instance):
    stark, air, tz_root, _, _, signed, _ = rescue_instance
    (p1, b1), (p2, b2) = signed[b"document one"], signed[b"document two"]
    streams = [DocumentProofStream(b"document one"), DocumentProofStream(b"document two"), DocumentProofStream(b"document two"),
               DocumentProofStream(b"document one")]
    proofs, boundaries = [p1, p2, p1, p2], [b1, b2, b1, b2]
    want = [host_verdict(stark.verify, p, air, b, tz_root, ps) for p, b, ps in zip(proofs, boundaries, streams)]
    assert want == [True, True, False, False]
    assert stark.verify_batch(proofs, air, boundaries, tz_root, streams) == want


@pytest.mark.parametrize("log_fri", [12, 14, 16])
def test_stark_verify_batch_synthetic_air(seeded_urandom, log_fri):
    s = 16
    field, T, packed, air, boundary = workloads.synthetic_stark_instance(log_fri, s)
    stark = FastStark(field, 4, s, 2 * s, 2, T)
    tz, committed, tz_root = stark.preprocess(device_resident=True)
    seeded_urandom(log_fri)
    trace = DeviceTrace.from_packed(packed, field)
    proofs = [stark.prove(trace, air, boundary, tz, committed) for _ in range(2)]
    objects = pickle.loads(proofs[0])
    bad = list(objects)
    bad[-2] = bad[-2] + field.one()
    wrong_boundary = [(c, r, v + field.one()) if k == 2 else (c, r, v) for k, (c, r, v) in enumerate(boundary)]
    cases = [(proofs[0], boundary), (pickle.dumps(bad), boundary), (proofs[1], boundary), (proofs[1], wrong_boundary)]
    want = [host_verdict(stark.verify, p, air, b, tz_root) for p, b in cases]
    assert want == [True, False, True, False]
    assert stark.verify_batch([p for p, _ in cases], air, [b for _, b in cases], tz_root) == want


def test_stark_verify_batch_configs4_size(seeded_urandom):
    s, log_fri = 40, 24
    field, T, packed, air, boundary = workloads.synthetic_stark_instance(log_fri, s)
    stark = FastStark(field, 4, s, 2 * s, 2, T)
    tz, committed, tz_root = stark.preprocess(device_resident=True)
    seeded_urandom(24)
    proof = stark.prove(DeviceTrace.from_packed(packed, field), air, boundary, tz, committed)
    objects = pickle.loads(proof)
    bad = list(objects)
    bad[-1] = [flipped(bad[-1][0])] + bad[-1][1:]
    cases = [proof, pickle.dumps(bad)]
    want = [host_verdict(stark.verify, p, air, boundary, tz_root) for p in cases]
    assert want == [True, False]
    assert stark.verify_batch(cases, air, [boundary] * 2, tz_root) == want


# ---- what goes to the device -----------------------------------------------------------------------------------------------------

# (the `row_counts` spies: tests/verify_spies.py, imported above)

def test_honest_fri_proofs_check_every_row_on_the_device(row_counts):
    field = Field.main()
    N, s = 1 << 12, 12
    proofs = []
    for seed in range(3):
        fr, proof = fri_proof(field, N, s, 40 + seed)
        proofs.append(proof)
    rounds = fr.num_rounds()
    values = [[] for _ in proofs]
    assert fr.verify_batch([ProofStream().deserialize(p) for p in proofs], values) == [True] * 3
    assert row_counts["merkle"] == 3 * 3 * s * (rounds - 1)
    assert row_counts["colinearity"] == 3 * s * (rounds - 1)
    assert row_counts["undecided"] == row_counts["host_merkle"] == row_counts["host_colinearity"] == 0


def test_honest_stark_proofs_check_every_row_on_the_device(rescue_instance, row_counts):
    stark, air, tz_root, proofs, boundaries, _, _ = rescue_instance
    assert stark.verify_batch(proofs, air, boundaries, tz_root) == [True] * len(proofs)
    s, rounds = stark.fri.num_colinearity_tests, stark.fri.num_rounds()
    fri_rows = 3 * s * (rounds - 1)
    opened_rows = (stark.num_registers + 2) * 4 * s          # every committed codeword at 2 s opened points and their successors
    assert row_counts["merkle"] == len(proofs) * (fri_rows + opened_rows)
    assert row_counts["colinearity"] == len(proofs) * s * (rounds - 1)
    assert row_counts["undecided"] == row_counts["host_merkle"] == row_counts["host_colinearity"] == 0


def test_truncated_round_zero_values_when_a_later_triple_is_malformed():
    """a failed colinearity test followed by a malformed triple: Fri.verify returns False at the failed test, having appended the
    pairs up to it; the batch keeps the same pairs"""
    field = Field.main()
    s = 8
    fr, proof = fri_proof(field, 1 << 10, s, 77)
    objects = pickle.loads(proof)
    rounds = fr.num_rounds()
    a, b, c = objects[rounds + 2]
    objects[rounds + 2] = (a, b, c + field.one())          # test 1 of round 0 fails
    objects[rounds + 5] = objects[rounds + 5][:2]           # test 4 of round 0 cannot be unpacked
    changed = pickle.dumps(objects)
    host = []
    assert fr.verify(ProofStream().deserialize(changed), host) is False
    got = []
    assert fr.verify_batch([ProofStream().deserialize(changed)], [got]) == [False]
    assert got == host and len(got) == 4

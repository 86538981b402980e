"""Fri.prove_batch, Merkle.commit_batch and the Merkle forest underneath (csrc/merkle_forest.cuh through sc_merkle_forest_* and
sc_fri_fold_forest_dev): pinned to the reference's own proofs (tests/golden/fri.json), member by member against Fri.prove (itself
pinned to the reference by tests/test_gpu_host.py), forests against single trees and sc_fri_fold_dev, and the argument errors."""
import ctypes
import hashlib
import random

import pytest

from conftest import load_golden
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
from fri import Fri                                # noqa: E402
from ip import ProofStream                         # noqa: E402
from merkle import Merkle                          # noqa: E402
from ntt import fast_coset_evaluate_device         # noqa: E402
from starkcore import CodewordMatrix, DeviceCodeword, DeviceVector, MerkleForest   # noqa: E402
from univariate import Polynomial                  # noqa: E402

field = Field.main()
P = Field.P_MAIN
SC_ERR_BAD_ARG = -6


def codeword(seed, N):
    """a device-resident codeword of rate 1/4 on generator * <omega_N>, as tests/test_gpu_host.py builds the golden ones"""
    om = field.primitive_nth_root(N)
    coeffs = [FieldElement(v, field) for v in synth.synth_ints(seed, N // 4)]
    return fast_coset_evaluate_device(Polynomial(coeffs), field.generator(), om, N)


def fresh(cw):
    """a fresh copy of a device codeword (its own vector, no cached objects, no tree)"""
    return DeviceCodeword(DeviceVector.from_bytes(cw.vec.to_bytes()), field)


# ---- 1. pinned to the reference
def test_member_zero_is_the_references_proof():
    for rec in load_golden("fri.json")["prove_synth"]:
        N = 1 << rec["logN"]
        fr = Fri(field.generator(), field.primitive_nth_root(N), N, rec["expansion_factor"], rec["num_colinearity_tests"])
        assert fr.num_rounds() == rec["num_rounds"]
        members = [codeword(rec["coeff_seed"] + k, N) for k in range(5)]
        assert hashlib.sha256(members[0].vec.to_bytes()).hexdigest() == rec["codeword_sha256"]
        streams = [ProofStream() for _ in members]
        tops = fr.prove_batch(members, streams)
        ps = streams[0]
        assert tops[0] == rec["top_level_indices"]
        assert [o.hex() for o in ps.objects[:rec["num_rounds"]]] == rec["roots"]
        ser = ps.serialize()
        assert len(ps.objects) == rec["num_objects"] and len(ser) == rec["serialized_len"]
        assert hashlib.sha256(ser).hexdigest() == rec["serialized_sha256"], rec["logN"]
        assert all(fr.verify(s, []) for s in streams)


# ---- 2. member by member against Fri.prove, 3. the batched path ran
def make_streams(kind, K):
    """K equal pairs of fresh streams: one for prove_batch, one for prove"""
    def one(m):
        if kind == "plain":
            return ProofStream()
        if kind == "signature":
            return SignatureProofStream(b"document %d" % m)
        ps = ProofStream() if kind == "prior" else SignatureProofStream(b"signed %d" % m)
        for j in range(3):
            ps.push(hashlib.blake2b(b"earlier commitment %d %d" % (m, j)).digest())
        ps.push((FieldElement(7 + m, field), FieldElement(11, field)))      # not a digest: the single prover leaves its library path
        return ps
    return [one(m) for m in range(K)], [one(m) for m in range(K)]


N2, S2 = 1 << 10, 10
SHAPE2 = (field.generator(), field.primitive_nth_root(N2), N2, 4, S2)


@pytest.mark.parametrize("K", [1, 2, 5, 64])
@pytest.mark.parametrize("kind", ["plain", "signature", "prior", "prior_signature"])
@pytest.mark.parametrize("as_lists", [False, True])
def test_members_equal_single_proofs(K, kind, as_lists, monkeypatch):
    fr = Fri(*SHAPE2)
    base = [codeword(9000 + k, N2) for k in range(K)]
    single_inputs = [cw.tolist() if as_lists else fresh(cw) for cw in base]
    batch_inputs = [[FieldElement(e.value, field) for e in cw.tolist()] if as_lists else fresh(cw) for cw in base]
    batch_streams, single_streams = make_streams(kind, K)
    want = [fr.prove(cw, ps) for cw, ps in zip(single_inputs, single_streams)]
    before = sc.forest_stats()

    def refuse(*a, **k):
        raise AssertionError("the batched path must not go through the single prover")
    with monkeypatch.context() as mp:
        for name in ("prove", "commit", "query"):
            mp.setattr(Fri, name, refuse)
        got = fr.prove_batch(batch_inputs, batch_streams)
    after = sc.forest_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (fr.num_rounds(), K * fr.num_rounds())      # one forest of K trees per round
    assert got == want
    for m in range(K):
        assert batch_streams[m].serialize() == single_streams[m].serialize(), m
    prior = 4 if kind.startswith("prior") else 0
    for ps in batch_streams:
        ps.read_index = prior
        assert fr.verify(ps, []) is True
    for ps in batch_streams:
        ps.read_index = prior
    assert fr.verify_batch(batch_streams, [[] for _ in batch_streams]) == [True] * K


def test_shapes_outside_the_batched_path_go_member_by_member():
    before = sc.forest_stats()
    # fewer than two rounds
    N = 32
    fr = Fri(field.generator(), field.primitive_nth_root(N), N, 4, 4)
    assert fr.num_rounds() == 1
    cws = [codeword(300 + k, N) for k in range(3)]
    a, b = [ProofStream() for _ in cws], [ProofStream() for _ in cws]
    assert fr.prove_batch([fresh(c) for c in cws], a) == [fr.prove(fresh(c), s) for c, s in zip(cws, b)]
    assert [s.serialize() for s in a] == [s.serialize() for s in b]
    # a length that is not a power of two: the single prover's assertion, member by member
    om88 = field.primitive_nth_root(8) * FieldElement(pow(Field.G_MAIN, (P - 1) // 11, P), field)      # p - 1 = 11 * 37 * 2^119
    fr88 = Fri(field.generator(), om88, 88, 2, 1)
    members = [[FieldElement(v, field) for v in synth.synth_ints(40 + k, 88)] for k in range(2)]
    with pytest.raises(AssertionError):
        fr88.prove(members[0], ProofStream())
    with pytest.raises(AssertionError):
        fr88.prove_batch(members, [ProofStream(), ProofStream()])
    assert sc.forest_stats() == before
    assert fr.prove_batch([], []) == []


def outcome(fn):
    """what a call gives: ("ok", result) or ("raised", exception type)"""
    try:
        return ("ok", fn())
    except Exception as e:      # noqa: BLE001
        return ("raised", type(e))


def test_another_field_goes_member_by_member():
    """the forest kernels are hard-wired to the main field: a Fri over another field, or a member whose elements are another
    field's, must never reach them -- same result (or same exception) as `prove` member by member, forest counter unchanged"""
    before = sc.forest_stats()
    small = Field(97)                                              # 96 = 3 * 2^5; 5 generates the units
    N = 32
    om = FieldElement(pow(5, 96 // N, 97), small)
    assert pow(om.value, N, 97) == 1 and pow(om.value, N // 2, 97) != 1
    fr = Fri(FieldElement(5, small), om, N, 2, 2)
    assert fr.num_rounds() >= 2                                    # (only the field keeps it off the batched path)
    rng = random.Random(97)
    values = [[rng.randrange(97) for _ in range(N)] for _ in range(3)]
    make = lambda: [[FieldElement(v, small) for v in row] for row in values]
    a, b = [ProofStream() for _ in values], [ProofStream() for _ in values]
    got = outcome(lambda: fr.prove_batch(make(), a))
    want = outcome(lambda: [fr.prove(cw, s) for cw, s in zip(make(), b)])
    assert got == want
    if got[0] == "ok":
        assert [s.serialize() for s in a] == [s.serialize() for s in b]
    assert sc.forest_stats() == before
    # a Fri over the main field with a member of another field: as a list, and as a device codeword
    main = Fri(*SHAPE2)
    good = codeword(11, N2)
    other_values = [rng.randrange(97) for _ in range(N2)]
    for wrap in (lambda: [FieldElement(v, small) for v in other_values],
                 lambda: DeviceCodeword(DeviceVector.from_ints(other_values), small)):
        a, b = [ProofStream(), ProofStream()], [ProofStream(), ProofStream()]
        got = outcome(lambda: main.prove_batch([fresh(good), wrap()], a))
        want = outcome(lambda: [main.prove(cw, s) for cw, s in zip([fresh(good), wrap()], b)])
        assert got == want
        if got[0] == "ok":
            assert [s.serialize() for s in a] == [s.serialize() for s in b]
        assert sc.forest_stats() == before


def test_batches_above_the_forest_limit_are_split(monkeypatch):
    """with the limit lowered to two members' worth of leaves, a batch of five is three forests per round, and the results do not change"""
    fr = Fri(*SHAPE2)
    base = [codeword(9100 + k, N2) for k in range(5)]
    single_streams = [ProofStream() for _ in base]
    want = [fr.prove(fresh(cw), ps) for cw, ps in zip(base, single_streams)]
    monkeypatch.setattr(sc, "FOREST_MAX_LEAVES", 2 * N2)
    before = sc.forest_stats()
    streams = [ProofStream() for _ in base]
    assert fr.prove_batch([fresh(cw) for cw in base], streams) == want
    after = sc.forest_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (3 * fr.num_rounds(), 5 * fr.num_rounds())
    assert [s.serialize() for s in streams] == [s.serialize() for s in single_streams]
    arrays = [[FieldElement(v, field) for v in synth.synth_ints(9200 + k, N2)] for k in range(5)] + [[FieldElement(v, field) for v in synth.synth_ints(9300, 64)]]
    before = sc.forest_stats()
    assert Merkle.commit_batch(arrays) == [Merkle.commit(a) for a in arrays]
    after = sc.forest_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (3 + 1, 6)


def test_assertions_come_before_any_work():
    fr = Fri(*SHAPE2)
    good = codeword(1, N2)
    streams = [ProofStream(), ProofStream()]
    before = sc.forest_stats()
    with pytest.raises(AssertionError):
        fr.prove_batch([good, codeword(2, N2 // 2)], streams)           # a member of another length
    with pytest.raises(AssertionError):
        fr.prove_batch([good], streams)                                 # one stream too many
    wrong = Fri(field.generator(), field.primitive_nth_root(2 * N2), N2, 4, S2)      # omega of the wrong order
    with pytest.raises(AssertionError):
        wrong.prove_batch([good, good], streams)
    assert all(len(s.objects) == 0 for s in streams) and sc.forest_stats() == before


# ---- 4. forests against single trees
FOREST_SHAPES = [(2, 1), (2, 257), (4, 3), (4, 64), (128, 3), (128, 257), (256, 1), (256, 64), (256, 257), (512, 3), (512, 257), (1 << 12, 1), (1 << 12, 64),
                 (1 << 12, 257), (1 << 15, 3), (1 << 15, 64)]


# every shape with the default choice between one and four lanes per compression; the smaller ones with either form forced as well
FOREST_CASES = [(n, c, 256) for n, c in FOREST_SHAPES] + [(n, c, v) for v in (0, 1 << 20) for n, c in FOREST_SHAPES if n * c <= 1 << 18]


@pytest.mark.parametrize("n,count,four_lane_wgs", FOREST_CASES)
def test_forest_equals_single_trees(n, count, four_lane_wgs):
    rng = random.Random(n * 1000 + count)
    packed = synth.synth_packed(n + count, n * count).tobytes()
    rows = [packed[16 * n * t:16 * n * (t + 1)] for t in range(count)]
    sc.set_tuning("forest_four_lane_wgs", four_lane_wgs)
    try:
        forest = MerkleForest.build(CodewordMatrix.from_members(rows))
        roots = forest.roots
    finally:
        sc.set_tuning("forest_four_lane_wgs", 256)
    check = range(count) if count <= 64 else sorted({0, 1, count // 2, 255, 256, count - 1})
    trees = {t: sc.MerkleTree.from_bytes(rows[t]) for t in check}
    for t in check:
        assert roots[t] == trees[t].root, (t, n, count)
    positions = [(0, 0), (count - 1, n - 1), (count - 1, n - 1), (0, n - 1), (count - 1, 0)]
    positions += [(t, rng.randrange(n)) for t in check for _ in range(3)]
    values, paths = forest.query(positions)
    for (t, i), v, path in zip(positions, values, paths):
        assert v == int.from_bytes(rows[t][16 * i:16 * i + 16], "little")
        if t in trees:
            assert path == trees[t].open(i)
        assert Merkle.verify(roots[t], i, path, FieldElement(v, field))
    assert forest.open(count - 1, n - 1) == paths[1]


def test_commit_batch_equals_commit_and_the_goldens():
    arrays, want = [], []
    for rec in load_golden("merkle.json")["commit"]:
        vals = [int(v) for v in rec["values"]] if "values" in rec else synth.synth_ints(rec["seed"], rec["n"])
        arrays.append([FieldElement(v, field) for v in vals])
        want.append(bytes.fromhex(rec["root"]))
    extra = [[FieldElement(v, field) for v in synth.synth_ints(600 + k, 64)] for k in range(5)]
    device = [codeword(700 + k, 256) for k in range(3)]
    everything = arrays + extra + device
    got = Merkle.commit_batch(everything)
    assert got[:len(arrays)] == want
    assert got == [Merkle.commit(a) for a in everything]
    with pytest.raises(AssertionError):
        Merkle.commit_batch([arrays[-1], [field.one()] * 3])
    assert Merkle.commit_batch([]) == []


# ---- 5. the fold
def fold_case(vals_rows, n, alphas, offset, omega):
    lib = sc.lib()
    count = len(vals_rows)
    matrix = CodewordMatrix.from_members([synth.pack_ints(v) for v in vals_rows])
    forest = MerkleForest.fold_build(matrix, alphas, offset, omega)
    roots = forest.roots
    out = forest.matrix.to_bytes()
    for t in range(count):
        src, dst = DeviceVector.from_bytes(synth.pack_ints(vals_rows[t])), DeviceVector(max(1, n // 2))
        sc._check(lib.sc_fri_fold_dev(src.ptr, n, sc.fe_bytes(alphas[t]), sc.fe_bytes(offset), sc.fe_bytes(omega), dst.ptr, None))
        single = dst.to_bytes(0, n // 2)
        assert out[8 * n * t:8 * n * (t + 1)] == single, (n, t)
        if n >= 4:
            assert roots[t] == sc.MerkleTree.from_bytes(single).root, (n, t)
        else:
            assert roots[t] == hashlib.blake2b(b"%d" % int.from_bytes(single, "little")).digest()
    return out


def test_fold_forest_equals_single_folds_and_the_goldens():
    from oracle import py_oracle as po
    for rec in load_golden("fri.json")["fold"]:
        n, om = rec["n"], int(rec["omega"])
        cw = [po.evaluate(list(range(64)), pow(om, i, P)) for i in range(n)] if rec["kind"] == "test_fri_codeword" else synth.synth_ints(rec["seed"], n)
        out = fold_case([cw], n, [int(rec["alpha"])], int(rec["offset"]), om)          # one record of this n: a forest of one row
        assert hashlib.sha256(out).hexdigest() == rec["sha256"], n
        # ... and as row 0 of a forest with other rows and other challenges
        rows = [cw] + [synth.synth_ints(50 + k, n) for k in range(4)]
        alphas = [int(rec["alpha"])] + synth.synth_ints(60 + n, 4)
        out = fold_case(rows, n, alphas, int(rec["offset"]), om)
        assert hashlib.sha256(out[:8 * n]).hexdigest() == rec["sha256"], n
    for n, count in ((1 << 13, 3), (512, 300), (64, 257)):
        om = field.primitive_nth_root(n).value
        fold_case([synth.synth_ints(70 + t, n) for t in range(count)], n, [0, P - 1] + synth.synth_ints(80 + n, count - 2), Field.G_MAIN, om)


# ---- 6. argument errors: SC_ERR_BAD_ARG, nothing enqueued, and the library goes on working
def test_argument_errors():
    lib = sc.lib()
    n, count = 64, 3
    rows = [synth.synth_packed(90 + t, n).tobytes() for t in range(count)]
    matrix = CodewordMatrix.from_members(rows)
    out = CodewordMatrix(count, n // 2)
    h = ctypes.c_void_p()
    alphas = sc.pack([1, 2, 3])
    g, om = sc.fe_bytes(Field.G_MAIN), sc.fe_bytes(field.primitive_nth_root(n).value)
    before = sc.forest_stats()
    for bad_n in (0, 1, 3, 48):
        assert lib.sc_merkle_forest_build_dev(matrix.vec.ptr, bad_n, count, ctypes.byref(h), None) == SC_ERR_BAD_ARG
        assert lib.sc_fri_fold_forest_dev(matrix.vec.ptr, bad_n, count, alphas, g, om, out.vec.ptr, ctypes.byref(h), None) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_forest_build_dev(matrix.vec.ptr, n, 0, ctypes.byref(h), None) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_forest_build_dev(None, n, count, ctypes.byref(h), None) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_forest_build_dev(matrix.vec.ptr, n, count, None, None) == SC_ERR_BAD_ARG
    assert lib.sc_fri_fold_forest_dev(matrix.vec.ptr, n, 0, alphas, g, om, out.vec.ptr, ctypes.byref(h), None) == SC_ERR_BAD_ARG
    assert lib.sc_fri_fold_forest_dev(matrix.vec.ptr, n, count, None, g, om, out.vec.ptr, ctypes.byref(h), None) == SC_ERR_BAD_ARG
    assert lib.sc_fri_fold_forest_dev(None, n, count, alphas, g, om, out.vec.ptr, ctypes.byref(h), None) == SC_ERR_BAD_ARG
    assert lib.sc_fri_fold_forest_dev(matrix.vec.ptr, n, count, alphas, g, om, None, ctypes.byref(h), None) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_forest_roots(None, ctypes.create_string_buffer(64)) == SC_ERR_BAD_ARG
    # above the largest forest: unsupported (the Python side splits the batch), nothing enqueued
    assert lib.sc_merkle_forest_build_dev(matrix.vec.ptr, 1 << 20, 17, ctypes.byref(h), None) == sc.SC_ERR_UNSUPPORTED
    assert sc.forest_stats() == before
    forest = MerkleForest.build(matrix)
    elems, paths = ctypes.create_string_buffer(16 * 2), ctypes.create_string_buffer(64 * 6 * 2)
    one = (ctypes.c_uint64 * 1)(2)
    for tree, index in ((count, 0), (0, n), (1 << 40, 0), (0, 1 << 63)):
        assert lib.sc_merkle_forest_query_dev(1, (ctypes.c_void_p * 1)(forest._h), (ctypes.c_void_p * 1)(matrix.vec.ptr), (ctypes.c_uint64 * 2)(0, tree),
                                              (ctypes.c_uint64 * 2)(0, index), one, elems, paths) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_forest_query_dev(1, (ctypes.c_void_p * 1)(None), (ctypes.c_void_p * 1)(matrix.vec.ptr), (ctypes.c_uint64 * 2)(0, 0),
                                          (ctypes.c_uint64 * 2)(0, 0), one, elems, paths) == SC_ERR_BAD_ARG
    assert lib.sc_merkle_forest_query_dev(1, (ctypes.c_void_p * 1)(forest._h), (ctypes.c_void_p * 1)(matrix.vec.ptr), (ctypes.c_uint64 * 2)(0, 0),
                                          (ctypes.c_uint64 * 2)(0, 0), one, None, paths) == SC_ERR_BAD_ARG
    # a following valid call still gives the right roots and openings (here through plain host buffers, not the pinned pool)
    assert forest.roots == [sc.MerkleTree.from_bytes(r).root for r in rows]
    assert lib.sc_merkle_forest_query_dev(1, (ctypes.c_void_p * 1)(forest._h), (ctypes.c_void_p * 1)(matrix.vec.ptr), (ctypes.c_uint64 * 2)(0, 2),
                                          (ctypes.c_uint64 * 2)(5, 63), one, elems, paths) == 0
    assert elems.raw == rows[0][80:96] + rows[2][-16:]
    assert paths.raw[64 * 6:] == b"".join(sc.MerkleTree.from_bytes(rows[2]).open(63))
    assert Merkle.commit_batch([[FieldElement(v, field) for v in sc.unpack(r)] for r in rows]) == forest.roots

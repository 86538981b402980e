"""Pair leaves for FRI on the GPU (Fri(pair_leaves=True), csrc/fri_pairs.cuh, csrc/merkle_rows.hip):
sc_fri_fold_pairs_commit_dev against sc_fri_fold_dev followed by sc_merkle_rows_build_dev on two pointers, at every size at which the
build takes another path; sc_fri_pairs_query_dev against the hashlib model and Merkle.open_pair; proofs against the plain-Python prover
of tests/fri_pairs_cases.py, byte for byte; the verifier's rejections, alone and inside a verify_batch; prove_batch; FastStark and
FastRPSSS with the option; the sharded classes' refusal.

Two checks compare an option-on run with an option-off run of the same codeword.  The pair roots differ from the plain roots, so the two
transcripts -- and with them the challenges and the sampled indices -- differ between the runs; what is equal, and asserted, is the RULE:
each run's returned indices are sample_indices (the one, unchanged function) of its own transcript, at the same seed position, and each
run's polynomial_values are [(a, cw[a]), (a + N/2, cw[a + N/2])] per test over its own indices, in the same order."""
import ctypes
import functools
import os
import pickle
import random
from hashlib import blake2s, shake_256

import pytest

import fri_pairs_cases as cases
from fri_pairs_cases import G, P
from ip import ProofStream

pytestmark = pytest.mark.gpu
vp, u64 = ctypes.c_void_p, ctypes.c_uint64
GUARD = b"\xEE"
SC_OK, SC_ERR_NOT_POW2, SC_ERR_BAD_ARG = 0, -2, -6          # include/starkcore.h
PAD = 4                                                    # sentinel elements on either side of an output window


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


@pytest.fixture
def seeded(monkeypatch):
    def seed(value):
        rng = random.Random(value)
        monkeypatch.setattr(os, "urandom", lambda k: bytes(rng.getrandbits(8) for _ in range(k)))
    return seed


def field_and(values=None):
    from algebra import Field, FieldElement
    field = Field.main()
    return field, (None if values is None else [FieldElement(v, field) for v in values])


def level_of(sc, tree, level):
    out = sc.DeviceVector(4 * (tree.n >> level))
    tree.copy_level(level, out.ptr)
    sc.synchronize()
    return out.to_bytes()


# ---- sc_fri_fold_pairs_commit_dev ------------------------------------------------------------------------------------------------------
def fold_pairs_commit(sc, raw, n, stream=None):
    """-> (the folded bytes, the tree): the fold written into a window with PAD sentinel elements on either side, which must survive"""
    source = sc.DeviceVector.from_bytes(raw)
    window = sc.DeviceVector.from_bytes(GUARD * (16 * (n // 2 + 2 * PAD)))
    handle = vp()
    sc._check(sc.lib().sc_fri_fold_pairs_commit_dev(source.ptr, n, sc.fe_bytes(cases.FOLD_ALPHA), sc.fe_bytes(G), sc.fe_bytes(cases.root_of_unity(n)),
                                                    vp(window.ptr + 16 * PAD), ctypes.byref(handle), stream))
    tree = sc.MerkleTree(handle, None, n // 4)
    tree.root                                       # (waits for the build)
    got = window.to_bytes()
    assert got[:16 * PAD] == GUARD * (16 * PAD) and got[16 * (PAD + n // 2):] == GUARD * (16 * PAD)
    tree._keep = (source, window)
    return got[16 * PAD:16 * (PAD + n // 2)], tree


def fold_then_rows(sc, raw, n):
    """the yardstick: sc_fri_fold_dev, then sc_merkle_rows_build_dev over the two halves of its output"""
    source, folded = sc.DeviceVector.from_bytes(raw), sc.DeviceVector(n // 2)
    sc._check(sc.lib().sc_fri_fold_dev(source.ptr, n, sc.fe_bytes(cases.FOLD_ALPHA), sc.fe_bytes(G), sc.fe_bytes(cases.root_of_unity(n)), folded.ptr, None))
    table, handle, root = (vp * 2)(folded.ptr, folded.ptr + 16 * (n // 4)), vp(), ctypes.create_string_buffer(64)
    sc._check(sc.lib().sc_merkle_rows_build_dev(table, 2, n // 4, root, ctypes.byref(handle), None))
    tree = sc.MerkleTree(handle, root.raw, n // 4)
    tree._keep = folded
    return folded.to_bytes(), tree


@pytest.mark.parametrize("n", (4, 8, 512, 1024, 2048, 1 << 19, 1 << 20))
def test_fold_pairs_commit(sc, n):
    """4 and 8: trees of one and of two leaves; 512: 128 leaves, the fold kernel and the plain row leaf launch; 1024: 256 leaves, the
    smallest fused tree, one workgroup; 2048: two; 2^19: 2^17 leaves, the last size of the latency form (FUSE_MAX_W); 2^20: the first of
    the throughput form.  The folded vector and every level of the tree, byte for byte; up to 2048 also against hashlib."""
    raw = cases.fold_input(n)
    folded, tree = fold_pairs_commit(sc, raw, n)
    expected, yardstick = fold_then_rows(sc, raw, n)
    assert folded == expected
    assert tree.root == yardstick.root
    for level in range(tree.depth + 1):
        assert level_of(sc, tree, level) == level_of(sc, yardstick, level), "level %d" % level
    if n <= 2048:
        _, model, levels = cases.fold_reference(n)
        assert cases.unpack(folded) == model and tree.root == levels[-1][0]
        for level, digests in enumerate(levels):
            assert level_of(sc, tree, level) == b"".join(digests), "level %d" % level
    elif n == 1 << 19:                              # (2^17 leaves by hashlib: a fraction of a second)
        levels = cases.pair_levels_packed(folded)
        assert level_of(sc, tree, 0) == b"".join(levels[0]) and tree.root == levels[-1][0]


def test_fold_pairs_commit_on_a_caller_stream(sc):
    """free of the one-stream rule, as sc_fri_fold_commit_dev is: two folds alternate on two caller streams with no host wait between"""
    import torch
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    sizes = (2048, 1024, 4096, 512)
    sources = [sc.DeviceVector.from_bytes(cases.fold_input(n)) for n in sizes]
    outputs = [sc.DeviceVector(n // 2) for n in sizes]
    sc.synchronize()
    trees = []
    for k, (n, source, output) in enumerate(zip(sizes, sources, outputs)):
        handle = vp()
        sc._check(sc.lib().sc_fri_fold_pairs_commit_dev(source.ptr, n, sc.fe_bytes(cases.FOLD_ALPHA), sc.fe_bytes(G), sc.fe_bytes(cases.root_of_unity(n)),
                                                        output.ptr, ctypes.byref(handle), vp(streams[k % 2].cuda_stream)))
        trees.append(sc.MerkleTree(handle, None, n // 4))
    for n, tree, output in zip(sizes, trees, outputs):
        folded = cases.fold(cases.unpack(cases.fold_input(n)), cases.FOLD_ALPHA, G, cases.root_of_unity(n))
        assert tree.root == cases.pair_levels(folded)[-1][0]
    for s in streams:
        s.synchronize()
    for n, output in zip(sizes, outputs):
        assert cases.unpack(output.to_bytes()) == cases.fold(cases.unpack(cases.fold_input(n)), cases.FOLD_ALPHA, G, cases.root_of_unity(n))


def test_fold_pairs_commit_refusals(sc):
    lib = sc.lib()
    source, output = sc.DeviceVector.from_bytes(cases.fold_input(8)), sc.DeviceVector.from_bytes(GUARD * 64)
    alpha, offset, omega = sc.fe_bytes(cases.FOLD_ALPHA), sc.fe_bytes(G), sc.fe_bytes(cases.root_of_unity(8))
    handle = vp()
    for args in ((None, 8, alpha, offset, omega, output.ptr, ctypes.byref(handle), None),
                 (source.ptr, 8, alpha, offset, omega, None, ctypes.byref(handle), None),
                 (source.ptr, 8, alpha, offset, omega, output.ptr, None, None),
                 (source.ptr, 8, None, offset, omega, output.ptr, ctypes.byref(handle), None)):
        assert lib.sc_fri_fold_pairs_commit_dev(*args) == SC_ERR_BAD_ARG
    for n in (0, 2, 6, 12):
        assert lib.sc_fri_fold_pairs_commit_dev(source.ptr, n, alpha, offset, omega, output.ptr, ctypes.byref(handle), None) == SC_ERR_NOT_POW2
    sc.synchronize()
    assert not handle.value and output.to_bytes() == GUARD * 64


# ---- sc_fri_pairs_query_dev ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query_codeword(n):
    ints = cases.codeword(n, 4, seed=5)
    return ints, cases.pair_levels(ints)


def pairs_query(sc, codewords, requests, pinned):
    """sc_fri_pairs_query_dev into guarded buffers -> (pairs bytes, paths bytes)"""
    count = len(codewords)
    trees = [cw.pair_tree() for cw in codewords]
    flat = [i for request in requests for i in request]
    total = len(flat)
    pair_bytes, path_bytes = 32 * total, sum(64 * t.depth * len(r) for t, r in zip(trees, requests))
    arguments = (count, (vp * max(count, 1))(*[t._h for t in trees]), (vp * max(count, 1))(*[cw.vec.ptr for cw in codewords]), (u64 * max(total, 1))(*flat),
                 (u64 * max(count, 1))(*map(len, requests)))
    if pinned:
        split = (pair_bytes + 64 + 255) & ~255
        buffer = sc.HostBuffer(split + path_bytes + 64)
        buffer.array[:] = 0xEE
        sc._check(sc.lib().sc_fri_pairs_query_dev(*arguments, buffer.ptr, vp(buffer.ptr.value + split)))
        raw = buffer.array.tobytes()
        assert raw[pair_bytes:split] == GUARD * (split - pair_bytes) and raw[split + path_bytes:] == GUARD * 64
        return raw[:pair_bytes], raw[split:split + path_bytes]
    pairs, paths = ctypes.create_string_buffer(GUARD * (pair_bytes + 64), pair_bytes + 64), ctypes.create_string_buffer(GUARD * (path_bytes + 64), path_bytes + 64)
    sc._check(sc.lib().sc_fri_pairs_query_dev(*arguments, pairs, paths))
    assert pairs.raw[pair_bytes:] == GUARD * 64 and paths.raw[path_bytes:] == GUARD * 64
    return pairs.raw[:pair_bytes], paths.raw[:path_bytes]


@pytest.mark.parametrize("pinned", (False, True))
def test_pairs_query(sc, pinned):
    """three codewords of different lengths (pair trees of 512, 4 and 32 leaves) and two members that open nothing, in one call: leaf 0,
    the last leaf, a repeated leaf; values and paths against the hashlib model and against Merkle.open_pair on the host lists"""
    from merkle import Merkle
    field, _ = field_and()
    sizes = (1024, 64, 8, 64, 8)
    requests = [[0, 511, 77, 77, 256], [], [3, 0, 3], [0, 31, 16, 16], []]
    codewords = [sc.DeviceCodeword.from_list(field_and(query_codeword(n)[0])[1], field) for n in sizes]
    pairs, paths = pairs_query(sc, codewords, requests, pinned)
    expected_pairs, expected_paths = [], []
    for n, request in zip(sizes, requests):
        ints, levels = query_codeword(n)
        for a in request:
            expected_pairs.append(cases.pack([ints[a], ints[a + n // 2]]))
            expected_paths.append(b"".join(cases.path(levels, a)))
    assert pairs == b"".join(expected_pairs) and paths == b"".join(expected_paths)
    for n, request in zip(sizes, requests):
        host = field_and(query_codeword(n)[0])[1]
        for a in request[:2]:
            pair, path = Merkle.open_pair(a, host)
            assert [v.value for v in pair] == [query_codeword(n)[0][a], query_codeword(n)[0][a + n // 2]] and path == cases.path(query_codeword(n)[1], a)


def test_pairs_query_binding_and_host_definitions(sc):
    """starkcore.query_pairs, DeviceCodeword.start_pair_tree / pair_tree, Merkle.commit_pairs / open_pair on a DeviceCodeword (two pointers
    into the one vector), and commit_pairs against Merkle.commit of the same codeword"""
    from merkle import Merkle
    field, _ = field_and()
    ints, levels = query_codeword(1024)
    host = field_and(ints)[1]
    resident = sc.DeviceCodeword.from_list(host, field)
    assert resident.start_pair_tree().root == levels[-1][0] == Merkle.commit_pairs(resident) == Merkle.commit_pairs(host)
    assert Merkle.commit_pairs(resident) == Merkle.commit_rows([host[:512], host[512:]]) != Merkle.commit(resident)
    assert Merkle.commit_pairs(host[512:] + host[:512]) != levels[-1][0]
    (pairs, paths), (none, nothing) = sc.query_pairs([resident, resident], [[5, 511, 5], []])
    assert (none, nothing) == ([], [])
    assert [(a.value, b.value) for a, b in pairs] == [(ints[a], ints[a + 512]) for a in (5, 511, 5)]
    assert pairs[0][0] is pairs[2][0] is host[5] and pairs[1][1] is host[1023]           # entries keep their identity
    assert paths == [cases.path(levels, a) for a in (5, 511, 5)]
    pair, path = Merkle.open_pair(300, resident)
    assert pair == (host[300], host[812]) and Merkle.verify_pair(levels[-1][0], 300, path, pair) is True
    assert sc.query_pairs([resident], [[]]) == [([], [])]
    with pytest.raises(AssertionError):
        Merkle.open_pair(512, resident)


def test_pairs_query_refusals(sc):
    lib = sc.lib()
    field, _ = field_and()
    codewords = [sc.DeviceCodeword.from_list(field_and(query_codeword(n)[0])[1], field) for n in (64, 8)]
    trees = [cw.pair_tree() for cw in codewords]
    handles, pointers = (vp * 2)(*[t._h for t in trees]), (vp * 2)(*[cw.vec.ptr for cw in codewords])
    indices, counts = (u64 * 3)(0, 31, 3), (u64 * 2)(2, 1)
    pairs, paths = ctypes.create_string_buffer(GUARD * 256, 256), ctypes.create_string_buffer(GUARD * 1024, 1024)
    assert lib.sc_fri_pairs_query_dev(0, None, None, None, None, None, None) == SC_OK
    assert lib.sc_fri_pairs_query_dev(2, handles, pointers, indices, (u64 * 2)(0, 0), pairs, paths) == SC_OK
    assert lib.sc_fri_pairs_query_dev(2, handles, pointers, None, (u64 * 2)(0, 0), None, None) == SC_OK
    refused = [(2, None, pointers, indices, counts, pairs, paths), (2, handles, None, indices, counts, pairs, paths),
               (2, handles, pointers, None, counts, pairs, paths), (2, handles, pointers, indices, None, pairs, paths),
               (2, handles, pointers, indices, counts, None, paths), (2, handles, pointers, indices, counts, pairs, None),
               (2, (vp * 2)(trees[0]._h, None), pointers, indices, counts, pairs, paths),
               (2, handles, (vp * 2)(codewords[0].vec.ptr, None), indices, counts, pairs, paths),
               (2, handles, pointers, (u64 * 3)(0, 32, 3), counts, pairs, paths),            # leaf 32 of 32
               (2, handles, pointers, (u64 * 3)(0, 31, 4), counts, pairs, paths),            # leaf 4 of 4
               (2, handles, pointers, (u64 * 3)(0, 1 << 63, 3), counts, pairs, paths)]
    for arguments in refused:
        assert lib.sc_fri_pairs_query_dev(*arguments) == SC_ERR_BAD_ARG
    sc.synchronize()
    assert pairs.raw == GUARD * 256 and paths.raw == GUARD * 1024
    sc._check(lib.sc_fri_pairs_query_dev(2, handles, pointers, indices, counts, pairs, paths))
    assert pairs.raw[:96] != GUARD * 96 and pairs.raw[96:] == GUARD * 160


# ---- proofs ----------------------------------------------------------------------------------------------------------------------------
class DocumentStream(ProofStream):
    """a ProofStream subclass whose challenges are prefixed by a document's digest, as the signature scheme's is"""

    def __init__(self, document):
        ProofStream.__init__(self)
        self.document, self.prefix = document, blake2s(bytes(document)).digest()

    def prover_fiat_shamir(self, num_bytes=32):
        return shake_256(self.prefix + self.serialize()).digest(num_bytes)

    def verifier_fiat_shamir(self, num_bytes=32):
        return shake_256(self.prefix + pickle.dumps(self.objects[:self.read_index])).digest(num_bytes)

    def deserialize(self, bb):
        stream = DocumentStream(self.document)
        stream.objects = pickle.loads(bb)
        return stream


def new_stream(document=None):
    return ProofStream() if document is None else DocumentStream(document)


def fri_of(n, s, grinding_bits=0, pair_leaves=True):
    from fri import Fri
    field, _ = field_and()
    return Fri(field.generator(), field.primitive_nth_root(n), n, 4, s, grinding_bits=grinding_bits, pair_leaves=pair_leaves)


def resident_codeword(sc, n, seed=0):
    field, host = field_and(cases.codeword(n, 4, seed))
    return sc.DeviceCodeword.from_list(host, field)


def expected_values(ints, indices):
    n = len(ints)
    return [point for index in indices for a in [index % (n // 2)] for point in ((a, ints[a]), (a + n // 2, ints[a + n // 2]))]


@pytest.mark.parametrize("n,s,grinding_bits,document", [(4096, 4, 0, None), (64, 2, 0, None), (4096, 4, 4, None), (64, 2, 4, None),
                                                        (4096, 4, 0, b"a document"), (64, 2, 4, b"a document")])
def test_proof_is_the_plain_provers(sc, n, s, grinding_bits, document):
    """Fri(.., 4096, 4, 4): eight codewords, pair trees of 2048 .. 16 leaves -- the fused rounds and the unfused ones in one proof.  The
    serialized proof is the plain-Python prover's, byte for byte; verify accepts it after serialize / deserialize; the returned indices
    and polynomial_values follow the option-off rule (see the module's docstring)."""
    from algebra import FieldElement
    field, _ = field_and()
    ints = cases.codeword(n, 4)
    on, off = fri_of(n, s, grinding_bits), fri_of(n, s, grinding_bits, pair_leaves=False)
    stream = new_stream(document)
    indices = on.prove(resident_codeword(sc, n), stream)
    model = new_stream(document)
    top, codewords, roots = cases.prove(ints, G, cases.root_of_unity(n), 4, s, model, lambda v: FieldElement(v, field), grinding_bits)
    proof = stream.serialize()
    assert proof == model.serialize()
    assert indices == top
    objects = pickle.loads(proof)
    rounds = on.num_rounds()
    assert len(objects) == rounds + 1 + (1 if grinding_bits else 0) + 2 * s * (rounds - 1)
    assert sum(len(o) for o in objects if type(o) is list and o and type(o[0]) is bytes) == cases.digest_count(n, 4, s)
    values = []
    assert on.verify(stream.deserialize(proof), values) is True
    assert [(i, v.value) for i, v in values] == expected_values(ints, indices)
    # the option-off run of the same codeword: the same sampling function at the same seed position, the same form of polynomial_values
    plain = new_stream(document)
    plain_indices = off.prove(resident_codeword(sc, n), plain)
    plain_values = []
    assert off.verify(plain.deserialize(plain.serialize()), plain_values) is True
    assert [(i, v.value) for i, v in plain_values] == expected_values(ints, plain_indices)
    for run, fri, got in ((stream, on, indices), (plain, off, plain_indices)):
        reader = run.deserialize(run.serialize())
        reader.read_index = rounds + 1 + (1 if grinding_bits else 0)
        assert off.sample_indices(reader.verifier_fiat_shamir(), n // 2, n >> (rounds - 1), s) == got
    assert len(proof) < len(plain.serialize())
    # a host list (of elements over the prover's own field object: a proof is pickled by identity) proves to the same bytes
    again = new_stream(document)
    assert on.prove([FieldElement(v, on.field) for v in ints], again) == indices and again.serialize() == proof


@functools.lru_cache(maxsize=None)
def proof_objects_of(n, s, pair_leaves=True):
    import starkcore
    stream = new_stream()
    indices = fri_of(n, s, pair_leaves=pair_leaves).prove(resident_codeword(starkcore, n), stream)
    return pickle.loads(stream.serialize()), tuple(indices)


def stream_of(objects):
    stream = new_stream()
    stream.objects = pickle.loads(pickle.dumps(list(objects)))
    return stream


REJECTIONS = ("y_a changed", "members swapped", "digest changed", "path short", "three values", "value not below p", "last codeword changed",
              "option-off proof")


@pytest.mark.parametrize("what", REJECTIONS)
def test_rejections(sc, what):
    """each from verify, and as the middle member of a verify_batch of three whose other members stay accepted"""
    from algebra import FieldElement
    field, _ = field_and()
    n, s = 4096, 4
    on = fri_of(n, s)
    objects, indices = proof_objects_of(n, s)
    rounds = on.num_rounds()
    first = rounds + 1                              # round 0's pairs; its paths from first + s
    changed = pickle.loads(pickle.dumps(objects))
    ya, yb = changed[first]
    if what == "y_a changed":
        changed[first] = (FieldElement((ya.value + 1) % P, field), yb)
    elif what == "members swapped":
        changed[first] = (yb, ya)
    elif what == "digest changed":
        changed[first + s][2] = bytes([changed[first + s][2][0] ^ 1]) + changed[first + s][2][1:]
    elif what == "path short":
        changed[first + s + 1] = changed[first + s + 1][:-1]
    elif what == "three values":
        changed[first + 2 * s] = changed[first + 2 * s] + (ya,)
    elif what == "value not below p":
        changed[first + 1] = (changed[first + 1][0], FieldElement(P, field))
    elif what == "last codeword changed":
        a = indices[1] % len(changed[rounds])
        changed[rounds][a] = FieldElement((changed[rounds][a].value + 1) % P, field)
    else:
        changed = list(proof_objects_of(n, s, pair_leaves=False)[0])
    assert on.verify(stream_of(objects), []) is True
    assert on.verify(stream_of(changed), []) is False
    assert on.verify_batch([stream_of(objects), stream_of(changed), stream_of(objects)], [[], [], []]) == [True, False, True]


def test_option_on_proof_at_an_option_off_verifier(sc):
    n, s = 4096, 4
    off = fri_of(n, s, pair_leaves=False)
    objects, _ = proof_objects_of(n, s)
    plain, _ = proof_objects_of(n, s, pair_leaves=False)
    assert off.verify(stream_of(objects), []) is False
    assert off.verify_batch([stream_of(plain), stream_of(objects), stream_of(plain)], [[], [], []]) == [True, False, True]


def test_verify_batch_values_stop_at_the_first_failed_test(sc):
    """round 0 appends its pairs test by test and stops at the first failed colinearity test, in verify and in verify_batch alike"""
    from algebra import FieldElement
    field, _ = field_and()
    n, s = 4096, 4
    on = fri_of(n, s)
    objects, indices = proof_objects_of(n, s)
    first = on.num_rounds() + 1
    changed = pickle.loads(pickle.dumps(objects))
    ya, yb = changed[first + 2]
    changed[first + 2] = (FieldElement((ya.value + 1) % P, field), yb)          # the third test of round 0 fails
    alone, batched = [], [[], []]
    assert on.verify(stream_of(changed), alone) is False
    assert on.verify_batch([stream_of(changed), stream_of(objects)], batched) == [False, True]
    assert [i for i, _ in alone] == [i for i, _ in batched[0]] and len(alone) == 6
    assert [(i, v.value) for i, v in batched[1]] == expected_values(cases.codeword(n, 4), indices)


@pytest.mark.parametrize("documents", (None, (b"first", b"second", b"third")))
def test_prove_batch(sc, documents):
    """three members against three prove calls: same bytes, same indices; once with member-specific stream prefixes"""
    n, s = 4096, 4
    on = fri_of(n, s)
    documents = documents or (None, None, None)
    alone, alone_indices = [], []
    for k, document in enumerate(documents):
        stream = new_stream(document)
        alone_indices.append(on.prove(resident_codeword(sc, n, seed=k), stream))
        alone.append(stream.serialize())
    streams = [new_stream(document) for document in documents]
    assert on.prove_batch([resident_codeword(sc, n, seed=k) for k in range(3)], streams) == alone_indices
    assert [stream.serialize() for stream in streams] == alone
    assert len(set(alone)) == 3
    assert on.verify_batch([stream.deserialize(proof) for stream, proof in zip(streams, alone)], [[], [], []]) == [True, True, True]


# ---- FastStark / FastRPSSS -------------------------------------------------------------------------------------------------------------
S = 8


@functools.lru_cache(maxsize=None)
def stark_instance():
    import synth
    import workloads
    from algebra import FieldElement
    from fast_stark import FastStark
    field, T, _, air, boundary = workloads.synthetic_stark_instance(10, S)
    rows = [[FieldElement(a, field), FieldElement(b, field)] for a, b in zip(*synth.synthetic_air_columns(T))]
    off = FastStark(field, 4, S, 2 * S, 2, T)
    return field, T, rows, air, boundary, off, off.preprocess()


@pytest.mark.parametrize("options", ({}, {"row_commitments": True, "grinding_bits": 4}))
def test_fast_stark(sc, seeded, options):
    """the small synthetic AIR: prove, verify, verify_batch; the proof is shorter than the same prover's without pair leaves"""
    from fast_stark import FastStark
    field, T, rows, air, boundary, off, (tz, tz_codeword, root) = stark_instance()
    on = FastStark(field, 4, S, 2 * S, 2, T, pair_leaves=True, **options)
    same = FastStark(field, 4, S, 2 * S, 2, T, **options)
    assert on.pair_leaves is True and on.fri.pair_leaves is True and same.fri.pair_leaves is False
    seeded(71)
    proof = on.prove([list(r) for r in rows], air, boundary, tz, tz_codeword)
    seeded(71)
    other = same.prove([list(r) for r in rows], air, boundary, tz, tz_codeword)
    assert on.verify(proof, air, boundary, root) is True
    assert len(proof) < len(other)
    assert same.verify(proof, air, boundary, root) is False and on.verify(other, air, boundary, root) is False
    tampered = pickle.loads(proof)
    at = next(k for k, o in enumerate(tampered) if type(o) is tuple and len(o) == 2)
    tampered[at] = (tampered[at][1], tampered[at][0])
    assert on.verify_batch([proof, pickle.dumps(tampered), proof], air, [boundary] * 3, root) == [True, False, True]
    seeded(73)
    alone = [on.prove([list(r) for r in rows], air, boundary, tz, tz_codeword) for _ in range(2)]
    seeded(73)
    assert on.prove_batch([[list(r) for r in rows] for _ in range(2)], air, [boundary] * 2, tz, tz_codeword) == alone


@functools.lru_cache(maxsize=None)
def signer():
    from fast_rpsss import FastRPSSS
    return FastRPSSS(pair_leaves=True)


def test_signature(sc):
    scheme = signer()
    assert scheme.stark.pair_leaves is True and scheme.stark.fri.pair_leaves is True
    sk = scheme.field.sample(b"a key for a signature with pair leaves")
    pk = scheme.rp.hash(sk)
    signature = scheme.sign(sk, b"a document")
    assert scheme.verify(pk, b"a document", signature) is True
    assert scheme.verify(pk, b"another document", signature) is False
    objects = pickle.loads(signature)
    # the signature scheme's FRI shape (2^12, s = 64: four codewords): 64 (11 + 10 + 9) digests in the query phase's paths of pairs
    pair_places = [k for k, o in enumerate(objects) if type(o) is tuple and len(o) == 2]
    assert len(pair_places) == 64 * 3
    assert sum(len(objects[k + 64]) for k in pair_places) == 1920 == cases.digest_count(4096, 4, 64)


def test_sign_batch(sc, seeded):
    scheme = signer()
    sks = [scheme.field.sample(b"key %d of a batch with pair leaves" % k) for k in range(2)]
    pks = scheme.rp.hash_batch(sks)
    documents = [b"document %d" % k for k in range(2)]
    seeded(79)
    alone = [scheme.sign(sk, document) for sk, document in zip(sks, documents)]
    seeded(79)
    signatures = scheme.sign_batch(sks, documents)
    assert signatures == alone
    assert scheme.verify_batch(pks, documents, signatures) == [True, True]
    assert scheme.verify_batch(pks, documents, signatures[::-1]) == [False, False]


def test_sharded_classes_refuse():
    from algebra import Field
    from sharded_fri import ShardedFri
    from sharded_stark import ShardedFastStark
    with pytest.raises(AssertionError, match="pair_leaves is not supported"):
        ShardedFastStark(Field.main(), 4, S, 2 * S, 2, 32, 0, 1, None, pair_leaves=True)
    with pytest.raises(AssertionError, match="pair_leaves"):
        ShardedFri(fri_of(4096, 4), 64, 0, 1, None)

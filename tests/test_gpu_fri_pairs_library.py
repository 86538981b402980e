"""Fri.prove with pair leaves as ONE library call (Fri._prove_pairs_in_library, sc_fri_prove_pairs_dev, fri_tail_kernel<true>, DESIGN.md
3.4e): proofs against the plain-Python prover of tests/fri_pairs_cases.py, byte for byte, at the sizes at which the persistent tail
kernel's pair form takes another path; against the round-by-round route (Fri.PAIRS_IN_LIBRARY = False) where rounds run above the tail;
the tail switched on and off; which route a stream takes; the entry through ctypes -- layout of the answers, handles, refusals; FastStark.
No test makes the tail kernel give up: its waits are the option-off form's, which tests/test_gpu_host.py covers.

The codeword and the Fri are built over DIFFERENT Field objects on purpose, as tests/test_gpu_fri_pairs.py builds them: a proof is pickled
by identity, and every element of a proof carries the field object of the codeword that was proved."""
import ctypes
import functools
import os
import pickle
import random

import numpy as np
import pytest

import fri_pairs_cases as cases
from fri_pairs_cases import G
from ip import ProofStream

pytestmark = pytest.mark.gpu
vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
SC_OK, SC_ERR_NOT_POW2, SC_ERR_BAD_ARG, SC_ERR_UNSUPPORTED = 0, -2, -6, -7          # include/starkcore.h
GUARD = 0xEE


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


@pytest.fixture
def round_by_round(monkeypatch):
    """switches the library route off for the rest of the test when called"""
    from fri import Fri
    return lambda: monkeypatch.setattr(Fri, "PAIRS_IN_LIBRARY", False)


def main_field():
    from algebra import Field
    return Field.main()


def fri_of(n, s, grinding_bits=0):
    from fri import Fri
    field = main_field()
    return Fri(field.generator(), field.primitive_nth_root(n), n, 4, s, grinding_bits=grinding_bits, pair_leaves=True)


def resident(sc, ints):
    return sc.DeviceCodeword(sc.DeviceVector.from_bytes(cases.pack(ints)), main_field())


def resident_raw(sc, raw):
    return sc.DeviceCodeword(sc.DeviceVector.from_bytes(raw), main_field())


def tail_stats(sc):
    out = (u64 * 2)()
    sc._check(sc.lib().sc_fri_tail_stats(out))
    return out[0], out[1]                          # launches, launches that gave up


@functools.lru_cache(maxsize=None)
def model(n, s, grinding_bits):
    """the plain-Python prover's (proof bytes, top-level indices, codewords, roots), computed once"""
    from algebra import FieldElement
    field = main_field()
    stream = ProofStream()
    top, codewords, roots = cases.prove(cases.codeword(n, 4), G, cases.root_of_unity(n), 4, s, stream, lambda v: FieldElement(v, field), grinding_bits)
    return stream.serialize(), tuple(top), codewords, roots


# ---- bytes against the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,s,grinding_bits", [(64, 2, 0), (64, 2, 4), (4096, 4, 0), (4096, 4, 4), (1 << 17, 4, 0)])
def test_proof_is_the_plain_provers(sc, n, s, grinding_bits):
    """64: three codewords of 64, 32 and 16 elements, every round far below one workgroup (pair trees of 32, 16 and 8 leaves; trees of 2
    leaves and of 1 leaf, which no Fri of expansion factor 4 reaches: test_entry_smallest_trees); 4096: every round in the tail, the four-lane form;
    2^17: the tail's first round makes 2^16 elements (2^15 leaves, one lane per leaf, 128 workgroups), its second the widest grid (2^14
    leaves, four lanes per leaf, 256 workgroups).  One launch, no fall-back; the bytes and the indices are the model's; verify accepts."""
    fri = fri_of(n, s, grinding_bits)
    proof, top, _, _ = model(n, s, grinding_bits)
    before = tail_stats(sc)
    stream = ProofStream()
    indices = fri.prove(resident(sc, cases.codeword(n, 4)), stream)
    assert tail_stats(sc) == (before[0] + 1, before[1])
    assert any(type(segment).__name__ == "FriPairsQueryPhase" for segment in stream.objects._segments)
    got = stream.serialize()
    assert got == proof
    assert indices == list(top)
    assert fri.verify(stream.deserialize(got), []) is True


def test_rounds_above_the_tail(sc, round_by_round):
    """2^18: round 0's tree and one fold-and-commit launch (2^17 elements out) before the tail takes over.  Residues need not be a
    codeword for a prover; the round-by-round route is the yardstick."""
    n, s = 1 << 18, 4
    fri = fri_of(n, s)
    raw = cases.fold_input(n, seed=3)
    before = tail_stats(sc)
    stream = ProofStream()
    indices = fri.prove(resident_raw(sc, raw), stream)
    assert tail_stats(sc) == (before[0] + 1, before[1])
    got = stream.serialize()
    round_by_round()
    yardstick = ProofStream()
    assert fri.prove(resident_raw(sc, raw), yardstick) == indices
    assert tail_stats(sc) == (before[0] + 1, before[1])        # (that route never enters the tail kernel)
    assert yardstick.serialize() == got
    assert len(pickle.loads(got)) == fri.num_rounds() + 1 + 2 * s * (fri.num_rounds() - 1)


@pytest.mark.parametrize("n,s,grinding_bits", [(4096, 4, 0), (64, 2, 4), (1 << 17, 4, 0)])
def test_tail_on_and_off(sc, n, s, grinding_bits):
    fri = fri_of(n, s, grinding_bits)
    proof, top, _, _ = model(n, s, grinding_bits)
    for tail in (1, 0):
        sc.set_tuning("fri_tail", tail)
        try:
            before = tail_stats(sc)
            stream = ProofStream()
            indices = fri.prove(resident(sc, cases.codeword(n, 4)), stream)
            after = tail_stats(sc)
        finally:
            sc.set_tuning("fri_tail", 1)
        assert after == (before[0] + tail, before[1]), tail
        assert indices == list(top) and stream.serialize() == proof, tail


# ---- which route a stream takes ---------------------------------------------------------------------------------------------------------
class Subclass(ProofStream):
    pass


def test_route_taken(sc, monkeypatch, round_by_round):
    import proof_objects
    from algebra import FieldElement
    from fri import Fri
    n, s = 4096, 4
    fri = fri_of(n, s)
    proof, top, _, _ = model(n, s, 0)
    ints = cases.codeword(n, 4)
    taken = []
    real = Fri._prove_pairs_in_library

    def watched(self, *args):
        result = real(self, *args)
        taken.append(result is not None)
        return result
    monkeypatch.setattr(Fri, "_prove_pairs_in_library", watched)
    stream = ProofStream()
    assert fri.prove(resident(sc, ints), stream) == list(top)
    lazy = stream.objects
    assert isinstance(lazy, proof_objects.LazyProofObjects)
    assert [type(segment).__name__ for segment in lazy._segments if not isinstance(segment, proof_objects._Real)] == ["ElementList", "FriPairsQueryPhase"]
    pickled, real_pickler = [], sc.pickle_proof

    def library_pickler(ops, *args, **kwargs):
        pickled.append(len(ops))
        return real_pickler(ops, *args, **kwargs)
    monkeypatch.setattr(sc, "pickle_proof", library_pickler)
    assert stream.serialize() == proof
    assert len(pickled) == 1 and pickled[0] < len(proof) // 8  # through the library's pickler, ONCE, the payload by address ...
    assert lazy._all is None and not lazy._cache               # ... and nothing was materialised
    # a subclass of ProofStream and a host list: the round-by-round route, the same bytes
    other = Subclass()
    assert fri.prove(resident(sc, ints), other) == list(top) and other.serialize() == proof
    listed = ProofStream()
    assert fri.prove([FieldElement(v, fri.field) for v in ints], listed) == list(top) and listed.serialize() == proof
    assert taken == [True, False, False]
    # detached objects against the round-by-round route's
    detached = list(stream.objects.detach())
    round_by_round()
    plain = ProofStream()
    fri.prove(resident(sc, ints), plain)
    assert taken == [True, False, False]                       # (switched off: not even asked)
    assert type(plain.objects) is list
    assert detached == plain.objects and [type(o) for o in detached] == [type(o) for o in plain.objects]
    assert pickle.dumps(detached) == proof


# ---- the entry through ctypes -----------------------------------------------------------------------------------------------------------
class Call:
    """one call of sc_fri_prove_pairs_dev on the 4096-element codeword with ONE further (ordinary tree, vector) pair; every output
    buffer is filled with a guard pattern first"""
    N, S, SHIFT = 4096, 4, 4

    def __init__(self, sc, pinned, keep_state=False, grinding_bits=0):
        self.sc, self.rounds = sc, cases.num_rounds(self.N, 4, self.S)
        rounds, s, N = self.rounds, self.S, self.N
        self.codeword = resident(sc, cases.codeword(N, 4))
        self.extra = resident(sc, cases.codeword(N, 4, seed=9))
        self.extra_tree = self.extra.tree()
        self.depths = [(N >> (j + 1)).bit_length() - 1 for j in range(rounds - 1)]
        self.pair_bytes = (32 * s * (rounds - 1) + 255) & ~255
        self.element_bytes = (16 * 4 * s + 255) & ~255
        self.own_paths = 64 * s * sum(self.depths)
        self.path_bytes = (self.own_paths + 64 * 4 * s * 12 + 255) & ~255
        self.total = s * (rounds - 1) + 4 * s
        self.need = self.pair_bytes + self.element_bytes + self.path_bytes + 8 * self.total
        self.roots = ctypes.create_string_buffer(bytes([GUARD]) * (64 * rounds), 64 * rounds)
        self.last = ctypes.create_string_buffer(bytes([GUARD]) * (16 * (N >> (rounds - 1))), 16 * (N >> (rounds - 1)))
        self.top = (u64 * s)(*[GUARD] * s)
        self.quad = (u64 * (4 * s))(*[GUARD] * (4 * s))
        self.nonce = u64(GUARD)
        self.vecs = (vp * (rounds - 1))() if keep_state else None
        self.trees = (vp * rounds)() if keep_state else None
        self.grinding_bits = grinding_bits
        if pinned:
            self.buffer = sc.HostBuffer(self.need + 4096)
            self.array, self.answers = self.buffer.array, self.buffer.ptr
        else:
            self.array = np.empty(self.need + 4096, dtype=np.uint8)
            self.answers = vp(self.array.ctypes.data)
        self.array[:] = GUARD

    def arguments(self, **changed):
        sc = self.sc
        a = dict(d_codeword=self.codeword.vec.ptr, N=self.N, offset=sc.fe_bytes(G), omega=sc.fe_bytes(cases.root_of_unity(self.N)), rounds=self.rounds,
                 num_tests=self.S, prior_data=b"", prior_lens=(u32 * 1)(), prior_count=0, extra_count=1, extra_trees=(vp * 1)(self.extra_tree._h),
                 extra_vecs=(vp * 1)(self.extra.vec.ptr), extra_shift=self.SHIFT, vecs_out=self.vecs, trees_out=self.trees, roots_out=self.roots,
                 alphas_out=None, last=self.last, top=self.top, quad=self.quad, answers=self.answers, answers_bytes=self.need, stream=None,
                 grinding_bits=self.grinding_bits, nonce_out=ctypes.byref(self.nonce))
        assert set(changed) <= set(a)
        a.update(changed)
        return tuple(a.values())

    def run(self, **changed):
        return self.sc.lib().sc_fri_prove_pairs_dev(*self.arguments(**changed))

    def untouched(self):
        guard = bytes([GUARD])
        return (self.roots.raw == guard * len(self.roots.raw) and self.last.raw == guard * len(self.last.raw) and list(self.top) == [GUARD] * self.S
                and list(self.quad) == [GUARD] * (4 * self.S) and self.nonce.value == GUARD and bool((self.array == GUARD).all())
                and (self.trees is None or not any(self.trees)) and (self.vecs is None or not any(self.vecs)))

    def sections(self):
        s, rounds = self.S, self.rounds
        raw = self.array.tobytes()
        at_paths, at_where = self.pair_bytes + self.element_bytes, self.pair_bytes + self.element_bytes + self.path_bytes
        return dict(pairs=raw[:32 * s * (rounds - 1)], elements=raw[self.pair_bytes:self.pair_bytes + 16 * 4 * s],
                    paths=raw[at_paths:at_paths + self.own_paths], extra_paths=raw[at_paths + self.own_paths:at_paths + self.own_paths + 64 * 4 * s * 12],
                    where=np.frombuffer(raw[at_where:at_where + 8 * self.total], dtype=np.uint64).tolist(), behind=raw[self.need:])


@pytest.mark.parametrize("grinding_bits", (0, 4))
def test_entry_answers(sc, grinding_bits):
    """pinned and ordinary answers: the same contents, the sentinels behind answers_bytes intact; every section against the model"""
    _, top, codewords, roots = model(Call.N, Call.S, grinding_bits)
    calls = [Call(sc, pinned, grinding_bits=grinding_bits) for pinned in (True, False)]
    for call in calls:
        sc._check(call.run())
    direct, staged = (call.sections() for call in calls)
    assert direct == staged
    assert direct["behind"] == bytes([GUARD]) * 4096
    call, s, N, rounds = calls[0], Call.S, Call.N, calls[0].rounds
    assert call.roots.raw == b"".join(roots) and cases.unpack(call.last.raw) == codewords[-1]
    assert list(call.top) == list(top)
    if grinding_bits:
        assert call.nonce.value == pickle.loads(model(N, s, grinding_bits)[0])[rounds + 1]
    else:
        assert call.nonce.value == GUARD
    leaves = [[index % (N >> (j + 1)) for index in top] for j in range(rounds - 1)]
    quad = sorted(p for i in top for p in (i, (i + Call.SHIFT) % N, (i + N // 2) % N, (i + Call.SHIFT + N // 2) % N))
    assert list(call.quad) == quad
    assert direct["where"] == [a for per in leaves for a in per] + quad
    assert direct["pairs"] == b"".join(cases.pack([codewords[j][a], codewords[j][a + (N >> (j + 1))]]) for j in range(rounds - 1) for a in leaves[j])
    assert direct["paths"] == b"".join(b"".join(cases.path(cases.pair_levels(codewords[j]), a)) for j in range(rounds - 1) for a in leaves[j])
    (values, paths), = sc.query_codewords_raw([call.extra], [quad])
    assert direct["elements"] == bytes(values) and direct["extra_paths"] == paths.tobytes()


def test_entry_handles(sc):
    """vecs_out / trees_out given: the folded codewords, and ordinary trees of n_r / 2 leaves that sc_fri_pairs_query_dev and
    sc_merkle_open_batch work on"""
    _, top, codewords, roots = model(Call.N, Call.S, 0)
    call = Call(sc, pinned=True, keep_state=True)
    sc._check(call.run())
    s, N, rounds = Call.S, Call.N, call.rounds
    vectors = [call.codeword.vec] + [sc.DeviceVector.adopt(call.vecs[r], N >> (r + 1)) for r in range(rounds - 1)]
    trees = [sc.MerkleTree(vp(call.trees[r]), call.roots.raw[64 * r:64 * r + 64], N >> (r + 1)) for r in range(rounds)]
    for r in range(rounds):
        assert sc.lib().sc_merkle_leaves(trees[r]._h) == N >> (r + 1)
        assert cases.unpack(vectors[r].to_bytes()) == codewords[r]
    sections = call.sections()
    opened = rounds - 1
    leaves = sections["where"][:s * opened]
    pairs, paths = ctypes.create_string_buffer(32 * s * opened), ctypes.create_string_buffer(call.own_paths)
    sc._check(sc.lib().sc_fri_pairs_query_dev(opened, (vp * opened)(*[t._h for t in trees[:opened]]), (vp * opened)(*[v.ptr for v in vectors[:opened]]),
                                              (u64 * len(leaves))(*leaves), (u64 * opened)(*[s] * opened), pairs, paths))
    assert pairs.raw == sections["pairs"] and paths.raw == sections["paths"]
    last_tree = trees[-1]                                     # the last codeword's pair tree: built, rooted, never opened by the call
    levels = cases.pair_levels(codewords[-1])
    assert last_tree.root == levels[-1][0] == roots[-1]
    opened_paths = ctypes.create_string_buffer(64 * last_tree.depth * 2)
    sc._check(sc.lib().sc_merkle_open_batch(last_tree._h, (u64 * 2)(0, len(levels[0]) - 1), 2, opened_paths))
    assert opened_paths.raw == b"".join(b"".join(cases.path(levels, a)) for a in (0, len(levels[0]) - 1))


@pytest.mark.parametrize("rounds,s", [(5, 2), (5, 4), (6, 1), (6, 2)])
def test_entry_smallest_trees(sc, rounds, s):
    """N = 64 folded down to a last codeword of 4 elements (a pair tree of 2 leaves) and of 2 elements (1 leaf, an empty path) -- shapes the
    entry takes and the tail kernel's pair form must serve although no Fri of expansion factor 4 asks for them: every round in the tail,
    every tree far below one workgroup.  Roots, last codeword and indices against a plain-Python commit loop over cases.pair_levels and
    cases.fold; the pairs and paths against that model and against sc_fri_pairs_query_dev on the trees the call hands out."""
    from algebra import FieldElement
    from fri_pairs_cases import P
    N, field = 64, main_field()
    model, current, offset, omega = ProofStream(), cases.codeword(N, 4), G, cases.root_of_unity(N)
    codewords, levels = [], []
    for r in range(rounds):
        codewords.append(current)
        levels.append(cases.pair_levels(current))
        model.push(levels[-1][-1][0])
        if r + 1 < rounds:
            current = cases.fold(current, int.from_bytes(model.prover_fiat_shamir(), "big") % P, offset, omega)
            omega, offset = omega * omega % P, offset * offset % P
    n_last = N >> (rounds - 1)
    assert len(codewords[-1]) == n_last == (4 if rounds == 5 else 2) and [len(l[0]) for l in levels][-2:] == [n_last, n_last // 2]
    model.push([FieldElement(v, field) for v in codewords[-1]])
    top = cases.sample_indices(model.prover_fiat_shamir(), N // 2, n_last, s)
    opened = rounds - 1
    depths = [(N >> (j + 1)).bit_length() - 1 for j in range(opened)]
    pair_bytes, own_paths = (32 * s * opened + 255) & ~255, 64 * s * sum(depths)
    path_bytes = (own_paths + 255) & ~255
    need = pair_bytes + path_bytes + 8 * s * opened
    codeword = resident(sc, cases.codeword(N, 4))
    buffer = sc.HostBuffer(need + 256)
    buffer.array[:] = GUARD
    roots, last = ctypes.create_string_buffer(64 * rounds), ctypes.create_string_buffer(16 * n_last)
    indices, vecs, trees = (u64 * s)(), (vp * opened)(), (vp * rounds)()
    before = tail_stats(sc)
    sc._check(sc.lib().sc_fri_prove_pairs_dev(codeword.vec.ptr, N, sc.fe_bytes(G), sc.fe_bytes(cases.root_of_unity(N)), rounds, s, b"", (u32 * 1)(), 0,
                                              0, None, None, 0, vecs, trees, roots, None, last, indices, None, buffer.ptr, need, None, 0, None))
    assert tail_stats(sc) == (before[0] + 1, before[1])
    vectors = [codeword.vec] + [sc.DeviceVector.adopt(vecs[r], N >> (r + 1)) for r in range(opened)]
    handles = [sc.MerkleTree(vp(trees[r]), roots.raw[64 * r:64 * r + 64], N >> (r + 1)) for r in range(rounds)]
    assert roots.raw == b"".join(l[-1][0] for l in levels)
    assert cases.unpack(last.raw) == codewords[-1] and list(indices) == top
    for r in range(rounds):
        assert cases.unpack(vectors[r].to_bytes()) == codewords[r] and sc.lib().sc_merkle_leaves(handles[r]._h) == N >> (r + 1)
    raw = buffer.array.tobytes()
    assert raw[need:] == bytes([GUARD]) * 256
    leaves = [[index % (N >> (j + 1)) for index in top] for j in range(opened)]
    assert np.frombuffer(raw[pair_bytes + path_bytes:need], dtype=np.uint64).tolist() == [a for per in leaves for a in per]
    pairs, paths = raw[:32 * s * opened], raw[pair_bytes:pair_bytes + own_paths]
    assert pairs == b"".join(cases.pack([codewords[j][a], codewords[j][a + (N >> (j + 1))]]) for j in range(opened) for a in leaves[j])
    assert paths == b"".join(b"".join(cases.path(levels[j], a)) for j in range(opened) for a in leaves[j])
    again_pairs, again_paths = ctypes.create_string_buffer(32 * s * opened), ctypes.create_string_buffer(own_paths)
    flat = [a for per in leaves for a in per]
    sc._check(sc.lib().sc_fri_pairs_query_dev(opened, (vp * opened)(*[t._h for t in handles[:opened]]), (vp * opened)(*[v.ptr for v in vectors[:opened]]),
                                              (u64 * len(flat))(*flat), (u64 * opened)(*[s] * opened), again_pairs, again_paths))
    assert again_pairs.raw == pairs and again_paths.raw == paths


def test_entry_refusals(sc):
    """every refusal returns its code with nothing written and no launch of the tail kernel"""
    call = Call(sc, pinned=True, keep_state=True)
    before = tail_stats(sc)
    refused = [
        (SC_ERR_NOT_POW2, dict(N=3000)), (SC_ERR_NOT_POW2, dict(N=4096 + 2048)), (SC_ERR_NOT_POW2, dict(rounds=13)),
        (SC_ERR_BAD_ARG, dict(d_codeword=None)), (SC_ERR_BAD_ARG, dict(offset=None)), (SC_ERR_BAD_ARG, dict(omega=None)),
        (SC_ERR_BAD_ARG, dict(roots_out=None)), (SC_ERR_BAD_ARG, dict(last=None)), (SC_ERR_BAD_ARG, dict(top=None)), (SC_ERR_BAD_ARG, dict(answers=None)),
        (SC_ERR_BAD_ARG, dict(extra_trees=None)), (SC_ERR_BAD_ARG, dict(extra_vecs=None)), (SC_ERR_BAD_ARG, dict(quad=None)),
        (SC_ERR_BAD_ARG, dict(extra_trees=(vp * 1)(None))), (SC_ERR_BAD_ARG, dict(prior_count=1, prior_data=None)),
        (SC_ERR_BAD_ARG, dict(num_tests=0)), (SC_ERR_BAD_ARG, dict(num_tests=(Call.N >> (call.rounds - 1)) + 1)),
        (SC_ERR_BAD_ARG, dict(rounds=1)), (SC_ERR_BAD_ARG, dict(rounds=0)), (SC_ERR_BAD_ARG, dict(answers_bytes=call.need - 1)),
        (SC_ERR_BAD_ARG, dict(grinding_bits=-1)), (SC_ERR_BAD_ARG, dict(grinding_bits=64)), (SC_ERR_BAD_ARG, dict(grinding_bits=4, nonce_out=None)),
        (SC_ERR_UNSUPPORTED, dict(prior_count=1, prior_data=bytes(256), prior_lens=(u32 * 1)(256))),
        (SC_ERR_UNSUPPORTED, dict(prior_count=1000, prior_data=bytes(1000), prior_lens=(u32 * 1000)(*[1] * 1000))),
        # rounds + extra_count > 32: eight codewords and 25 further pairs
        (SC_ERR_UNSUPPORTED, dict(extra_count=25, extra_trees=(vp * 25)(*[call.extra_tree._h] * 25), extra_vecs=(vp * 25)(*[call.extra.vec.ptr] * 25))),
    ]
    assert call.rounds == 8
    for code, changed in refused:
        assert call.run(**changed) == code, changed
        assert call.untouched(), changed
    sc.synchronize()
    assert call.untouched() and tail_stats(sc) == before
    # an ordinary host buffer whose answers_bytes is too small, and then the call as it stands
    small = Call(sc, pinned=False)
    assert small.run(answers_bytes=small.need - 1) == SC_ERR_BAD_ARG and small.untouched()
    sc._check(small.run())
    assert not small.untouched() and tail_stats(sc) == (before[0] + 1, before[1])


# ---- FastStark --------------------------------------------------------------------------------------------------------------------------
S = 8


@functools.lru_cache(maxsize=None)
def stark_instance():
    import synth
    import workloads
    from algebra import FieldElement
    from fast_stark import FastStark
    field, T, _, air, boundary = workloads.synthetic_stark_instance(10, S)
    rows = [[FieldElement(a, field), FieldElement(b, field)] for a, b in zip(*synth.synthetic_air_columns(T))]
    plain = FastStark(field, 4, S, 2 * S, 2, T)
    return field, T, rows, air, boundary, plain.preprocess()


@pytest.mark.parametrize("options", ({}, {"row_commitments": True, "grinding_bits": 4}))
def test_fast_stark(sc, seeded, monkeypatch, options):
    """the small synthetic AIR with the route on and off: the same proof, which verifies; with the route on the committed codewords'
    openings arrive in the FRI call -- also_open.answers is set by it and query_codewords_raw is not called at all"""
    from fast_stark import FastStark
    from fri import Fri
    field, T, rows, air, boundary, (tz, tz_codeword, root) = stark_instance()
    stark = FastStark(field, 4, S, 2 * S, 2, T, pair_leaves=True, **options)
    round_trips, seen = [], []
    real_query, real_route = sc.query_codewords_raw, Fri._prove_pairs_in_library

    def counted(*args):
        round_trips.append(len(args[0]))
        return real_query(*args)

    def watched(self, codeword, proof_stream, also_open):
        result = real_route(self, codeword, proof_stream, also_open)
        seen.append((result is not None, also_open is not None and also_open.answers is not None and also_open.position_arrays is not None))
        return result
    monkeypatch.setattr(sc, "query_codewords_raw", counted)
    monkeypatch.setattr(Fri, "_prove_pairs_in_library", watched)
    seeded(83)
    proof = stark.prove([list(r) for r in rows], air, boundary, tz, tz_codeword)
    assert seen == [(True, True)] and round_trips == []
    monkeypatch.setattr(Fri, "PAIRS_IN_LIBRARY", False)
    seeded(83)
    yardstick = stark.prove([list(r) for r in rows], air, boundary, tz, tz_codeword)
    assert seen == [(True, True)] and len(round_trips) == 1
    assert proof == yardstick
    assert stark.verify(proof, air, boundary, root) is True

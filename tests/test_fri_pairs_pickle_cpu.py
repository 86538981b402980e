"""The described query phase of a proof with pair leaves (proof_objects.FriPairsQueryPhase, the 'X' op of csrc/proof_pickle.h) against
CPython's pickle.dumps of the objects it stands for, byte for byte; and the C ABI's new entry in the header, the binding and the built
library.  sc_pickle_proof is host only: runs without a GPU.

The arrays are laid out as sc_fri_prove_pairs_dev lays out its answers: per opened codeword j (2^depth_j pair leaves, 2^(depth_j + 1)
elements) s pairs of 32 bytes, s paths of 64 depth_j bytes and s leaf numbers as uint64, codeword after codeword."""
import ctypes
import os
import pickle
import pickletools
import random
import re

import numpy as np
import pytest

import proof_objects as po_
import starkcore as sc
from algebra import Field, FieldElement
from conftest import PKG, REPO
from ip import ProofStream

MAIN = Field.main()


class Holder:
    """the part of starkcore.DeviceCodeword a segment uses: a field, and entry objects made once per index"""
    _full = None

    def __init__(self, n, field, rng):
        self.field, self.values, self._elems = field, [rng.randrange(field.p) for _ in range(n)], {}

    def raw(self, indices):
        return b"".join(self.values[i].to_bytes(16, "little") for i in indices)

    def _entries(self, indices, values):
        for i, v in zip(indices, values):
            assert v == self.values[i]
            if i not in self._elems:
                self._elems[i] = FieldElement(v, self.field)
        return [self._elems[i] for i in indices]


class Case:
    """`rounds - 1` opened codewords of 2^(depth + 1) elements, s distinct leaves each, random digests"""

    def __init__(self, seed, s, depths):
        rng = random.Random(seed)
        self.s, self.depths = s, list(depths)
        self.holders = [Holder(2 << d, MAIN, rng) for d in depths]
        self.leaves = [rng.sample(range(1 << d), s) for d in depths]
        self.pairs = np.frombuffer(b"".join(h.raw([i for a in leaves for i in (a, a + (1 << d))])
                                            for h, leaves, d in zip(self.holders, self.leaves, depths)), dtype=np.uint8)
        self.path_bytes = [rng.randbytes(64 * d * s) for d in depths]
        self.paths = np.frombuffer(b"".join(self.path_bytes), dtype=np.uint8)
        self.positions = np.asarray([a for leaves in self.leaves for a in leaves], dtype=np.uint64)

    def segment(self, pairs=None, paths=None, positions=None):
        return po_.FriPairsQueryPhase(self.holders, self.s, self.depths, self.pairs if pairs is None else pairs,
                                      self.paths if paths is None else paths, self.positions if positions is None else positions)

    def objects(self):
        """what Fri._prove_pairs pushes: per codeword s tuples of the holders' own entry objects, then s lists of fresh digests"""
        out = []
        for h, leaves, d, raw in zip(self.holders, self.leaves, self.depths, self.path_bytes):
            for a in leaves:
                out.append(tuple(h._entries([a, a + (1 << d)], [h.values[a], h.values[a + (1 << d)]])))
            for t in range(self.s):
                out.append([bytes(bytearray(raw[64 * (d * t + l):64 * (d * t + l + 1)])) for l in range(d)])
        return out


def described(stream):
    """the stream's bytes through the library's pickler -- which must not have materialised anything on the way"""
    lazy = stream.objects
    assert isinstance(lazy, po_.LazyProofObjects)
    got = stream.serialize()
    assert lazy._all is None and not lazy._cache
    return got


def stream_with(case, segment, front=(), behind=()):
    stream = ProofStream()
    for obj in front:
        stream.push(obj)
    lazy = po_.lazy_objects(stream)
    lazy.add(segment)
    for obj in behind:
        lazy.append(obj)
    return stream


@pytest.mark.parametrize("s,depths", [(1, [3]), (1, [1]), (2, [1]), (1, [0]), (2, [5, 4, 3, 2, 1]), (64, [11, 10, 9])])
def test_segment_pickles_like_its_objects(s, depths):
    """one pair and one path (two codewords, s = 1); a pair tree of 2 leaves (paths of one digest) and of 1 leaf (empty paths); the
    signature scheme's shape.  The described bytes, the materialised objects and the objects of the round-by-round route agree."""
    case = Case(11 * s + len(depths), s, depths)
    roots = [random.Random(5).randbytes(64) for _ in range(len(depths) + 1)]
    stream = stream_with(case, case.segment(), front=roots)
    got = described(stream)
    want = pickle.dumps(roots + case.objects())
    assert got == want
    assert len(stream.objects) == len(roots) + 2 * s * len(depths)
    materialised = list(stream.objects)
    assert pickle.dumps(materialised) == want
    expected = case.objects()
    for mine, theirs in zip(materialised[len(roots):], expected):
        assert type(mine) is type(theirs) and mine == theirs
        if type(mine) is tuple:
            assert mine[0] is theirs[0] and mine[1] is theirs[1]          # the holders' own entry objects
    loaded = pickle.loads(got)
    assert [type(o) for o in loaded[len(roots):]] == ([tuple] * s + [list] * s) * len(depths)


def test_memo_numbers_continue_across_the_segment():
    """an ElementList in front (the last codeword) and Openings behind (a committed codeword, one position twice: a memo hit behind
    the segment's own memo entries), with a nonce and a plain path around them"""
    rng = random.Random(21)
    case = Case(22, 5, [4, 3])
    last = Holder(8, MAIN, rng)
    committed = Holder(64, MAIN, rng)
    opened = [3, 9, 9, 40]
    paths = np.frombuffer(rng.randbytes(64 * 6 * len(opened)), dtype=np.uint8).reshape(len(opened), 64 * 6)
    root, loose = rng.randbytes(64), [rng.randbytes(64) for _ in range(3)]
    stream = ProofStream()
    stream.push(root)
    lazy = po_.lazy_objects(stream)
    lazy.add(po_.ElementList(last, last.raw(range(8))))
    lazy.append(12345678901)
    lazy.add(case.segment())
    lazy.add(po_.Openings(committed, opened, committed.raw(opened), paths))
    lazy.append(loose)
    got = described(stream)
    entries = committed._entries(opened, [committed.values[i] for i in opened])
    behind = [x for e, p in zip(entries, paths) for x in (e, [bytes(bytearray(p[64 * l:64 * l + 64])) for l in range(6)])]
    want = pickle.dumps([root, last._entries(range(8), last.values), 12345678901] + case.objects() + behind + [loose])
    assert got == want
    assert pickle.dumps(list(stream.objects)) == want


def frames_inside(blob):
    """(frames that begin inside a pair, frames that begin inside a path) of a pickle whose only tuples are pairs of fresh elements and
    whose only byte strings behind the first frame are path digests"""
    ops = list(pickletools.genops(blob))
    in_pair = in_path = 0
    for k, (op, _, _) in enumerate(ops):
        if op.name != "FRAME" or k < 2:
            continue
        if ops[k + 1][0].name == "SHORT_BINBYTES":
            in_path += 1
            continue
        fresh = 0
        for nxt, _, _ in ops[k + 1:]:
            if nxt.name == "NEWOBJ":
                fresh += 1
            elif nxt.name in ("TUPLE2", "EMPTY_LIST"):
                in_pair += nxt.name == "TUPLE2" and fresh < 2
                break
    return in_pair, in_path


def test_frame_boundaries_inside_pairs_and_paths():
    """192 pairs and 1 920 digests are 140 KiB of pickle: two frame boundaries.  A byte string of growing length in front moves them
    through the second codeword's pairs and paths; every placement pickles as CPython pickles it, and placements of both kinds occur."""
    case = Case(31, 64, [11, 10, 9])
    objects = case.objects()
    pairs = paths = 0
    for lead in range(0, 15000, 97):
        front = [random.Random(lead).randbytes(lead)]
        got = described(stream_with(case, case.segment(), front=front))
        assert got == pickle.dumps(front + objects), lead
        a, b = frames_inside(got)
        pairs, paths = pairs + a, paths + b
    assert pairs > 0 and paths > 0


def test_arrays_that_are_not_contiguous_take_the_fallback():
    """strided views: one op per codeword over contiguous copies; the bytes and the objects are the same"""
    case = Case(41, 4, [5, 4, 2])

    def strided(array):
        wide = np.zeros(2 * len(array), dtype=array.dtype)
        wide[::2] = array
        return wide[::2]
    want = pickle.dumps(case.objects())
    for which in ("pairs", "paths", "positions"):
        segment = case.segment(**{which: strided(getattr(case, which))})
        assert not getattr(segment, which).flags["C_CONTIGUOUS"]
        stream = stream_with(case, segment)
        assert described(stream) == want
        assert pickle.dumps(list(stream.objects)) == want
    everything = case.segment(strided(case.pairs), strided(case.paths), strided(case.positions))
    assert described(stream_with(case, everything)) == want


def test_the_entry_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "starkcore.h")).read(), flags=re.S)
    declaration = re.search(r"\bint\s+sc_fri_prove_pairs_dev\s*\(([^;]*)\)\s*;", header)
    assert declaration is not None
    grind = re.search(r"\bint\s+sc_fri_prove_grind_dev\s*\(([^;]*)\)\s*;", header)
    assert re.sub(r"\s+", " ", declaration.group(1)) == re.sub(r"\s+", " ", grind.group(1))        # the arguments of sc_fri_prove_grind_dev
    assert sc.SIGNATURES["sc_fri_prove_pairs_dev"] == sc.SIGNATURES["sc_fri_prove_grind_dev"]
    library = ctypes.CDLL(os.path.join(PKG, "libstarkcore.so"))
    assert hasattr(library, "sc_fri_prove_pairs_dev")

"""Every kernel that has a Merkle leaf stage, fed tests/leaf_edges.py: residues whose decimal strings have every length from 1 to 39,
zero, all-zero and all-nines base-10^9 groups, limb boundaries, p - 1.  Expected digests are hashlib.blake2b over str(value) and
over left + right (leaf_edges.tree_levels); expected folds are oracle/py_oracle.py's fold in Python integers.  Each test compares
the root and opens paths at the first and last leaf of 1, 20 and 39 characters.

Which test reaches which leaf stage, and why its shape does (stark-anatomy_amd/csrc/merkle_fri.hip, merkle_build_device, with
`constexpr uint64_t FUSE_MAX_W = 1ull << 17;` of csrc/core.h; BIG below is the first power of two above FUSE_MAX_W, 2^18):

  test_leaf_kernel_small_trees            merkle_leaf_kernel (leaf_message), one workgroup: the last branch, N < 256 -- N = 1 (every
                                          edge residue in thread 0), N = 2, N = 128 through sc_merkle_commit / sc_merkle_build
  test_leaf_kernel_many_workgroups        merkle_leaf_kernel, N / 256 workgroups: `else if (N > FUSE_MAX_W)` once merkle_big_nlev = 0
                                          has switched off `N > FUSE_MAX_W && (g.merkle_big_nlev > 0 || fold)`; N = BIG
  test_subtree_four_lane_leaves           merkle_subtree_kernel<true, true> (leaf_message_lds): `N >= 256 && N <= FUSE_MAX_W`;
                                          N = 256, 512, 2^12, and 2^15 = 128 blocks of 256, each rotated one further, so that every
                                          thread index (the LDS slot is 80 bytes * threadIdx.x) converts every edge residue
  test_subtree_one_lane_leaves            merkle_subtree_kernel<true, false>: `N > FUSE_MAX_W && (g.merkle_big_nlev > 0 || fold)`
                                          with the default merkle_big_nlev = 2; N = BIG
  test_fold_fused_leaves                  merkle_subtree_kernel<true, true, true> (folded length 256) and <true, false, true> (BIG):
                                          the same two conditions with `fold` set, which fold_and_build does from `N / 2 >= 256`
  test_fold_fused_slab_leaves             merkle_subtree_kernel<true, true, true> with FoldIn's slab indexing (sc_fri_fold_slab_build_dev,
                                          `leaves >= 256`): 32 x 16 folded leaves
  test_forest_leaves                      forest_climb_kernel<true, FOUR, false>: forest_build's `four = nlev >= 2 && wgs <=
                                          g.forest_four_lane_wgs` (`int forest_four_lane_wgs = 256;` of csrc/core.h, wgs = count * N / 256).
                                          3 trees of 64 and of 512 leaves: four lanes; of 2 leaves (nlev = 1) and of 2^15 leaves (384
                                          workgroups): one lane.  2 and 64 leaves put several trees into one workgroup
  test_forest_fold_fused_leaves           forest_climb_kernel<true, FOUR, true> at the same shapes (sc_fri_fold_forest_dev)
  test_tail_kernel_on_a_periodic_codeword fri_tail_kernel (leaf_message): fri_commit_locked hands over at `n / 2 <= (1ull << TAIL_MAX_LOG)`
                                          (2^16); inside, `quad = logn <= TAIL_QUAD_LOG` (2^14).  N = 2^11: four lanes per leaf from the
                                          first round; N = 2^17: one lane per leaf for 2^16 and 2^15 leaves, four below
  test_verify_kernel_on_edge_leaves       merkle_verify_kernel (leaf_message) through sc_merkle_verify_batch's residue rows
  test_folds_on_degenerate_operands       fri_fold_kernel, fold_element (merkle_subtree_kernel<true, true, true>) and fri_tail_kernel's fold

sc_fri_tail_stats and sc_merkle_forest_stats are asserted, so a tail or forest test cannot pass on a fall-back path."""
import ctypes
import os
import pickle
import re
from hashlib import blake2b, shake_256

import numpy as np
import pytest

import leaf_edges as le
from oracle import py_oracle as po

pytestmark = pytest.mark.gpu
P = po.P
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "stark-anatomy_amd", "csrc")


def _constant(pattern):
    with open(os.path.join(CSRC, "core.h")) as f:
        m = re.search(pattern, f.read())
    assert m, pattern
    return int(m.group(1))


FUSE_MAX_W = 1 << _constant(r"constexpr uint64_t FUSE_MAX_W = 1ull << (\d+);")
FOREST_FOUR_LANE_WGS = _constant(r"int forest_four_lane_wgs = (\d+);")
BIG = max(1 << 17, 1 << FUSE_MAX_W.bit_length())                       # the first power of two above FUSE_MAX_W (2^17 if that is above it)
FOREST_TREES = 3
FOREST_BIG = 1 << (FOREST_FOUR_LANE_WGS * 256 // FOREST_TREES).bit_length()     # the first N with 3 N / 256 > forest_four_lane_wgs
assert BIG > FUSE_MAX_W and BIG // 2 <= FUSE_MAX_W
assert FOREST_TREES * FOREST_BIG // 256 > FOREST_FOUR_LANE_WGS >= FOREST_TREES * 512 // 256


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    starkcore.set_tuning("merkle_big_nlev", 2)


def check_tree(tree, vals, levels, what=None):
    """root and the paths at the first and last leaf of 1, 20 and 39 characters against hashlib"""
    assert tree.root == le.tree_root(levels), what
    idx = le.positions_of_lengths(vals)
    for i, path in zip(idx, tree.open_batch(idx)):
        assert path == le.tree_path(levels, i), (what, i, vals[i])


def tree_of(sc, vals):
    return sc.MerkleTree.from_device(sc.DeviceVector.from_bytes(le.pack(vals)))        # sc_merkle_build_dev


def tail_stats(sc):
    out = (ctypes.c_uint64 * 2)()
    sc._check(sc.lib().sc_fri_tail_stats(out))
    return out[0], out[1]                                                              # launches, launches that gave up


# ---- merkle_leaf_kernel ----------------------------------------------------------------------------------------------------------

def test_leaf_kernel_small_trees(sc):
    lib = sc.lib()
    root = ctypes.create_string_buffer(64)
    for v in le.EDGE_LEAVES:                                                           # N = 1: the root is the leaf digest
        sc._check(lib.sc_merkle_commit(le.pack([v]), 1, root))
        assert root.raw == blake2b(str(v).encode()).digest(), v
    for i in range(0, le.PERIOD, 2):                                                   # N = 2
        pair = le.EDGE_LEAVES[i:i + 2]
        levels = le.tree_levels(pair)
        sc._check(lib.sc_merkle_commit(le.pack(pair), 2, root))
        assert root.raw == le.tree_root(levels), pair
        tree = sc.MerkleTree.from_bytes(le.pack(pair))
        assert tree.open_batch([0, 1]) == [le.tree_path(levels, 0), le.tree_path(levels, 1)], pair
    vals, levels = le.edge_tree(128)                                                   # N = 128
    sc._check(lib.sc_merkle_commit(le.pack(vals), 128, root))
    assert root.raw == le.tree_root(levels) == po.merkle_commit(vals)
    tree = sc.MerkleTree.from_bytes(le.pack(vals))
    check_tree(tree, vals, levels)
    assert tree.open_batch(list(range(128))) == [le.tree_path(levels, i) for i in range(128)]


def test_leaf_kernel_many_workgroups(sc):
    vals, levels = le.edge_tree(BIG)
    try:
        sc.set_tuning("merkle_big_nlev", 0)
        check_tree(tree_of(sc, vals), vals, levels)
    finally:
        sc.set_tuning("merkle_big_nlev", 2)


# ---- merkle_subtree_kernel<true, *> ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [256, 512, 1 << 12, 1 << 15])
def test_subtree_four_lane_leaves(sc, n):
    assert 256 <= n <= FUSE_MAX_W
    vals, levels = le.edge_tree(n)
    check_tree(tree_of(sc, vals), vals, levels, n)


def test_subtree_one_lane_leaves(sc):
    sc.set_tuning("merkle_big_nlev", 2)
    vals, levels = le.edge_tree(BIG)
    check_tree(tree_of(sc, vals), vals, levels)


# ---- the fold fused into the leaf stage ------------------------------------------------------------------------------------------
# in[i] = in[i + N/2] = V[i]: the fold of an equal pair is (2 v) / 2 + 0 * t = v for every alpha (tests/test_leaf_edges.py has
# po.fold confirm it), so the folded codeword is V and the leaf stage hashes edge residues it has just computed.
ALPHAS = (0, 1, P - 1, 0x0123456789ABCDEF0123456789ABCDEF % P)


@pytest.mark.parametrize("half,alphas", [(256, ALPHAS), (BIG, ALPHAS[3:])])
def test_fold_fused_leaves(sc, half, alphas):
    assert half == 256 or half > FUSE_MAX_W
    lib = sc.lib()
    vals, levels = le.edge_tree(half)
    src = sc.DeviceVector.from_bytes(le.pack(vals) * 2)
    omega = po.primitive_nth_root(2 * half)
    for alpha in alphas:
        out = sc.DeviceVector(half)
        h = ctypes.c_void_p()
        sc._check(lib.sc_fri_fold_commit_dev(src.ptr, 2 * half, sc.fe_bytes(alpha), sc.fe_bytes(po.GENERATOR), sc.fe_bytes(omega), out.ptr, ctypes.byref(h), None))
        tree = sc.MerkleTree(h, None, half)
        check_tree(tree, vals, levels, alpha)
        assert out.to_bytes() == le.pack(vals), alpha


def test_fold_fused_slab_leaves(sc):
    rows, cols, R, col_base = 64, 16, 64, 32                     # a rank's slab of a 64 x 64 codeword; partner rows are 32 apart
    leaves = rows // 2 * cols
    vals, levels = le.edge_tree(leaves)
    src = sc.DeviceVector.from_bytes(le.pack(vals) * 2)
    omega = po.primitive_nth_root(rows * R)
    for alpha in ALPHAS[2:]:
        dst = sc.DeviceVector(leaves)
        tree = sc.MerkleTree.from_folded_slab(src.ptr, rows, cols, R, col_base, sc.fe_bytes(alpha), sc.fe_bytes(po.GENERATOR), sc.fe_bytes(omega), dst.ptr, None)
        sc.synchronize()
        assert dst.to_bytes() == le.pack(vals), alpha
        assert tree.n == leaves
        check_tree(tree, vals, levels, alpha)


# ---- forest_climb_kernel<true, *, *> ---------------------------------------------------------------------------------------------

FOREST_SHAPES = [2, 64, 512, FOREST_BIG]


def forest_trees(n):
    """three trees, each another rotation of the edge list; two-leaf trees start at a leaf of 1, of 20 and of 39 characters"""
    starts = (0, 20, 39) if n == 2 else (0, 43, 86)
    assert n != 2 or [len(str(le.EDGE_LEAVES[s])) for s in starts] == [1, 20, 39]
    return [le.edge_tree(n, s) for s in starts]


def check_forest(sc, forest, trees, what):
    assert forest.roots == [le.tree_root(levels) for _, levels in trees], what
    positions = []
    for t, (vals, _) in enumerate(trees):
        positions += [(t, i) for i in ([0, 1] if len(vals) == 2 else le.positions_of_lengths(vals, required=t == 0))]
    elems, paths = forest.query(positions)
    for (t, i), e, path in zip(positions, elems, paths):
        assert e == trees[t][0][i] and path == le.tree_path(trees[t][1], i), (what, t, i)


@pytest.mark.parametrize("n", FOREST_SHAPES)
def test_forest_leaves(sc, n):
    trees = forest_trees(n)
    matrix = sc.CodewordMatrix(FOREST_TREES, n, sc.DeviceVector.from_bytes(b"".join(le.pack(vals) for vals, _ in trees)))
    before = sc.forest_stats()
    forest = sc.MerkleForest.build(matrix)
    check_forest(sc, forest, trees, n)
    after = sc.forest_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (1, FOREST_TREES)


@pytest.mark.parametrize("n", FOREST_SHAPES)
def test_forest_fold_fused_leaves(sc, n):
    """n = the folded length.  Equal pairs: every tree's folded row is its edge leaves whatever its alpha is"""
    trees = forest_trees(n)
    matrix = sc.CodewordMatrix(FOREST_TREES, 2 * n, sc.DeviceVector.from_bytes(b"".join(le.pack(vals) * 2 for vals, _ in trees)))
    omega = po.primitive_nth_root(2 * n)
    roots = []
    for alphas in (ALPHAS[:3], ALPHAS[1:]):
        before = sc.forest_stats()
        forest = sc.MerkleForest.fold_build(matrix, list(alphas), po.GENERATOR, omega)
        check_forest(sc, forest, trees, (n, alphas))
        assert forest.matrix.to_bytes() == b"".join(le.pack(vals) for vals, _ in trees), (n, alphas)
        after = sc.forest_stats()
        assert (after[0] - before[0], after[1] - before[1]) == (1, FOREST_TREES)
        roots.append(forest.roots)
    assert roots[0] == roots[1]


# ---- sc_fri_prove_dev: fri_tail_kernel -------------------------------------------------------------------------------------------

def fold_ref(cw, alpha, offset, omega):
    half = len(cw) // 2
    if cw[:half] == cw[half:]:           # equal pairs fold to themselves (see above); po.fold costs two inversions per element
        return cw[:half]
    return po.fold(cw, alpha, offset, omega)


def prove_and_check(sc, cw0, s):
    """sc_fri_prove_dev (fri.py:115-130) on the codeword cw0 with s colinearity tests, as test_fri_prove_in_one_call_through_the_cabi
    calls it: every root against hashlib trees of po.fold's codewords (alphas recomputed from the transcript, ip.py:18-25), the last
    codeword, the indices, every opened element and every opened path.  Returns the codewords, the alphas and the tail counters' change."""
    from algebra import Field, FieldElement
    lib, field = sc.lib(), Field.main()
    N = len(cw0)
    om, g = po.primitive_nth_root(N), po.GENERATOR
    rounds, length = 0, N
    while length > 4 and length > 4 * s:
        rounds, length = rounds + 1, length // 2
    n_last = N >> (rounds - 1)
    codewords, trees, transcript, alphas, omega, offset = [list(cw0)], [], [], [], om, g
    for r in range(rounds):
        trees.append(le.tree_levels(codewords[-1]))
        transcript.append(le.tree_root(trees[-1]))
        if r + 1 < rounds:
            alphas.append(field.sample(shake_256(pickle.dumps(transcript)).digest(32)).value)
            codewords.append(fold_ref(codewords[-1], alphas[-1], offset, omega))
            omega, offset = omega * omega % P, offset * offset % P
    last = [FieldElement(v, field) for v in codewords[-1]]
    seed = shake_256(pickle.dumps(transcript + [last])).digest(32)
    top, residues, counter = [], set(), 0
    while len(top) < s:
        i = int.from_bytes(blake2b(seed + bytes(counter)).digest(), "big") % (N // 2)
        counter += 1
        if i % n_last not in residues:
            residues.add(i % n_last)
            top.append(i)
    positions, idx, prev = [], list(top), None
    for j in range(rounds):
        half, here = (N >> j) // 2, []
        if j + 1 < rounds:
            idx = [i % half for i in idx]
            here += idx + [i + half for i in idx]
        elif j > 0:
            here += prev
        prev = idx
        positions.append(here)
    counts = [len(p) for p in positions]
    depths = [(N >> j).bit_length() - 1 for j in range(rounds)]
    total = sum(counts)
    el_bytes = (16 * total + 255) & ~255
    path_bytes = sum(64 * c * d for c, d in zip(counts, depths))
    nbytes = el_bytes + path_bytes + 8 * total
    vec = sc.DeviceVector.from_bytes(le.pack(cw0))
    vecs = (ctypes.c_void_p * max(1, rounds - 1))()
    handles = (ctypes.c_void_p * rounds)()
    roots_out = ctypes.create_string_buffer(64 * rounds)
    alphas_out = (ctypes.c_uint64 * max(2, 2 * (rounds - 1)))()
    last_raw = ctypes.create_string_buffer(16 * n_last)
    top_out = (ctypes.c_uint64 * s)()
    pinned = sc.HostBuffer(nbytes)
    before = tail_stats(sc)
    sc._check(lib.sc_fri_prove_dev(vec.ptr, N, sc.fe_bytes(g), sc.fe_bytes(om), rounds, s, b"", (ctypes.c_uint32 * 1)(), 0, 0, None, None, 0,
                                   vecs, handles, roots_out, alphas_out, last_raw, top_out, None, pinned.ptr, nbytes, None))
    after = tail_stats(sc)
    raw = pinned.array.tobytes()
    for r in range(rounds):
        assert roots_out.raw[64 * r:64 * r + 64] == transcript[r], r
    assert [alphas_out[2 * r] | alphas_out[2 * r + 1] << 64 for r in range(rounds - 1)] == alphas
    assert last_raw.raw == le.pack(codewords[-1]) and list(top_out) == top
    where = np.frombuffer(raw[el_bytes + path_bytes:el_bytes + path_bytes + 8 * total], dtype=np.uint64).tolist()
    vo, po_ = 0, el_bytes
    for j, (c, d) in enumerate(zip(counts, depths)):
        assert where[vo:vo + c] == positions[j], j
        for t, i in enumerate(positions[j]):
            assert raw[16 * (vo + t):16 * (vo + t + 1)] == codewords[j][i].to_bytes(16, "little"), (j, t)
            assert raw[po_ + 64 * d * t:po_ + 64 * d * (t + 1)] == b"".join(le.tree_path(trees[j], i)), (j, t)
        vo += c
        po_ += 64 * c * d
    # the device state that was handed out: every codeword, and every tree at the leaves of 1, 20 and 39 characters
    for r in range(rounds):
        tree = sc.MerkleTree(ctypes.c_void_p(handles[r]), transcript[r], N >> r)
        if r > 0:
            assert sc.DeviceVector.adopt(vecs[r - 1], N >> r).to_bytes() == le.pack(codewords[r]), r
        idx = le.positions_of_lengths(codewords[r], required=False) or [0, (N >> r) - 1]
        assert tree.open_batch(idx) == [le.tree_path(trees[r], i) for i in idx], r
    return codewords, alphas, (after[0] - before[0], after[1] - before[1])


@pytest.mark.parametrize("logn", [11, 17])
def test_tail_kernel_on_a_periodic_codeword(sc, logn):
    """cw[i] = V[i mod 128]: every fold down to length 128 pairs equal values, so every round's codeword is V over and over and the tail
    kernel hashes short strings in every round and every workgroup; the rounds below 128 fold unequal pairs (po.fold)."""
    N = 1 << logn
    cw0 = [le.EDGE_LEAVES[i % le.PERIOD] for i in range(N)]
    codewords, alphas, (launches, gave_up) = prove_and_check(sc, cw0, 4)
    assert (launches, gave_up) == (1, 0)
    assert len(codewords[-1]) == 32 and len(codewords) == logn - 4
    for r, cw in enumerate(codewords):
        if len(cw) >= le.PERIOD:
            assert cw == cw0[:len(cw)], r
    assert codewords[-1] != codewords[-2][:32] and codewords[-2] != codewords[-3][:64]              # (unequal pairs below 128)


# ---- merkle_verify_kernel --------------------------------------------------------------------------------------------------------

def test_verify_kernel_on_edge_leaves(sc):
    """for every edge leaf the honest row, and the rows with the neighbouring residues: next to a power of ten the neighbour's string
    has another length, so an error in the length cannot cancel against one in the digits"""
    vals, levels = le.edge_tree(128)
    depth = len(levels) - 1
    digests = b"".join(b"".join(le.tree_path(levels, i)) for i in range(128))
    rows, want = [], []
    for i, v in enumerate(vals):
        for leaf, verdict in ((v, 1), (v + 1, 0), (v - 1, 0)):
            if leaf >= 0:
                rows.append((i, depth * i, leaf))
                want.append(verdict)
    arr = sc.merkle_rows([r[0] for r in rows], [r[1] for r in rows], [0] * len(rows), [depth] * len(rows), [sc.LEAF_RESIDUE] * len(rows),
                         b"".join(r[2].to_bytes(16, "little") for r in rows))
    assert len(rows) == 3 * 128 - 1
    assert sc.merkle_verify_batch(arr, digests, le.tree_root(levels)).tolist() == want


# ---- the fold kernels on degenerate operands -------------------------------------------------------------------------------------

def test_folds_on_degenerate_operands(sc):
    """fri_fold_kernel (sc_fri_fold_dev), fold_element in the fused leaf stage (sc_fri_fold_commit_dev) and the tail kernel's fold
    (sc_fri_prove_dev, with its own Fiat-Shamir alpha) on 256 pairs with equal operands, sum 0, sums of either parity on either side
    of p, 0 against p - 1 and both 0 (leaf_edges.degenerate_fold_pairs) -- against po.fold"""
    lib = sc.lib()
    pairs = le.degenerate_fold_pairs()
    cw = [a for a, _ in pairs] + [b for _, b in pairs]
    N = len(cw)
    assert N == 512
    omega = po.primitive_nth_root(N)
    src = sc.DeviceVector.from_bytes(le.pack(cw))
    for alpha in (0, 1, P - 1):
        want = po.fold(cw, alpha, po.GENERATOR, omega)
        out = sc.DeviceVector(N // 2)
        sc._check(lib.sc_fri_fold_dev(src.ptr, N, sc.fe_bytes(alpha), sc.fe_bytes(po.GENERATOR), sc.fe_bytes(omega), out.ptr, None))
        sc.synchronize()
        assert out.to_bytes() == le.pack(want), alpha
        out2 = sc.DeviceVector(N // 2)
        h = ctypes.c_void_p()
        sc._check(lib.sc_fri_fold_commit_dev(src.ptr, N, sc.fe_bytes(alpha), sc.fe_bytes(po.GENERATOR), sc.fe_bytes(omega), out2.ptr, ctypes.byref(h), None))
        tree = sc.MerkleTree(h, None, N // 2)
        levels = le.tree_levels(want)
        assert tree.root == le.tree_root(levels), alpha
        assert out2.to_bytes() == le.pack(want), alpha
        assert tree.open_batch([0, 255]) == [le.tree_path(levels, 0), le.tree_path(levels, 255)], alpha
    codewords, alphas, (launches, gave_up) = prove_and_check(sc, cw, 4)
    assert (launches, gave_up) == (1, 0)
    assert codewords[1] == po.fold(cw, alphas[0], po.GENERATOR, omega)

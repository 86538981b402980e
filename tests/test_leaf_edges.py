"""tests/leaf_edges.py on the host: the edge list itself, the hashlib tree against the oracle's Merkle functions, and the two
identities tests/test_gpu_leaf_edges.py builds its fold inputs on, confirmed by oracle/py_oracle.py's fold."""
import leaf_edges as le
from oracle import py_oracle as po

P = po.P


def test_edge_leaves_cover_every_length_and_edge():
    assert le.P == P
    vals = le.EDGE_LEAVES
    counts = le.check_edge_leaves(vals)                  # 128 distinct residues below p, string lengths exactly 1..39
    print("EDGE_LEAVES per string length:", " ".join("%d:%d" % kv for kv in sorted(counts.items())))
    assert sum(counts.values()) == 128
    need = [0] + [10 ** k for k in range(39)] + [10 ** k - 1 for k in range(1, 39)]
    need += [10 ** 27, 10 ** 36 - 10 ** 27, 999999999 * (10 ** 9 + 1), 10 ** 18 + 10 ** 9 - 1, 999999999 * 10 ** 9]
    need += [(1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 64, 1 << 96, 1 << 127, P - 1, P - 2]
    assert all(v in vals for v in need)
    assert max(v // 10 ** 36 for v in vals) == (P - 1) // 10 ** 36 == 270 and any(v // 10 ** 36 == 270 and v < P - 2 for v in vals)
    assert sum(1 for k in range(39) if 10 ** k + 1 in vals) >= 30
    groups = lambda v: [v // 10 ** (9 * g) % 10 ** 9 for g in range(5)]
    assert any(groups(v)[1] == 0 and groups(v)[2] == 0 and groups(v)[3] for v in vals)             # zero groups in the middle
    assert any(999999999 in groups(v)[1:] for v in vals) and any(groups(v)[0] == 999999999 for v in vals)
    assert any(groups(v)[4] == 0 and groups(v)[3] for v in vals) and any(groups(v)[4] for v in vals)


def test_rotated_blocks_give_every_thread_every_leaf():
    """2^15 leaves are 128 blocks of 256, each rotated one further: thread t of a workgroup converts every edge residue in some
    block (tests/test_gpu_leaf_edges.py: test_subtree_four_lane_leaves); a rotation changes which tree is built"""
    vals = le.edge_leaves(1 << 15)
    for t in range(256):
        assert {vals[256 * b + t] for b in range(128)} == set(le.EDGE_LEAVES)
    assert le.edge_leaves(512, 0) != le.edge_leaves(512, 43) and le.edge_leaves(256)[128:] == le.EDGE_LEAVES
    vals = le.edge_leaves(256)
    opened = le.positions_of_lengths(vals)
    assert opened[:3] == [0, 20, 39] and len(opened) == 6 and sorted(len(str(vals[i])) for i in opened) == [1, 1, 20, 20, 39, 39]
    assert le.positions_of_lengths([5, 7], required=False) == [0, 1]


def test_hashlib_tree_is_the_oracles():
    for n in (1, 2, 8, 128):
        vals = le.edge_leaves(n, 17)
        levels = le.tree_levels(vals)
        assert le.tree_root(levels) == po.merkle_commit(vals)
        for i in ({0, n - 1, n // 3} if n > 1 else ()):
            assert le.tree_path(levels, i) == po.merkle_open(i, vals)


def test_equal_pairs_fold_to_themselves_and_a_periodic_codeword_stays_periodic():
    g = po.GENERATOR
    vals = le.edge_leaves(128)
    for alpha in (0, 1, P - 1, 0x0123456789ABCDEF0123456789ABCDEF % P):
        assert po.fold(vals + vals, alpha, g, po.primitive_nth_root(256)) == vals
    cw = [le.EDGE_LEAVES[i % 128] for i in range(512)]
    omega, offset = po.primitive_nth_root(512), g
    for alpha in (3, P - 5):
        nxt = po.fold(cw, alpha, offset, omega)
        assert nxt == cw[:len(cw) // 2]
        cw, omega, offset = nxt, omega * omega % P, offset * offset % P
    assert len(cw) == 128 and po.fold(cw, 3, offset, omega) != cw[:64]                            # below the period the pairs differ


def test_degenerate_fold_pairs_cover_the_cases():
    pairs = le.degenerate_fold_pairs()
    assert len(pairs) == 256 and all(0 <= a < P and 0 <= b < P for a, b in pairs)
    sums = {a + b for a, b in pairs}
    assert {0, 1, 2, P - 2, P - 1, P, P + 1, P + 2, 2 * P - 2, 2 * P - 3} <= sums
    assert {(0, 0), (0, P - 1), (P - 1, 0)} <= set(pairs)
    assert sum(1 for a, b in pairs if a == b) >= 30 and sum(1 for a, b in pairs if a + b == P) >= 30
    for lo, hi in ((0, P), (P, 2 * P)):                                                            # either parity on either side of p
        assert {(a + b) % 2 for a, b in pairs if lo < a + b < hi} == {0, 1}

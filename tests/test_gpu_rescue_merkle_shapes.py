"""The Rescue-Prime Merkle kernels (sc_rescue_merkle_*; csrc/rescue_merkle.hip and rescue_merkle.cuh) at every shape the entries
accept and at the long digests that tests/test_gpu_rescue_merkle.py never reaches: the 77 (m, capacity, d) triples of
rescue_merkle_cases.ALL_SHAPES on trees of 8 leaves, and LONG_SHAPES -- node messages whose right child lies across two blocks,
digests as long as the rate, d up to 7 -- on trees of 256 and 2048 leaves: every level, openings, both verifiers past their first
workgroup, subtree items, roots and path words at or above p, 1 and 27 rounds, walks of depth 63, and the Python class at d = 4, 7.

The helpers are those of tests/test_gpu_rescue_merkle.py: results land in guarded windows of sentinels, the inputs' bytes are what
they were.  The reference is the plain-integer model of tests/rescue_merkle_cases.py.  Exact."""
import random

import pytest

import rescue_merkle_cases as mc
import rescue_wide_cases as wc

pytestmark = pytest.mark.gpu

import starkcore as sc                              # noqa: E402
import rescue_prime                                 # noqa: E402
import rescue_merkle                                # noqa: E402
import test_gpu_rescue_merkle as base               # noqa: E402  (Window, HostWindow, Built, verify_call: the helpers, not copies of them)

P = mc.P
ROUNDS = mc.SWEEP_ROUNDS
FORMS = (0, 1 << 40)                                 # the tuning key: one lane per item, one lane per state register
long_shapes = pytest.mark.parametrize("m,capacity,d", mc.LONG_SHAPES)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert sc.device_count() > 0, "no GPU visible"
    sc.init()


@pytest.fixture(autouse=True)
def _restore_key():
    yield
    rescue_merkle.set_split_max_nodes(-1)


def levels_equal(tree, want, note):
    got = tree.levels()
    assert len(got) == len(want), note
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, note + ("level", j, "first node that differs", next(k for k in range(len(w)) if g[k] != w[k]))
    assert tree.root() == want[-1][0], note


def paths_of(levels, rows, indices):
    root = levels[-1][0]
    return [(root, i, mc.path(levels, i), rows[i]) for i in indices]


def every_second_tampered(valid, depth, d):
    """the odd items replaced by one of their single changes, cycling through the changes; the verdicts expected"""
    mixed, want = [], []
    for t, item in enumerate(valid):
        changes = mc.tampered(*item, depth, d)
        mixed.append(changes[(t // 2) % len(changes)][1:] if t % 2 else item)
        want.append(1 - t % 2)
    return mixed, want


@pytest.mark.parametrize("m", range(3, 9))
def test_every_legal_shape(m):
    n, depth = 8, 3
    shapes = [s for s in mc.ALL_SHAPES if s[0] == m]
    assert len(shapes) == m * (m - 1) // 2 - 1
    for _, capacity, d in shapes:
        rate = m - capacity
        for width in (1, rate + 1):
            want = base.as_lists(mc.reference(m, capacity, d, n, width, ROUNDS))
            rows = [list(r) for r in mc.rows(m, n, width)]
            valid = paths_of(want, rows, range(n))
            bad = [c[1:] for c in mc.tampered(*valid[5], depth, d)]
            items = valid + [mc.lift_item(it) for it in valid] + bad
            for key in FORMS:
                note = (capacity, d, width, key)
                rescue_merkle.set_split_max_nodes(key)
                tree = base.Built(m, capacity, d, n, width, n + 3)
                levels_equal(tree, want, note)
                assert tree.open_batch(list(range(n))) == [it[2] for it in valid], note
                tree.free()
                assert base.verify_call(m, capacity, d, items, depth, key) == [1] * 16 + [0] * len(bad), note


def long_levels(m, capacity, d, n, width):
    want = base.as_lists(mc.reference(m, capacity, d, n, width, ROUNDS))
    for key in mc.KEYS:
        rescue_merkle.set_split_max_nodes(key)
        for ld in (n, n + 3):
            tree = base.Built(m, capacity, d, n, width, ld)
            levels_equal(tree, want, (n, width, key, ld))
            tree.free()


@pytest.mark.parametrize("wide_rows", (False, True))
@long_shapes
def test_long_digests_every_level(m, capacity, d, wide_rows):
    rate = m - capacity
    long_levels(m, capacity, d, mc.LONG_N, 3 * rate + 1 if wide_rows else rate + 1)


@pytest.mark.parametrize("m,capacity,d", [(8, 1, 7), (5, 1, 3)])
def test_long_digests_across_workgroups(m, capacity, d):
    """2048 leaves of one element: the split form across many workgroups, the wide form across several; 512: its left corner"""
    for n in (2048, 512):
        long_levels(m, capacity, d, n, 1)


@long_shapes
def test_openings(m, capacity, d):
    n, rate = mc.LONG_N, m - capacity
    want = base.as_lists(mc.reference(m, capacity, d, n, rate + 1, ROUNDS))
    rng = random.Random(0x09E9 + 10 * m + d)
    tree = base.Built(m, capacity, d, n, rate + 1, n)
    for indices in ([n // 2], [(0, n - 1, n // 2, n - 1)[t % 4] for t in range(65)], [rng.randrange(n) for _ in range(257)]):
        assert tree.open_batch(indices) == [mc.path(want, i) for i in indices], len(indices)
    tree.free()


@long_shapes
def test_verification_beyond_one_workgroup(m, capacity, d):
    n, rate, depth = mc.LONG_N, m - capacity, 8
    mds, rc = wc.seeded_params(m, ROUNDS)
    levels = base.as_lists(mc.reference(m, capacity, d, n, rate + 1, ROUNDS))
    rows = [list(r) for r in mc.rows(m, n, rate + 1)]
    rng = random.Random(0x7E51 + 10 * m + d)
    assert 4 * (64 // m) < 257
    for k in (1, 64 // m, 64 // m + 1, 257):
        valid = paths_of(levels, rows, [rng.randrange(n) for _ in range(k)])
        mixed, want = every_second_tampered(valid, depth, d)
        if k == 64 // m + 1:                # the model agrees on which items a change has spoilt
            assert [int(mc.verify(*it, m, rate, d, mds, rc, ROUNDS)) for it in mixed[:6]] == want[:6]
        for key in FORMS:
            assert base.verify_call(m, capacity, d, valid, depth, key) == [1] * k, (k, key)
            assert base.verify_call(m, capacity, d, mixed, depth, key) == want, (k, key)


@long_shapes
def test_subtree_and_lifted_items(m, capacity, d):
    """items of depth 3 under distinct roots; the same with every root and path word that has a twin at or above p replaced by it
    (tests/test_rescue_merkle_shapes_cpu.py: at least 4 such root words and 4 such path words per batch); one such root word moved"""
    items = mc.lifted_batch(m, capacity, d)
    up = [mc.lift_item(it) for it in items]
    assert min(mc.lifted_words(up)) >= 4 and len(items) == 64 // m + 1
    bumped = mc.bumped_roots(up)
    for key in FORMS:
        assert base.verify_call(m, capacity, d, items, mc.SUBTREE_DEPTH, key) == [1] * len(items), key
        assert base.verify_call(m, capacity, d, up, mc.SUBTREE_DEPTH, key) == [1] * len(items), key
        assert base.verify_call(m, capacity, d, bumped, mc.SUBTREE_DEPTH, key) == [1 - t % 2 for t in range(len(items))], key


@pytest.mark.parametrize("rounds", (1, 27))
@pytest.mark.parametrize("m,capacity,d", [(8, 1, 4), (3, 1, 2)])
def test_rounds(m, capacity, d, rounds):
    n, rate, depth = 16, m - capacity, 4
    mds, rc = wc.seeded_params(m, rounds)
    rows = [list(r) for r in mc.rows(m, n, rate + 1)]
    want = mc.build(rows, m, rate, d, mds, rc, rounds)
    valid = paths_of(want, rows, range(n))
    bad = [c[1:] for c in mc.tampered(*valid[5], depth, d)]
    for key in FORMS:
        rescue_merkle.set_split_max_nodes(key)
        tree = base.Built(m, capacity, d, n, rate + 1, n + 3, rounds=rounds)
        levels_equal(tree, want, (rounds, key))
        tree.free()
        assert base.verify_call(m, capacity, d, valid + bad, depth, key, rounds=rounds) == [1] * n + [0] * len(bad), (rounds, key)


@pytest.mark.parametrize("m,capacity,d", [(8, 1, 4), (3, 1, 2)])
def test_depth_63(m, capacity, d):
    root, index, pth, row = mc.deep_walk(m, m - capacity, d, mc.DEEP_DEPTH, 0)
    assert index >> 62 == 1
    items = [(root, index, pth, row), (root, index ^ (1 << 62), pth, row), (root, index ^ 1, pth, row)]
    for key in FORMS:
        assert base.verify_call(m, capacity, d, items, mc.DEEP_DEPTH, key) == [1, 0, 0], key


@pytest.mark.parametrize("d", (4, 7))
def test_python_class(d):
    rp = rescue_prime.RescuePrime(m=8, capacity=1, rounds=2)
    tree = rescue_merkle.RescueMerkle(rp, digest_len=d)
    rows = [list(r) for r in mc.rows(8, 8, 8)]
    levels = tree.levels(rows)
    assert tree.commit_rows(rows) == tree.commit(rows) == levels[-1][0]
    paths = tree.open_rows([0, 7, 7], rows)
    assert paths == [tree.open(i, rows) for i in (0, 7, 7)]
    built = tree._rows_device(rows)
    assert built.leaves == 8 and built.depth == 3
    for j in range(4):
        assert built.level(j) == levels[j], j
    root = levels[-1][0]
    valid = [(root, i, mc.path(levels, i), rows[i]) for i in (0, 7, 7, 3)]
    wrong = [(root, 7, paths[1], rows[6]), (root, 0, paths[0], rows[0][:-1] + [rows[0][-1] ^ 1])]
    up = [mc.lift_item(it) for it in valid]
    assert min(mc.lifted_words(up)) >= 1
    items = valid + wrong + up
    want = [tree.verify(*it) for it in items]
    assert want == [True] * 4 + [False] * 2 + [True] * 4
    for key in FORMS:
        rescue_merkle.set_split_max_nodes(key)
        assert tree.verify_batch(*[[it[c] for it in items] for c in range(4)]) == want, key

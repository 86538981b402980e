"""The Rescue-Prime Merkle tree's lane functions (csrc/rescue_merkle.cuh through tests/emu/rescue_merkle_emu.cpp, built by g++) at
every legal shape and at the long digests, without a GPU: the 77 (m, capacity, d) triples of rescue_merkle_cases.ALL_SHAPES on trees
of 8 leaves, LONG_SHAPES on trees of 16 leaves at 1, 2 and 27 rounds, both forms, build and verify, against the plain-integer model;
roots and path words at or above p; and the checks of the cases themselves that tests/test_gpu_rescue_merkle_shapes.py relies on."""
import pytest

import rescue_prime
import rescue_merkle
import rescue_merkle_cases as mc
import rescue_wide_cases as wc
from test_rescue_merkle_cpu import emu, emu_levels, emu_verify, model_of            # noqa: F401  (emu: the fixture that builds the library)

P = mc.P


def items_of(levels, rows, d, leaf=5):
    """every path of a tree, the same items with roots and paths lifted, and the single changes of `leaf`'s item"""
    n, root = len(rows), levels[-1][0]
    valid = [(root, i, mc.path(levels, i), rows[i]) for i in range(n)]
    bad = [c[1:] for c in mc.tampered(*valid[leaf], n.bit_length() - 1, d)]
    return valid + [mc.lift_item(it) for it in valid], bad


@pytest.mark.parametrize("m,capacity,d", mc.ALL_SHAPES)
def test_every_legal_shape(emu, m, capacity, d):
    n, rate, rounds = 8, m - capacity, mc.SWEEP_ROUNDS
    mds, rc = wc.seeded_params(m, rounds)
    params = wc.params_bytes(mds, rc)
    for width in (1, rate + 1):
        rows = [list(r) for r in mc.rows(m, n, width)]
        want = mc.build(rows, m, rate, d, mds, rc, rounds)
        good, bad = items_of(want, rows, d)
        for split in (0, 1):
            got = emu_levels(emu, m, rows, n + 3, d, rate, params, rounds, split)
            for j, (g, w) in enumerate(zip(got, want)):
                assert g == w, (width, split, "level", j)
            assert len(got) == len(want)
            assert emu_verify(emu, m, good + bad, 3, d, rate, params, rounds, split) == [1] * 16 + [0] * len(bad), (width, split)


@pytest.mark.parametrize("rounds", (1, 2, 27))
@pytest.mark.parametrize("m,capacity,d", mc.LONG_SHAPES)
def test_long_digests(emu, m, capacity, d, rounds):
    n, rate = 16, m - capacity
    mds, rc = wc.seeded_params(m, rounds)
    params = wc.params_bytes(mds, rc)
    rows = [list(r) for r in mc.rows(m, n, rate + 1)]
    want = mc.build(rows, m, rate, d, mds, rc, rounds)
    good, bad = items_of(want, rows, d)
    for split in (0, 1):
        assert emu_levels(emu, m, rows, n + 3, d, rate, params, rounds, split) == want, split
        assert emu_verify(emu, m, good + bad, 4, d, rate, params, rounds, split) == [1] * 32 + [0] * len(bad), split


# ---- the cases themselves -----------------------------------------------------------------------------------------------------------

def test_shape_lists():
    legal = [(m, m - rate, d) for m in range(3, 9) for rate in range(2, m) for d in range(1, rate + 1)]
    assert len(mc.ALL_SHAPES) == 77 and sorted(mc.ALL_SHAPES) == sorted(set(legal))
    assert set(mc.SHAPES) <= set(mc.ALL_SHAPES) and set(mc.LONG_SHAPES) <= set(mc.ALL_SHAPES)
    assert all(d >= 3 or d == m - capacity for m, capacity, d in mc.LONG_SHAPES)
    assert [mc.straddles(m - capacity, d) for m, capacity, d in mc.LONG_SHAPES] == [True] * 4 + [False] * 2
    assert not any(mc.straddles(m - capacity, d) for m, capacity, d in mc.SHAPES)
    for (m, capacity, d), blocks in zip(mc.LONG_SHAPES, (2, 2, 2, 2, 3, 3)):
        rate = m - capacity
        padded = wc.pad(list(range(2, 2 * d + 2)), rate)
        assert len(padded) // rate == blocks == mc.node_blocks(rate, d)
        # a straddling message: the right child begins inside block 0 and ends in block 1, and the padding's 1 is not a block's first element
        assert mc.straddles(rate, d) == (d % rate != 0 and d // rate == 0 and (2 * d - 1) // rate == 1 and (2 * d) % rate != 0)


def test_lifted():
    assert mc.lifted(0) == P and mc.lifted(1) == P + 1 and mc.lifted(P - 1) == P - 1
    top = (1 << 128) - 1 - P
    assert mc.lifted(top) == (1 << 128) - 1 and mc.lifted(top + 1) == top + 1
    for v in (0, 1, top, top + 1, P - 1):
        assert mc.lifted(v) % P == v and mc.lifted(v) < 1 << 128


@pytest.mark.parametrize("m,capacity,d", mc.LONG_SHAPES)
def test_the_lifted_batch_holds_lifted_words(m, capacity, d):
    """what keeps the GPU test of lifted items from passing without a lifted word: at least 4 root words and 4 path words at or
    above p, distinct roots, and the model's verdicts"""
    rate = m - capacity
    mds, rc = wc.seeded_params(m, mc.SWEEP_ROUNDS)
    items = mc.lifted_batch(m, capacity, d)
    assert len(items) == 64 // m + 1 and len({tuple(it[0]) for it in items}) == len(items)
    assert all(len(it[2]) == mc.SUBTREE_DEPTH and it[1] < 1 << mc.SUBTREE_DEPTH for it in items)
    assert mc.lifted_words(items) == (0, 0)
    up = [mc.lift_item(it) for it in items]
    root_words, path_words = mc.lifted_words(up)
    print("lifted batch of", (m, capacity, d), ":", root_words, "root words and", path_words, "path words at or above p")
    assert root_words >= 4 and path_words >= 4
    bumped = mc.bumped_roots(up)
    for t in range(4):
        assert mc.verify(*items[t], m, rate, d, mds, rc, mc.SWEEP_ROUNDS) and mc.verify(*up[t], m, rate, d, mds, rc, mc.SWEEP_ROUNDS)
        assert mc.verify(*bumped[t], m, rate, d, mds, rc, mc.SWEEP_ROUNDS) == (t % 2 == 0)


@pytest.mark.parametrize("m,capacity,d", [(8, 1, 4), (3, 1, 2)])
def test_model_and_host_class_agree_on_lifted_and_tampered_items(m, capacity, d):
    rp = rescue_prime.RescuePrime(m=m, capacity=capacity, rounds=2)
    mds, rc = model_of(rp)
    rate = m - capacity
    tree = rescue_merkle.RescueMerkle(rp, digest_len=d)
    rows = [list(r) for r in mc.rows(m, 8, rate + 1)]
    levels = mc.build(rows, m, rate, d, mds, rc, 2)
    subtrees = [mc.subtree_item(levels, 2, i, rows[i]) for i in (1, 6)]
    up = [mc.lift_item((levels[-1][0], i, mc.path(levels, i), rows[i])) for i in range(4)] + [mc.lift_item(it) for it in subtrees]
    assert sum(mc.lifted_words(up)) >= 6
    changes = mc.tampered(*up[3], 3, d)
    bad = [changes[(5 * t) % len(changes)][1:] for t in range(6)]
    for want, items in ((True, up), (False, bad)):
        for it in items:
            assert mc.verify(*it, m, rate, d, mds, rc, 2) is want and tree.verify(*it) is want


@pytest.mark.parametrize("m,capacity,d", [(8, 1, 4), (3, 1, 2)])
def test_deep_walk(m, capacity, d):
    rate = m - capacity
    mds, rc = wc.seeded_params(m, mc.SWEEP_ROUNDS)
    root, index, pth, row = mc.deep_walk(m, rate, d, mc.DEEP_DEPTH, 0)
    assert len(pth) == 63 and all(len(s) == d for s in pth) and index >> 62 == 1 and len(row) == rate + 1
    assert {v for s in pth for v in s} >= set(mc.EDGES)
    assert mc.verify(root, index, pth, row, m, rate, d, mds, rc, mc.SWEEP_ROUNDS)
    assert not mc.verify(root, index ^ (1 << 62), pth, row, m, rate, d, mds, rc, mc.SWEEP_ROUNDS)
    assert not mc.verify(root, index ^ 1, pth, row, m, rate, d, mds, rc, mc.SWEEP_ROUNDS)

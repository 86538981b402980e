"""The plain-integer model and the cases of the Rescue-Prime Merkle tree (sc_rescue_merkle_*; stark-anatomy_amd/csrc/rescue_merkle.cuh
and rescue_merkle.hip, stark-anatomy_amd/rescue_merkle.py).  tests/test_rescue_merkle_cpu.py runs them against the host class and a
g++ build of the kernels' lane functions, tests/test_gpu_rescue_merkle.py against the kernels: both at SHAPES, digests of one or two
elements.  tests/test_rescue_merkle_shapes_cpu.py and tests/test_gpu_rescue_merkle_shapes.py take the same code through every legal
shape (ALL_SHAPES) and, at size, through the long digests (LONG_SHAPES).  The model stands on tests/rescue_wide_cases.py's `sponge`
(Python integers through `pow`), not on the package's rescue_prime.py.

The tree: leaf(row) = sponge(row, out_len = d), node(l, r) = sponge(l + r, out_len = d); level j has N >> j nodes; path[j] is node
(index >> j) ^ 1 of level j."""
import functools
import random

import rescue_wide_cases as wc

P, EDGES = wc.P, wc.EDGES
# (m, capacity, d): two blocks per node, one, three, one; then every other width at capacity 1, d = 1
SHAPES = ((3, 1, 1), (4, 1, 1), (4, 2, 2), (8, 3, 2), (5, 1, 1), (6, 1, 1), (7, 1, 1))
SIZES = (1, 2, 4, 256, 512, 2048)
SWEEP_ROUNDS = 2
KEYS = (0, 1 << 40, 8)                            # the tuning key: wide everywhere, split everywhere, mixed


def leaf_widths(rate):
    return sorted({1, rate - 1, rate, rate + 1, 3 * rate + 1} - {0})


def node_blocks(rate, d):
    return 2 * d // rate + 1


def tree_cases(rate):
    """(N, leaf width) of the GPU sweep: every leaf width of leaf_widths on the trees of 1, 2, 4 and 256 leaves.  The model is Python
    integers (0.1 .. 0.7 ms per permutation), so the trees of 512 and 2048 leaves, which are there for the grid (a wide level
    across workgroups, a split level across many), take rows of one element: the leaf kernels' paths through the block loop and
    the padding are the same at every size (DEEP_CASE below adds rows of several elements at 2048 leaves for one shape)"""
    return [(n, w) for n in (1, 2, 4, 256) for w in leaf_widths(rate)] + [(512, 1), (2048, 1)]


# One shape also takes the tree of 2048 leaves with rows of rate + 1 elements (two blocks per leaf, two per node, a width that
# leaves tail lanes in every wave): a leaf of several blocks in the split form across many workgroups, and paths of depth 11 from
# rows of several elements through both verifiers.
DEEP_SHAPE = (3, 1, 1)
DEEP_CASE = (2048, 3)

# Every (m, capacity, d) the entries accept: m = 3 .. 8, rate = 2 .. m - 1, d = 1 .. rate
ALL_SHAPES = tuple((m, m - rate, d) for m in range(3, 9) for rate in range(2, m) for d in range(1, rate + 1))
assert len(ALL_SHAPES) == 77
# The long digests, each with its padded node message (l, r: the children's digests; | between blocks):
LONG_SHAPES = (
    (8, 1, 4),      # l0 l1 l2 l3 r0 r1 r2 | r3 1 0 0 0 0 0: the child boundary inside block 0, the right child across the blocks, widest state
    (5, 1, 3),      # l0 l1 l2 r0 | r1 r2 1 0: the same, 12 items and 4 idle tail lanes per wave
    (7, 1, 5),      # l0 l1 l2 l3 l4 r0 | r1 r2 r3 r4 1 0: the same, 9 items per wave and 1 tail lane
    (6, 1, 4),      # l0 l1 l2 l3 r0 | r1 r2 r3 1 0: the same
    (8, 1, 7),      # l0 .. l6 | r0 .. r6 | 1 0 0 0 0 0 0: d = rate, the digest is the whole rate, boundaries aligned
    (3, 1, 2),      # l0 l1 | r0 r1 | 1 0: d = rate at the narrowest state, 21 items per wave
)
LONG_N = 256                                      # the tree the long shapes' openings, batches and subtree items come from
DEEP_DEPTH = 63                                   # the deepest walk the verifier accepts


def straddles(rate, d):
    """whether a node message has its child boundary inside a block and its right child across two blocks"""
    return d % rate != 0 and 2 * d > rate


@functools.lru_cache(maxsize=None)
def rows(m, n, width):
    """n rows of `width` words below 2^128: the first n of one seeded sequence per (m, width), so that a smaller tree is the left
    corner of a larger one.  From 8 rows on, row 5 c + e (mod n) carries EDGES[e] in position c: every edge in every position.
    Fewer rows are edge words throughout: row r carries EDGES[(r + c) mod 5] in position c"""
    rng = random.Random(0x7EE + 1000 * m + 10 * width)
    out = [[rng.randrange(1 << 128) for _ in range(width)] for _ in range(n)]
    for c in range(width):
        if n < 8:
            for r in range(n):
                out[r][c] = EDGES[(r + c) % len(EDGES)]
        else:
            for e, edge in enumerate(EDGES):
                out[(len(EDGES) * c + e) % n][c] = edge
    return tuple(tuple(r) for r in out)


def digest(message, m, rate, d, mds, rc, rounds):
    return wc.sponge(list(message), m, rate, mds, rc, rounds, d)


def build(row_list, m, rate, d, mds, rc, rounds):
    """every level, the leaves' digests first, [root] last; a digest is a list of d integers"""
    levels = [[digest(r, m, rate, d, mds, rc, rounds) for r in row_list]]
    while len(levels[-1]) > 1:
        below = levels[-1]
        levels.append([digest(below[i] + below[i + 1], m, rate, d, mds, rc, rounds) for i in range(0, len(below), 2)])
    return levels


def path(levels, index):
    return [level[(index >> j) ^ 1] for j, level in enumerate(levels[:-1])]


def fold(index, pth, row, m, rate, d, mds, rc, rounds):
    """the digest a walk reaches from `row` along `pth`: bit j of the index says whether it reaches level j from the right"""
    node = digest(row, m, rate, d, mds, rc, rounds)
    for sibling in pth:
        sibling = [v % P for v in sibling]
        node = digest(node + sibling if index % 2 == 0 else sibling + node, m, rate, d, mds, rc, rounds)
        index >>= 1
    return node


def verify(root, index, pth, row, m, rate, d, mds, rc, rounds):
    return [v % P for v in root] == fold(index, pth, row, m, rate, d, mds, rc, rounds)


@functools.lru_cache(maxsize=None)
def reference(m, capacity, d, n, width, rounds):
    """the levels of the tree over rows(m, n, width) under wide_cases' seeded constants: computed once, shared, never changed"""
    if n == 512 and rows(m, 2048, width)[:n] == rows(m, n, width):           # the left corner of the tree of 2048 leaves
        big = reference(m, capacity, d, 2048, width, rounds)
        return tuple(level[:n >> j] for j, level in enumerate(big[:n.bit_length()]))
    mds, rc = wc.seeded_params(m, rounds)
    return tuple(tuple(tuple(dg) for dg in level) for level in build([list(r) for r in rows(m, n, width)], m, m - capacity, d, mds, rc, rounds))


def level_words(level, d):
    """a level as the device keeps it: element e of node k at e * len(level) + k"""
    return [node[e] for e in range(d) for node in level]


def tampered(root, index, pth, row, depth, d):
    """the single changes that must each turn a valid item invalid: (label, root, index, path, row).  A changed word moves by one
    mod 2^128 (never by a multiple of p)"""
    bump = lambda v: (v + 1) % (1 << 128)
    out = []
    for e in range(d):
        r = list(root); r[e] = bump(r[e])
        out.append(("root word %d" % e, r, index, pth, row))
    for j in range(depth):
        q = [list(s) for s in pth]; q[j][(j + index) % d] = bump(q[j][(j + index) % d])
        out.append(("path level %d" % j, root, index, q, row))
    for c in sorted({0, len(row) - 1}):
        w = list(row); w[c] = bump(w[c])
        out.append(("row element %d" % c, root, index, pth, w))
    for j in range(depth):
        out.append(("index bit %d" % j, root, index ^ (1 << j), pth, row))
    return out


# ---- items beyond the paths of one tree ---------------------------------------------------------------------------------------------

def subtree_item(levels, j, index, row):
    """node (index >> j) of level j is the root of the tree over leaves (k << j) .. ((k + 1) << j) - 1: a valid item of depth j
    for the leaf `index` under it.  One tree gives many valid items of one depth with different roots"""
    return (levels[j][index >> j], index & ((1 << j) - 1), path(levels, index)[:j], row)


def lifted(word):
    """the same residue as a word at or above p, where one exists below 2^128 (about a quarter of the residues); else the word"""
    return word + P if word + P < (1 << 128) else word


def lift_item(item):
    """the item with every root and path word lifted: the same verdict (the model's % P, RescueMerkle.verify's _values)"""
    root, index, pth, row = item
    return ([lifted(v) for v in root], index, [[lifted(v) for v in s] for s in pth], row)


def lifted_words(items):
    """(root words, path words) at or above p in a batch"""
    return (sum(v >= P for it in items for v in it[0]), sum(v >= P for it in items for s in it[2] for v in s))


SUBTREE_DEPTH = 3


def lifted_batch(m, capacity, d):
    """64 // m + 1 subtree items of depth SUBTREE_DEPTH with distinct roots from the tree of LONG_N leaves (rows of rate + 1
    elements), canonical.  The roots are the nodes of level SUBTREE_DEPTH with the most words that `lifted` moves, each with the
    leaf under it whose path has the most such words: chosen, not left to chance"""
    rate = m - capacity
    levels = [[list(dg) for dg in level] for level in reference(m, capacity, d, LONG_N, rate + 1, SWEEP_ROUNDS)]
    row_list = rows(m, LONG_N, rate + 1)
    moved = lambda words: sum(lifted(v) != v for v in words)
    best = []
    for k in range(LONG_N >> SUBTREE_DEPTH):
        leaves = range(k << SUBTREE_DEPTH, (k + 1) << SUBTREE_DEPTH)
        index = max(leaves, key=lambda i: (moved(v for s in path(levels, i)[:SUBTREE_DEPTH] for v in s), -i))
        best.append((moved(levels[SUBTREE_DEPTH][k]), moved(v for s in path(levels, index)[:SUBTREE_DEPTH] for v in s), -k, index))
    best.sort(reverse=True)
    return [subtree_item(levels, SUBTREE_DEPTH, index, list(row_list[index])) for _, _, _, index in best[:64 // m + 1]]


def bumped_roots(items):
    """every second item (the odd ones) with one root word moved by one mod 2^128 -- a word at or above p where the root has one"""
    out = []
    for t, (root, index, pth, row) in enumerate(items):
        if t % 2:
            e = next((e for e, v in enumerate(root) if v >= P), 0)
            root = list(root)
            root[e] = (root[e] + 1) % (1 << 128)
        out.append((root, index, pth, row))
    return out


@functools.lru_cache(maxsize=None)
def deep_walk(m, rate, d, depth, seed, rounds=SWEEP_ROUNDS):
    """(root, index, path, row) of a walk of `depth` levels without a tree: a seeded row of rate + 1 words, `depth` seeded siblings
    (words below 2^128, the EDGES among them: sibling j carries EDGES[j mod 5] in element j mod d), a seeded index with bit
    depth - 1 set, and the root `verify`'s own fold reaches from them"""
    rng = random.Random(0xDEE9 + 1000 * seed + 100 * m + 10 * rate + d)
    row = [rng.randrange(1 << 128) for _ in range(rate + 1)]
    pth = [[rng.randrange(1 << 128) for _ in range(d)] for _ in range(depth)]
    for j in range(depth):
        pth[j][j % d] = EDGES[j % len(EDGES)]
    index = rng.randrange(1 << depth) | (1 << (depth - 1))
    mds, rc = wc.seeded_params(m, rounds)
    return (fold(index, pth, row, m, rate, d, mds, rc, rounds), index, pth, row)

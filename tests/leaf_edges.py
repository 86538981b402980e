"""Edge residues for the Merkle leaf stages, and the plainest reference of the trees over them.

A leaf is BLAKE2b-512(str(value)) (merkle.py:14, algebra.py:56-57), so every leaf stage on the device writes a residue as a decimal
string of 1 to 39 characters first.  EDGE_LEAVES holds the 128 residues at which that conversion can go wrong: every string length,
zero, base-10^9 groups that are all zeros or all nines, an empty top group, the 32-bit limb boundaries, the largest residues.
tests/test_leaf_edges.py checks the list on the host; tests/test_gpu_leaf_edges.py and test_merkle (tests/test_gpu_cabi.py) feed
it to every kernel that has a leaf stage.

The reference here is hashlib over Python's str() and nothing else: no digit code of the C oracle or of the library."""
from hashlib import blake2b

P = 1 + 407 * (1 << 119)
G9 = 10 ** 9                                    # the leaf stages convert in base-10^9 groups (csrc/merkle.cuh)


def _edge_leaves():
    vals = []

    def add(*more):
        for v in more:
            if v not in vals:
                vals.append(v)
    add(0)
    add(*[10 ** k for k in range(39)])
    add(*[10 ** k - 1 for k in range(1, 39)])
    add(10 ** 27,                               # an all-zero middle: groups 1, 0, 0, 0 (already there as a power of ten)
        10 ** 36 - 10 ** 27,                    # groups 999999999, 0, 0, 0 under an empty top group
        (G9 - 1) * (G9 + 1),                    # two groups of nines (= 10^18 - 1, already there)
        10 ** 18 + G9 - 1,                      # 1, 0, 999999999
        (G9 - 1) * G9)                          # nines above a zero group
    add((1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 64, 1 << 96, 1 << 127)
    add(P - 1, P - 2,
        270 * 10 ** 36 + 10 ** 27 + (G9 - 1))   # the largest top group a residue has (p = 270 497 897 142 ...), zero groups under it
    k = 0
    while len(vals) < 128:                      # 10^k + 1 while there is room
        add(10 ** k + 1)
        k += 1
    return vals


EDGE_LEAVES = _edge_leaves()
PERIOD = len(EDGE_LEAVES)
OPENED_LENGTHS = (1, 20, 39)                    # every test opens paths at leaves whose strings have these lengths


def check_edge_leaves(vals=EDGE_LEAVES):
    """what the tests rely on; returns {string length: how many values}"""
    assert len(vals) == 128 and len(set(vals)) == 128
    assert all(0 <= v < P for v in vals)
    counts = {}
    for v in vals:
        counts[len(str(v))] = counts.get(len(str(v)), 0) + 1
    assert sorted(counts) == list(range(1, 40)), sorted(counts)
    return counts


check_edge_leaves()


def edge_leaves(n, start=0):
    """n leaves: EDGE_LEAVES over and over, each block of 256 (a workgroup of the tree kernels) rotated one further than the block
    before it, the first by `start` -- leaf i is EDGE_LEAVES[(i + start + i // 256) % 128]"""
    return [EDGE_LEAVES[(i + start + (i >> 8)) % PERIOD] for i in range(n)]


def positions_of_lengths(vals, lengths=OPENED_LENGTHS, required=True):
    """the first and the last position of a leaf of each of `lengths` characters (required: every length must occur)"""
    out = []
    for want in lengths:
        hits = [i for i, v in enumerate(vals) if len(str(v)) == want]
        assert hits or not required, want
        out += hits[:1] + hits[-1:]
    return sorted(set(out))


_LEAF = {}


def leaf_digest(v):
    d = _LEAF.get(v)
    if d is None:
        d = _LEAF[v] = blake2b(str(v).encode()).digest()
    return d


def tree_levels(vals):
    """Merkle.commit (merkle.py:6-14) level by level: [leaf digests, their parents, ..., [root]]"""
    level = [leaf_digest(v) for v in vals]
    assert level and len(level) & (len(level) - 1) == 0
    levels = [level]
    while len(level) > 1:
        level = [blake2b(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
        levels.append(level)
    return levels


def tree_root(levels):
    return levels[-1][0]


def tree_path(levels, index):
    """Merkle.open (merkle.py:16-27): the siblings from the leaf level up"""
    return [levels[l][(index >> l) ^ 1] for l in range(len(levels) - 1)]


_TREES = {}


def edge_tree(n, start=0):
    """(values, levels) of the tree over edge_leaves(n, start); computed once per shape, never modified"""
    key = (n, start)
    if key not in _TREES:
        vals = edge_leaves(n, start)
        _TREES[key] = (vals, tree_levels(vals))
    return _TREES[key]


def pack(vals):
    return b"".join(v.to_bytes(16, "little") for v in vals)


def degenerate_fold_pairs():
    """256 pairs (a, b) = (in[i], in[i + 256]) of a length-512 fold input at which (a + b) / 2 + (a - b) t can go wrong: equal operands, sum 0
    mod p, sums that are odd and even on either side of p (the halving adds p to an odd sum), 0 against p - 1, both 0"""
    h = (P - 1) // 2
    pairs = [(0, 0), (0, P - 1), (P - 1, 0), (1, 1), (P - 1, P - 1), (h, h), (h + 1, h + 1),
             (1, P - 1), (P - 1, 1), (h, h + 1), (h + 1, h), (2, P - 2),            # a + b = p
             (h, h - 1), (h - 1, h), (1, P - 3), (P - 3, 1),                        # p - 2: odd, below p
             (h - 1, h + 1), (4, P - 5), (2, P - 3), (P - 3, 2),                    # p - 1: even, below p
             (5, P - 4), (2, P - 1), (P - 1, 2), (h + 2, h),                        # p + 1: even as an integer, 1 mod p
             (3, P - 1), (P - 1, 3), (h + 2, h + 1), (h + 1, h + 2),                # p + 2: 2 mod p
             (P - 1, P - 2), (P - 2, P - 1), (P - 2, P - 2),                        # 2 p - 3, 2 p - 4: the largest sums
             (0, 1), (1, 0), (0, 2), (2, 0), (1, 2)]                                # small sums: 1, 2, 3 (no reduction)
    for k, v in enumerate(EDGE_LEAVES):                                             # each edge residue as an operand, one kind of partner each
        pairs.append([(v, v), (v, (P - v) % P), (v, (P - 1 - v) % P), (v, (P + 1 - v) % P)][k % 4])
    for k, v in enumerate(EDGE_LEAVES):                                             # ... and as the other operand
        pairs.append([((P - v) % P, v), ((P - 1 - v) % P, v), ((P + 1 - v) % P, v), (v, (P + 2 - v) % P)][(k + 1) % 4])
    assert all(0 <= a < P and 0 <= b < P for a, b in pairs)
    return pairs[:256]

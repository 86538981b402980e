"""Merkle trees whose hash is the Rescue-Prime sponge: commitments over the proof's own field, which a later proof can open inside
an AIR.

`RescueMerkle(rp, digest_len=1)` over a `RescuePrime` of rate >= 2; d = digest_len, 1 <= d <= rate.  A tree over the N rows (N a
power of two, N >= 1) of a matrix, leaves and nodes being digests of d field elements:

    leaf(row)         = rp.sponge(row, out_len=d)            for a row of w >= 1 elements
    node(left, right) = rp.sponge(left + right, out_len=d)   for two digests of d elements

The padding is `rp.pad`'s, always: a single 1, then zeros -- w // rate + 1 permutations per leaf, 2 d // rate + 1 per node.  At d = 1
a node is `rp.compress`, element for element.  There is NO domain separation between leaves and nodes, like the tutorial's
`Merkle`: a row of 2 d elements hashes like the node over its two halves, so a caller that needs leaves and nodes told apart fixes
the depth (as `verify` does through the path's length) or the row width.

Level j has N >> j nodes, node k of level j + 1 is node(level_j[2k], level_j[2k + 1]), and path[j] is the digest of node
(index >> j) ^ 1 of level j: the sibling leaf's digest first, the sibling of the root's child last -- the order of `Merkle.open`.
N = 1: the root is the leaf's digest and the path is empty.

`commit`, `open` and `verify` are the host model on plain integers (FieldElements or ints go in, digests are lists of d ints): the
specification.  The device methods run csrc/rescue_merkle.cuh through the sc_rescue_merkle_* entries: `build_device` over a
coalesced matrix in HBM (element j of row i at j * ld + i: the columns of a matrix of codewords are the rows of the tree, without a
transpose) returns a `RescueTree` with every level resident; `commit_device`, `commit_rows`, `open_rows`; `verify_batch` walks
many paths in one launch.
"""
import ctypes

INT32_MAX = (1 << 31) - 1


def _values(elements, p):
    return [int(getattr(v, "value", v)) % p for v in elements]


def set_split_max_nodes(value):
    """the tuning key "rescue_tree_split_max_nodes": a level (or a batch of paths) of at most `value` nodes runs one lane per state
    register, a wider one one lane per node; 0: never, anything from 2^31 - 1 on: always, -1: the library's default"""
    import starkcore as sc
    sc.set_tuning("rescue_tree_split_max_nodes", max(-1, min(int(value), INT32_MAX)))


class RescueTree:
    """Owner of an sc_rescue_tree_t: a tree in HBM, all levels kept"""

    def __init__(self, handle, digest_len, p):
        import starkcore as sc
        self._h, self.digest_len, self._p = handle, digest_len, p
        self.leaves = int(sc.lib().sc_rescue_merkle_leaves(handle))
        self.depth = self.leaves.bit_length() - 1

    def root(self):
        import starkcore as sc
        out = ctypes.create_string_buffer(16 * self.digest_len)
        sc._check(sc.lib().sc_rescue_merkle_root(self._h, out))
        return sc.unpack(out.raw, self.digest_len)

    def open_batch(self, indices):
        """the paths of `indices`: per index a list of `depth` digests"""
        import starkcore as sc
        indices = [int(i) for i in indices]
        for i in indices:
            assert(0 <= i and i < self.leaves), "cannot open invalid index"
        k, d = len(indices), self.digest_len
        if k == 0 or self.depth == 0:
            return [[] for _ in indices]
        idx = (ctypes.c_uint64 * k)(*indices)
        out = ctypes.create_string_buffer(16 * d * self.depth * k)
        sc._check(sc.lib().sc_rescue_merkle_open_batch(self._h, idx, k, out))
        words = sc.unpack(out.raw, d * self.depth * k)
        return [[words[(t * self.depth + j) * d:(t * self.depth + j + 1) * d] for j in range(self.depth)] for t in range(k)]

    def open(self, index):
        return self.open_batch([index])[0]

    def level_device(self, j, stream=None):
        """level j as a DeviceVector of d rows of leaves >> j elements (element e of node k at e * (leaves >> j) + k)"""
        import starkcore as sc
        assert(0 <= j and j <= self.depth), "level out of range"
        out = sc.DeviceVector(self.digest_len * (self.leaves >> j))
        sc._check(sc.lib().sc_rescue_merkle_level_copy_dev(self._h, j, out.ptr, stream))
        return out

    def level(self, j):
        """the digests of level j, node by node"""
        import starkcore as sc
        w, d = self.leaves >> j, self.digest_len
        words = sc.unpack(self.level_device(j).to_bytes(), d * w)
        return [[words[e * w + k] for e in range(d)] for k in range(w)]

    def free(self):
        import starkcore as sc
        if self._h is not None and sc._lib is not None:
            sc._lib.sc_rescue_merkle_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RescueMerkle:
    def __init__(self, rp, digest_len=1):
        assert rp.rate >= 2, "a tree needs a rate of at least 2"
        assert 1 <= digest_len <= rp.rate, "1 <= digest_len <= rate"
        self.rp, self.digest_len, self.p = rp, digest_len, rp.p

    # ---- the host model: the specification
    def leaf(self, row):
        row = list(row)
        assert len(row) >= 1, "a row of at least one element"
        return self.rp.sponge(row, out_len=self.digest_len)

    def node(self, left, right):
        assert len(left) == self.digest_len and len(right) == self.digest_len, "two digests of digest_len elements"
        return self.rp.sponge(list(left) + list(right), out_len=self.digest_len)

    def levels(self, rows):
        """every level of the tree over `rows`, the leaves' digests first, [root] last"""
        rows = list(rows)
        assert(len(rows) >= 1 and len(rows) & (len(rows) - 1) == 0), "length must be power of two"
        out = [[self.leaf(row) for row in rows]]
        while len(out[-1]) > 1:
            below = out[-1]
            out.append([self.node(below[i], below[i + 1]) for i in range(0, len(below), 2)])
        return out

    def commit(self, rows):
        return self.levels(rows)[-1][0]

    def open(self, index, rows):
        rows = list(rows)
        assert(len(rows) >= 1 and len(rows) & (len(rows) - 1) == 0), "length must be power of two"
        assert(0 <= index and index < len(rows)), "cannot open invalid index"
        return [level[(index >> j) ^ 1] for j, level in enumerate(self.levels(rows)[:-1])]

    def verify(self, root, index, path, row):
        assert(0 <= index and index < (1 << len(path))), "cannot verify invalid index"
        digest = self.leaf(row)
        for sibling in path:
            sibling = _values(sibling, self.p)
            digest = self.node(digest, sibling) if index % 2 == 0 else self.node(sibling, digest)
            index >>= 1
        return _values(root, self.p) == digest

    # ---- on the device
    def build_device(self, matrix, n, width, ld=None, stream=None):
        """the tree over the n rows of `width` elements of a DeviceVector (element j of row i at j * ld + i, ld = n by default);
        only enqueued -- on `stream` (a raw hipStream_t) or the library's"""
        import starkcore as sc
        ld = n if ld is None else ld
        assert(n >= 1 and n & (n - 1) == 0), "length must be power of two"
        assert width >= 1 and ld >= n and matrix.n >= (width - 1) * ld + n, "width rows of n elements at stride ld"
        h = ctypes.c_void_p()
        rp = self.rp
        sc._check(sc.lib().sc_rescue_merkle_build_dev(matrix.ptr, ld, width, n, self.digest_len, rp.m, rp.rate, rp._params, rp.N, ctypes.byref(h), stream))
        return RescueTree(h, self.digest_len, self.p)

    def commit_device(self, matrix, n, width, ld=None):
        return self.build_device(matrix, n, width, ld).root()

    def _rows_device(self, rows):
        import starkcore as sc
        rows = [_values(row, 1 << 128) for row in rows]
        assert(len(rows) >= 1 and len(rows) & (len(rows) - 1) == 0), "length must be power of two"
        width = len(rows[0])
        assert width >= 1 and all(len(row) == width for row in rows), "rows of one length, at least one element"
        return self.build_device(sc.DeviceVector.from_bytes(sc.pack([row[j] for j in range(width) for row in rows])), len(rows), width)

    def commit_rows(self, rows):
        """self.commit(rows), through the device"""
        return self._rows_device(rows).root()

    def open_rows(self, indices, rows):
        """[self.open(i, rows) for i in indices], through the device: one build, one gather"""
        rows = list(rows)
        for i in indices:
            assert(0 <= i and i < len(rows)), "cannot open invalid index"
        return self._rows_device(rows).open_batch(indices)

    def verify_batch(self, roots, indices, paths, rows):
        """[self.verify(root, index, path, row) for each item] in one launch; the paths share one length and the rows one width"""
        import starkcore as sc
        roots, paths, rows, indices = list(roots), list(paths), list(rows), [int(i) for i in indices]
        k, d = len(indices), self.digest_len
        assert len(roots) == k and len(paths) == k and len(rows) == k, "one root, path and row per index"
        if k == 0:
            return []
        depth, width = len(paths[0]), len(rows[0])
        assert all(len(p) == depth for p in paths) and width >= 1 and all(len(r) == width for r in rows), "paths of one length, rows of one width"
        assert depth <= 63, "a path of at most 63 entries"
        for i in indices:
            assert(0 <= i and i < (1 << depth)), "cannot verify invalid index"
        words = lambda digest: _values(digest, 1 << 128)
        assert all(len(r) == d for r in roots) and all(len(s) == d for p in paths for s in p), "digests of digest_len elements"
        roots_b = sc.pack([v for r in roots for v in words(r)])
        paths_b = sc.pack([v for p in paths for s in p for v in words(s)])
        rows_b = sc.pack([v for r in rows for v in words(r)])
        idx = (ctypes.c_uint64 * k)(*indices)
        out = ctypes.create_string_buffer(k)
        rp = self.rp
        sc._check(sc.lib().sc_rescue_merkle_verify_batch(roots_b, idx, paths_b if depth else None, rows_b, k, depth, width, d, rp.m, rp.rate,
                                                         rp._params, rp.N, out))
        return [b == 1 for b in out.raw[:k]]

"""BLAKE2b-512 Merkle commitments -- host shim (interface of reference code/merkle.py:3-43).

`commit` / `open` on field-element arrays run on the GPU (leaf = H(decimal ASCII of the residue),
node = H(left || right)); the tree stays resident in HBM, so an opening is a gather of log2 N digests
instead of the reference's full rebuild per call.  The raw-digest variants (`commit_`, `open_`,
`verify_`) and `verify` are tiny and stay on the host with hashlib.
"""
from hashlib import blake2b

from starkcore import CodewordMatrix, DeviceCodeword, MerkleForest, MerkleTree
import starkcore as _sc


class Merkle:
    H = blake2b

    def commit_(leafs):
        assert(len(leafs) & (len(leafs) - 1) == 0), "length must be power of two"
        level = list(leafs)
        while len(level) > 1:
            level = [Merkle.H(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
        return level[0]

    def _tree(data_array):
        if isinstance(data_array, DeviceCodeword):
            return data_array.tree()
        # leaves travel as 16-byte residues; a field wider than that has no device leaf format (and no CPU fallback)
        assert(len(data_array) == 0 or data_array[0].field.p <= (1 << 128)), "the MI355X Merkle kernels take residues below 2^128 only"
        return MerkleTree.from_bytes(b"".join(da.value.to_bytes(16, "little") for da in data_array))

    def commit(data_array):
        assert(len(data_array) & (len(data_array) - 1) == 0), "length must be power of two"
        return Merkle._tree(data_array).root

    def commit_batch(data_arrays):
        """[Merkle.commit(a) for a in data_arrays], the arrays of one length as ONE forest (csrc/merkle_forest.cuh: one set of launches
        and one wait for all their roots); a batch above the library's forest limit is split"""
        data_arrays = list(data_arrays)
        roots, by_length = [None] * len(data_arrays), {}
        for k, a in enumerate(data_arrays):
            assert(len(a) & (len(a) - 1) == 0), "length must be power of two"
            if len(a) < 2:
                roots[k] = Merkle.commit(a)
                continue
            assert(isinstance(a, DeviceCodeword) or a[0].field.p <= (1 << 128)), "the MI355X Merkle kernels take residues below 2^128 only"
            by_length.setdefault(len(a), []).append(k)
        for n, members in by_length.items():
            step = max(1, _sc.FOREST_MAX_LEAVES // n)
            for lo in range(0, len(members), step):
                part = members[lo:lo + step]
                forest = MerkleForest.build(CodewordMatrix.from_members([data_arrays[k] for k in part]))
                for k, root in zip(part, forest.roots):
                    roots[k] = root
        return roots

    def open_(index, leafs):
        assert(len(leafs) & (len(leafs) - 1) == 0), "length must be power of two"
        assert(0 <= index and index < len(leafs)), "cannot open invalid index"
        level, path = list(leafs), []
        while len(level) > 1:
            path.append(level[index ^ 1])
            level = [Merkle.H(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
            index >>= 1
        return path

    def open(index, data_array):
        assert(len(data_array) & (len(data_array) - 1) == 0), "length must be power of two"
        assert(0 <= index and index < len(data_array)), "cannot open invalid index"
        return Merkle._tree(data_array).open(index)

    def verify_(root, index, path, leaf):
        assert(0 <= index and index < (1 << len(path))), "cannot verify invalid index"
        node = leaf
        for sibling in path:
            node = Merkle.H(node + sibling).digest() if index % 2 == 0 else Merkle.H(sibling + node).digest()
            index >>= 1
        return root == node

    def verify(root, index, path, data_element):
        return Merkle.verify_(root, index, path, Merkle.H(bytes(data_element)).digest())

    # ---- row commitments (not in the reference): ONE tree over the rows of a matrix of codewords.  Leaf i is the
    # hash of every column's value at index i, personalised so that a leaf (a row of 8 values is 128 bytes) is never a node's hash;
    # nodes are H(left || right) as above.  `columns`: w >= 1 equal-length sequences, lists of FieldElements or DeviceCodewords.
    ROW_PERSON = b"sc-merkle-row"
    ROWS_DEVICE_MIN = 256            # rows from which commit_rows / open_rows build the tree on the GPU (csrc/merkle_rows.cuh)

    def row_leaf(row):
        return blake2b(b"".join(v.value.to_bytes(16, "little") for v in row), person=Merkle.ROW_PERSON).digest()

    def _rows(columns):
        columns = list(columns)
        assert(len(columns) >= 1), "a row tree needs at least one column"
        n = len(columns[0])
        assert(all(len(c) == n for c in columns)), "columns of one length"
        assert(n >= 1 and n & (n - 1) == 0), "length must be power of two"
        return columns, n

    def _on_device(columns, n):
        return any(isinstance(c, DeviceCodeword) for c in columns) or (n >= Merkle.ROWS_DEVICE_MIN and _sc.device_count() > 0)

    def _row_leafs(columns):
        return [Merkle.row_leaf(row) for row in zip(*columns)]

    def commit_rows(columns):
        columns, n = Merkle._rows(columns)
        if Merkle._on_device(columns, n):
            return _sc.RowTree.build(columns).root
        return Merkle.commit_(Merkle._row_leafs(columns))

    def commit_rows_batch(members):
        """[Merkle.commit_rows(columns) for columns in members] -- as ONE row forest (starkcore.RowForest: one set of launches and one
        wait for all the roots) when every member has the same number of columns and the same power-of-two length (at least two rows)
        and the whole batch has at least ROWS_DEVICE_MIN rows: the members' columns become the columns of one device matrix (columns
        that are not on the device are uploaded into it), tree t over columns t w ... t w + w - 1.  A batch above the library's forest
        limit is split; any other batch goes member by member."""
        members = [Merkle._rows(columns) for columns in members]
        if not members:
            return []
        w, n = len(members[0][0]), members[0][1]
        alike = all(len(columns) == w and length == n for columns, length in members)
        if not alike or n < 2 or w > _sc.ROWS_MAX_COLUMNS or len(members) * n < Merkle.ROWS_DEVICE_MIN or _sc.device_count() == 0:
            return [Merkle.commit_rows(columns) for columns, _ in members]
        roots, step = [], max(1, _sc.FOREST_MAX_LEAVES // n)
        for lo in range(0, len(members), step):
            part = members[lo:lo + step]
            matrix = CodewordMatrix.from_members([column for columns, _ in part for column in columns])
            roots += _sc.RowForest.build([(matrix, w)], n, len(part)).roots
        return roots

    def open_rows(index, columns):
        """(row, path): the columns' values at `index` and the authentication path of that row's leaf"""
        columns, n = Merkle._rows(columns)
        assert(0 <= index and index < n), "cannot open invalid index"
        if Merkle._on_device(columns, n):
            field = next(c.field for c in columns if isinstance(c, DeviceCodeword)) if any(isinstance(c, DeviceCodeword) for c in columns) else columns[0][0].field
            rows, paths = _sc.RowTree.build(columns).query([index])
            return [_sc._field_element()(v, field) for v in rows[0]], paths[0]
        return [c[index] for c in columns], Merkle.open_(index, Merkle._row_leafs(columns))

    def verify_rows(root, index, path, row):
        return Merkle.verify_(root, index, path, Merkle.row_leaf(row))

    # ---- pair leaves (not in the reference): a codeword of n >= 2 values under the row tree of its two halves -- n/2
    # leaves, leaf i = row_leaf((cw[i], cw[i + n/2])) -- so the two points of a colinearity test of FRI open with one path.  Thin
    # definitions over the row trees above; a DeviceCodeword is served without a copy (two pointers into the one vector).
    def _pair_columns(codeword):
        n = len(codeword)
        assert(n >= 2 and n & (n - 1) == 0), "length must be a power of two of at least 2"
        return [codeword[:n // 2], codeword[n // 2:]]

    def commit_pairs(codeword):
        if isinstance(codeword, DeviceCodeword):
            return codeword.pair_tree().root
        return Merkle.commit_rows(Merkle._pair_columns(codeword))

    def open_pair(index, codeword):
        """((y_a, y_b), path): the values at `index` and `index + n/2` and the authentication path of their leaf"""
        if isinstance(codeword, DeviceCodeword):
            assert(0 <= index and index < len(codeword) // 2), "cannot open invalid index"
            (pairs, paths), = _sc.query_pairs([codeword], [[index]])
            return pairs[0], paths[0]
        row, path = Merkle.open_rows(index, Merkle._pair_columns(codeword))
        return (row[0], row[1]), path

    def verify_pair(root, index, path, pair):
        return Merkle.verify_rows(root, index, path, list(pair))

"""Membership in a Rescue-Prime Merkle tree, proved with a STARK: "this leaf digest lies under this root", without the path.

`RescueMembership(tree, depth, expansion_factor=4, num_colinearity_checks=64, security_level=128)` over a `RescueMerkle` whose node is
ONE permutation -- 2 d < rate for d = tree.digest_len, so that the padded message left + right + [1] + zeros is one block (m = 4,
capacity 1, d = 1 is the smallest such tree; m = 3 never qualifies) -- and paths of `depth` entries, 1 <= depth <= 63.

    public   the root R and a leaf digest L (d elements each; L = tree.leaf(row)), and the depth
    secret   index < 2^depth and path (depth digests, in the order of RescueMerkle.open)
    relation the walk of RescueMerkle.verify, started from L, ends in R

L and R are PUBLIC.  The index and the path are hidden only as far as FastStark's randomizers hide a trace (the proof opens
randomized codewords, never a trace row); nothing else is claimed.  There is no domain separation between leaves and nodes, as in the
tree: the statement speaks of a digest `depth` levels below R, and what that digest is a digest OF is the caller's business.

The trace has W = m + d + 1 registers -- the state 0 .. m - 1, the sibling m .. m + d - 1, the direction bit m + d -- and
T = depth (N + 1) + 1 rows (C = N + 1 rows per level):

    row 0                L + [0] (m - d) | [0] d | 0                                            (all of it public)
    row 1 + j C          digest_j + path[j] + [1] + zeros when bit j of the index is 0, path[j] + digest_j + [1] + zeros when it is 1
    rows 1 + j C + i     that state after rounds 0 .. i - 1, i = 1 .. N
    all C rows of level j carry path[j] and the bit in the sibling and bit registers
    digest_0 = L, digest_(j+1) = registers 0 .. d - 1 of level j's last row; row T - 1 holds R there

Boundary conditions: every register at row 0, registers 0 .. d - 1 at row T - 1.  None pins a secret, which is why the junction between
two levels reads the sibling and the bit of the NEXT row.  The 2 m + 1 transition constraints have per-row public values -- a selector
J (1 where t mod C = 0) and the round constants A_i, B_i of round (t mod C) - 1 (0 where J = 1) -- as COLUMNS interpolated over
{omicron^t, t < T - 1} (multivariate.XColumnsConstraint), over [X, p_0 .. p_(W-1), n_0 .. n_(W-1)] with bit = n_(m+d):

    (1 - J) (sum_k MDS[i][k] p_k^3 + A_i - (sum_k MDSinv[i][k] (n_k - B_k))^3)                                      i < m
    J bit (bit - 1)
    J (n_e - p_e - bit (n_(m+e) - p_e)),   J (n_(d+e) - n_(m+e) - bit (p_e - n_(m+e)))                             e < d
    J (n_(2d) - 1),   J n_k for 2 d < k < m

`trace`, `boundary_constraints`, `x_columns` and `transition_constraints` are the host specification (Python integers; the last two
memoised per instance).  `trace_batch_device` / `trace_device` run csrc/rescue_merkle.cuh through sc_rescue_merkle_path_trace_dev: one
launch for all members, each register of each member one run that a DeviceTrace wraps without a copy.  `prove`, `verify`,
`prove_batch` (one trace launch, then FastStark.prove_batch: the proofs of sequential `prove` calls, byte for byte, under the same
os.urandom), `verify_batch` and `prove_rows` (leaves hashed, paths opened from a resident RescueTree, then proved).
"""
import ctypes

from algebra import Field, FieldElement
from univariate import Polynomial
from multivariate import MPolynomial, XColumns, XColumnsConstraint
from fast_stark import FastStark, DeviceTrace


def _values(elements, p):
    return [int(getattr(v, "value", v)) % p for v in elements]


class RescueMembership:
    def __init__(self, tree, depth, expansion_factor=4, num_colinearity_checks=64, security_level=128):
        rp = tree.rp
        assert 2 * tree.digest_len < rp.rate, "a membership proof needs a tree whose node is one permutation: 2 * digest_len < rate"
        assert 1 <= depth <= 63, "a depth of 1 .. 63"
        self.tree, self.rp, self.depth = tree, rp, depth
        self.m, self.d, self.N, self.p = rp.m, tree.digest_len, rp.N, rp.p
        self.W, self.C = self.m + self.d + 1, self.N + 1
        self.T = depth * self.C + 1
        self.field = Field.main()
        assert self.field.p == self.p, "the tree hashes in the main field"
        self.stark = FastStark(self.field, expansion_factor, num_colinearity_checks, security_level, self.W, self.T, transition_constraints_degree=4)
        self._preprocessed = self._columns = self._constraints = None

    def _preprocess(self):
        """(transition zerofier, its codeword, its root): made when the first proof is made or checked"""
        if self._preprocessed is None:
            self._preprocessed = self.stark.preprocess()
        return self._preprocessed

    # ---- the host specification ------------------------------------------------------------------------------------------------------
    def _checked(self, leaf_digest, index, path):
        d, p = self.d, self.p
        leaf_digest, path = _values(leaf_digest, p), [_values(s, p) for s in path]
        assert len(leaf_digest) == d and all(len(s) == d for s in path), "digests of digest_len elements"
        assert len(path) == self.depth, "a path of `depth` entries"
        assert(0 <= index and index < (1 << self.depth)), "cannot verify invalid index"
        return leaf_digest, path

    def _rows(self, leaf_digest, index, path):
        """the T rows as lists of residues"""
        m, d = self.m, self.d
        digest = list(leaf_digest)
        rows = [digest + [0] * (m - d) + [0] * d + [0]]
        for j, sibling in enumerate(path):
            bit = (index >> j) & 1
            state = (sibling + digest if bit else digest + sibling) + [1] + [0] * (m - 2 * d - 1)
            rows.append(state + sibling + [bit])
            for r in range(self.N):
                state = self.rp._round(state, r)
                rows.append(state + sibling + [bit])
            digest = state[:d]
        return rows

    def trace(self, leaf_digest, index, path):
        """the execution trace: T rows of W FieldElements"""
        leaf_digest, path = self._checked(leaf_digest, index, path)
        return [[FieldElement(v, self.field) for v in row] for row in self._rows(leaf_digest, index, path)]

    def boundary_constraints(self, root, leaf_digest):
        root, leaf_digest = _values(root, self.p), _values(leaf_digest, self.p)
        assert len(root) == self.d and len(leaf_digest) == self.d, "digests of digest_len elements"
        fe = lambda v: FieldElement(v, self.field)
        first = leaf_digest + [0] * (self.W - self.d)
        return [(0, s, fe(v)) for s, v in enumerate(first)] + [(self.T - 1, e, fe(v)) for e, v in enumerate(root)]

    def x_column_values(self):
        """the 1 + 2 m public columns as residues on the transitions t = 0 .. T - 2: J, A_0 .. A_(m-1), B_0 .. B_(m-1)"""
        m, C, rc = self.m, self.C, self.rp._constants
        selector = [int(t % C == 0) for t in range(self.T - 1)]
        constant = lambda t, at: 0 if t % C == 0 else rc[2 * (t % C - 1) * m + at]
        return [selector] + [[constant(t, at) for t in range(self.T - 1)] for at in range(2 * m)]

    def x_columns(self):
        """the public columns as polynomials in X through {omicron^t, t < T - 1} (an XColumns)"""
        if self._columns is None:
            domain, power = [], self.field.one()
            for _ in range(self.T - 1):
                domain.append(power)
                power = power * self.stark.omicron
            self._columns = XColumns([Polynomial.interpolate_domain(domain, [FieldElement(v, self.field) for v in values]) for values in self.x_column_values()])
        return self._columns

    def transition_constraints(self):
        if self._constraints is None:
            self._constraints = self._transition_constraints()
        return self._constraints

    def _transition_constraints(self):
        m, d, W, field, p = self.m, self.d, self.W, self.field, self.p
        columns = self.x_columns()
        variables = MPolynomial.variables(1 + 2 * W + 1 + 2 * m, field)
        prev, nxt = variables[1:1 + W], variables[1 + W:1 + 2 * W]
        J, A, B = variables[1 + 2 * W], variables[2 + 2 * W:2 + 2 * W + m], variables[2 + 2 * W + m:2 + 2 * W + 2 * m]
        one, bit = MPolynomial.constant(field.one()), nxt[m + d]
        mds, inv, alpha = self.rp._mds, self.rp._mds_inv, self.rp.alpha
        P0, N0, J0, A0, B0 = 1, 1 + W, 1 + 2 * W, 2 + 2 * W, 2 + 2 * W + m           # where the variables lie in a point of residues
        air = []

        def add(inner, structured):
            air.append(XColumnsConstraint(inner, columns, structured))
        for i in range(m):
            lhs = MPolynomial.constant(field.zero())
            for k in range(m):
                lhs = lhs + MPolynomial.constant(self.rp.MDS[i][k]) * (prev[k] ^ alpha)
            lhs = lhs + A[i]
            rhs = MPolynomial.constant(field.zero())
            for k in range(m):
                rhs = rhs + MPolynomial.constant(self.rp.MDSinv[i][k]) * (nxt[k] - B[k])
            rhs = rhs ^ alpha

            def round_constraint(v, p, i=i):
                lhs = v[A0 + i]
                for k in range(m):
                    lhs += mds[i][k] * pow(v[P0 + k], alpha, p)
                rhs = 0
                for k in range(m):
                    rhs += inv[i][k] * (v[N0 + k] - v[B0 + k])
                return (1 - v[J0]) * (lhs - pow(rhs % p, alpha, p))
            add((one - J) * (lhs - rhs), round_constraint)
        B1 = N0 + m + d
        add(J * bit * (bit - one), lambda v, p: v[J0] * v[B1] * (v[B1] - 1))
        for e in range(d):
            add(J * (nxt[e] - prev[e] - bit * (nxt[m + e] - prev[e])),
                lambda v, p, e=e: v[J0] * (v[N0 + e] - v[P0 + e] - v[B1] * (v[N0 + m + e] - v[P0 + e])))
            add(J * (nxt[d + e] - nxt[m + e] - bit * (prev[e] - nxt[m + e])),
                lambda v, p, e=e: v[J0] * (v[N0 + d + e] - v[N0 + m + e] - v[B1] * (v[P0 + e] - v[N0 + m + e])))
        add(J * (nxt[2 * d] - one), lambda v, p: v[J0] * (v[N0 + 2 * d] - 1))
        for k in range(2 * d + 1, m):
            add(J * nxt[k], lambda v, p, k=k: v[J0] * v[N0 + k])
        assert len(air) == 2 * m + 1
        return air

    # ---- device traces ---------------------------------------------------------------------------------------------------------------
    def trace_matrix_device(self, leaf_digests, indices, paths, stream=None):
        """the traces of k members as one DeviceVector of k W T elements, register s of member i's row t at (W i + s) T + t"""
        import starkcore as sc
        leaf_digests, paths, indices = list(leaf_digests), list(paths), [int(i) for i in indices]
        k, d = len(indices), self.d
        assert len(leaf_digests) == k and len(paths) == k, "one leaf digest and one path per index"
        words = lambda digest: _values(digest, 1 << 128)
        assert all(len(l) == d for l in leaf_digests) and all(len(s) == d for pth in paths for s in pth), "digests of digest_len elements"
        assert all(len(pth) == self.depth for pth in paths), "paths of `depth` entries"
        for i in indices:
            assert(0 <= i and i < (1 << self.depth)), "cannot verify invalid index"
        out = sc.DeviceVector(max(1, k * self.W * self.T))
        if k:
            leaves_b = sc.pack([v for l in leaf_digests for v in words(l)])
            paths_b = sc.pack([v for pth in paths for s in pth for v in words(s)])
            idx = (ctypes.c_uint64 * k)(*indices)
            rp = self.rp
            sc._check(sc.lib().sc_rescue_merkle_path_trace_dev(leaves_b, idx, paths_b, k, self.depth, d, rp.m, rp.rate, rp._params, rp.N, out.ptr, stream))
        return out

    def trace_batch_device(self, leaf_digests, indices, paths):
        """[DeviceTrace of self.trace(...) for each member]: one launch; the columns are views of one matrix, no copy"""
        import starkcore as sc
        indices = list(indices)
        whole = self.trace_matrix_device(leaf_digests, indices, paths)
        W, T = self.W, self.T
        return [DeviceTrace([sc.DeviceVector.wrap(whole.ptr + 16 * T * (W * i + s), T, whole) for s in range(W)], self.field)
                for i in range(len(indices))]

    def trace_device(self, leaf_digest, index, path):
        return self.trace_batch_device([leaf_digest], [index], [path])[0]

    # ---- proofs ------------------------------------------------------------------------------------------------------------------------
    def _device_flow(self):
        """does FastStark prove a trace of this length with its polynomials in HBM?  Shorter ones keep the reference's host lists"""
        return self.stark.randomized_trace_length >= FastStark.DEVICE_MIN

    def prove(self, root, leaf_digest, index, path, proof_stream=None):
        """a proof that `leaf_digest` lies `depth` levels under `root`; a false witness raises what FastStark.prove raises"""
        zerofier, codeword, _ = self._preprocess()
        trace = self.trace_device(leaf_digest, index, path) if self._device_flow() else self.trace(leaf_digest, index, path)
        return self.stark.prove(trace, self.transition_constraints(), self.boundary_constraints(root, leaf_digest), zerofier, codeword, proof_stream)

    def verify(self, root, leaf_digest, proof, proof_stream=None):
        _, _, zerofier_root = self._preprocess()
        return self.stark.verify(proof, self.transition_constraints(), self.boundary_constraints(root, leaf_digest), zerofier_root, proof_stream)

    def prove_batch(self, roots, leaf_digests, indices, paths, proof_streams=None):
        """[self.prove(root, leaf_digest, index, path, stream) for ...] -- the same bytes under the same os.urandom -- with one launch of
        the trace kernel for all members and one FastStark.prove_batch"""
        roots, leaf_digests, indices, paths = list(roots), list(leaf_digests), list(indices), list(paths)
        assert len(roots) == len(leaf_digests) == len(indices) == len(paths), "one root, leaf digest and path per index"
        proof_streams = [None] * len(roots) if proof_streams is None else list(proof_streams)
        if not roots:
            return []
        if not self._device_flow():
            return [self.prove(*member) for member in zip(roots, leaf_digests, indices, paths, proof_streams)]
        zerofier, codeword, _ = self._preprocess()
        traces = self.trace_batch_device(leaf_digests, indices, paths)
        boundaries = [self.boundary_constraints(root, leaf) for root, leaf in zip(roots, leaf_digests)]
        return self.stark.prove_batch(traces, self.transition_constraints(), boundaries, zerofier, codeword, proof_streams)

    def verify_batch(self, roots, leaf_digests, proofs, proof_streams=None):
        """[self.verify(root, leaf_digest, proof) ...] in one FastStark.verify_batch call; a malformed proof is reported False"""
        roots, leaf_digests, proofs = list(roots), list(leaf_digests), list(proofs)
        assert len(roots) == len(leaf_digests) == len(proofs), "one root and one leaf digest per proof"
        if not proofs:
            return []
        _, _, zerofier_root = self._preprocess()
        boundaries = [self.boundary_constraints(root, leaf) for root, leaf in zip(roots, leaf_digests)]
        return self.stark.verify_batch(proofs, self.transition_constraints(), boundaries, zerofier_root, proof_streams)

    def prove_rows(self, rescue_tree, indices, rows):
        """membership proofs for rows[i] at leaf indices[i] of a resident RescueTree (RescueMerkle.build_device): the leaves hashed in
        one launch, the paths opened in one, the proofs made by prove_batch -> (root, leaf digests, proofs)"""
        indices, rows = [int(i) for i in indices], [list(row) for row in rows]
        assert len(indices) == len(rows), "one row per index"
        assert rescue_tree.depth == self.depth and rescue_tree.digest_len == self.d, "a tree of this scheme's depth and digest length"
        root = rescue_tree.root()
        leaf_digests = self.rp.sponge_batch(rows, out_len=self.d)
        paths = rescue_tree.open_batch(indices)
        return root, leaf_digests, self.prove_batch([root] * len(indices), leaf_digests, indices, paths)

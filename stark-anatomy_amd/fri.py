"""FRI low-degree test -- host orchestration over device-resident codewords.

Interface of reference code/fri.py:11-231 (`Fri(offset, omega, initial_domain_length, expansion_factor,
num_colinearity_tests)` with num_rounds / sample_index / sample_indices / eval_domain / commit / query /
prove / verify).  What moved to the GPU: the split-and-fold of fri.py:85, the Merkle commitment of every
round (fri.py:71) and the authentication paths of the query phase (fri.py:108-111), served from trees
that stay in HBM.  The Fiat-Shamir transcript (ip.py) stays on the host and is byte-identical, so alphas
and query indices match the reference.
"""
import pickle as _pickle
from hashlib import blake2b

from algebra import *
from merkle import *
from ip import *
from ntt import *
from univariate import *
import starkcore as _sc
import proof_objects as _po
import grinding as _grinding
from starkcore import DeviceCodeword, DeviceVector, query_codewords


class AlsoOpen:
    """Openings a caller wants together with the query phase: `requests(top_level_indices)` -> (codewords, index lists); `answers`
    = [(packed residues, paths array)] per codeword once the query phase has fetched them, or None if it took another route.
    codewords / shift (optional): the same request as data -- device codewords of the domain's length, all opened at the sorted
    positions {i, i + shift, i + N/2, i + shift + N/2 (mod N)} over the top-level indices i (fast_stark.py:154-158) -- which lets
    the library derive the positions itself and serve Fri.prove in one call (sc_fri_prove_dev)"""

    def __init__(self, requests, codewords=None, shift=None):
        self.requests, self.answers = requests, None
        self.codewords, self.shift = codewords, shift
        self.position_arrays = None                        # per codeword: its opened positions as a uint64 array next to the answers


class AlsoOpenForests:
    """What AlsoOpen is to `prove`, for `prove_batch`: committed codewords that live in Merkle forests -- matrices of rows of the
    domain's length N -- opened per member at the sorted positions {i, i + shift, i + N/2, i + shift + N/2 (mod N)}, duplicates kept,
    over that member's top-level indices i (fast_stark.py:154-158).  forests: MerkleForests; owners[p][m]: the tree numbers of
    forests[p] that belong to member m of the batch -- m R ... m R + R - 1 for a forest of R boundary-quotient codewords per member,
    [m] for one codeword per member, [0] for every member of a forest over ONE codeword all members share (the transition
    zerofier's: its root is Merkle.commit's of that codeword).  After prove_batch: positions[m] = member m's positions, answers[m] =
    [(int residues, paths)] at them, one pair per (forest, tree) in the order of `owners`.  On the forest path the openings travel in
    the launch that fetches the members' FRI openings."""

    def __init__(self, forests, owners, shift):
        self.forests, self.owners, self.shift = list(forests), list(owners), shift
        self.answers, self.positions = None, None

    def _check(self, N, members):
        for forest in self.forests:
            assert(forest.n == N), "a forest opened with a FRI batch has rows of the domain's length"
        assert(len(self.owners) == len(self.forests)), "one list of owners per forest"
        for of_forest in self.owners:
            assert(isinstance(of_forest, (list, tuple)) and len(of_forest) == members and all(isinstance(trees, (list, tuple)) for trees in of_forest)), \
                "owners: per forest one list of tree numbers per member"

    def _positions(self, indices, N):
        duplicated = list(indices) + [(i + self.shift) % N for i in indices]
        return sorted(duplicated + [(i + N // 2) % N for i in duplicated])

    def _requests(self, members):
        """per forest, the (tree, position) pairs of the given members (numbers in the batch), whose positions are known"""
        return [[(tree, position) for m in members for tree in of_forest[m] for position in self.positions[m]] for of_forest in self.owners]

    def _take(self, members, fetched):
        """fetched: per forest (values, paths) in the order of _requests(members)"""
        at = [0] * len(self.forests)
        for m in members:
            self.answers[m] = []
            k = len(self.positions[m])
            for p, of_forest in enumerate(self.owners):
                values, paths = fetched[p]
                for _ in of_forest[m]:
                    self.answers[m].append((values[at[p]:at[p] + k], paths[at[p]:at[p] + k]))
                    at[p] += k


def library_transcript(proof_stream, rounds):
    """The byte strings in `proof_stream` if the library may run `rounds` rounds of the commit phase on it itself
    (sc_fri_commit_dev computes SHAKE-256(pickle(objects)) on its own), else None.  Only a plain ProofStream: a subclass may derive
    its challenges differently (the reference's SignatureProofStream prefixes the document).  Only distinct byte strings so far
    (roots): that list has a fixed pickle layout.  The size test counts what the C side counts (3 bytes of pickle opcodes per prior
    item, 67 per root of this commit); the library still answers "unsupported" for anything else it does not take, and then the
    caller's Python loop runs."""
    if type(proof_stream) is not ProofStream or _pickle.DEFAULT_PROTOCOL != 4:
        return None                                      # (csrc/transcript.h writes protocol 4, the default of CPython 3.8 - 3.13)
    prior = list(proof_stream.objects)
    if (len(prior) + rounds < 999 and all(type(o) is bytes and len(o) < 256 for o in prior) and len(set(map(id, prior))) == len(prior)
            and sum(len(o) + 3 for o in prior) + 67 * rounds < 60000):
        return prior
    return None


def _residue(element):
    """the canonical int of a FieldElement of the main field, None for anything else"""
    if type(element) is FieldElement and type(element.value) is int and 0 <= element.value < Field.P_MAIN and element.field.p == Field.P_MAIN:
        return element.value
    return None


class CombinationRows:
    """The opened points of the proofs that share one AIR on one FRI domain, as rows of sc_stark_combination_batch
    (csrc/combination.cuh): what all share, the members (one per proof: its weights and the coefficient lists of its boundary
    zerofiers and interpolants, equal lists stored once), and per opened point a row next to the host function that decides it
    when the device does not."""

    def __init__(self, registers, tables, generator, omega, domain_length, step, transition_shifts, boundary_shifts, min_rows=0, keep=None):
        self.registers, self.tables, self.min_rows, self.keep = registers, tables, min_rows, keep
        self.generator, self.omega, self.domain_length, self.step = generator, omega, domain_length, step
        self.transition_shifts, self.boundary_shifts = list(transition_shifts), list(boundary_shifts)
        self.weights, self.polys, self.pool, self.places, self.members = [], [], [], {}, 0
        self.rows, self.owners, self.hosts = [], [], []
        self.host_only = []                      # (owner, host function) of rows the format cannot hold

    def member(self, weights, zerofiers, interpolants):
        """a proof's tables -> its member number, None when a value is not a residue of the main field"""
        try:
            values = [_residue(w) for w in weights]
            lists = [[_residue(c) for c in polynomial.coefficients] for pair in zip(zerofiers, interpolants) for polynomial in pair]
        except Exception:
            return None
        if len(values) != 1 + 2 * len(self.transition_shifts) + 2 * self.registers or len(lists) != 2 * self.registers:
            return None
        if None in values or any(None in coefficients for coefficients in lists):
            return None
        self.weights.append(_sc.pack(values))
        for coefficients in lists:
            key = tuple(coefficients)
            place = self.places.get(key)
            if place is None:
                place = self.places[key] = sum(map(len, self.pool)) if coefficients else 0
                self.pool.append(coefficients)
            self.polys += [place, len(coefficients)]
        self.members += 1
        return self.members - 1

    def add(self, owner, member, index, claimed, randomizer, zerofier, current, following, host):
        """one opened point; host: () -> bool, the loop body of FastStark.verify the row stands for"""
        try:
            values = [_residue(v) for v in [claimed, randomizer, zerofier] + list(current) + list(following)]
            fits = member is not None and type(index) is int and 0 <= index < self.domain_length and None not in values and len(values) == 3 + 2 * self.registers
        except Exception:
            fits = False
        if not fits:
            self.host_only.append((owner, host))
            return
        self.rows.append(member.to_bytes(8, "little") + index.to_bytes(8, "little") + _sc.pack(values))
        self.owners.append(owner)
        self.hosts.append(host)

    def verdicts(self):
        """the device call: a uint8 array over the rows"""
        import numpy as np
        nterms, exps, coefs = self.tables
        shared = _sc.Combination(self.registers, nterms, exps, coefs, self.generator, self.omega, self.domain_length, self.step, self.transition_shifts,
                                 self.boundary_shifts, self.members, b"".join(self.weights), np.asarray(self.polys, dtype=np.uint64),
                                 _sc.pack([c for coefficients in self.pool for c in coefficients]))
        return _sc.combination_batch(shared, np.frombuffer(b"".join(self.rows), dtype=_sc.combination_row_dtype(self.registers)))


class BatchChecks:
    """The checks of a batch of proofs collected as rows (csrc/merkle_verify.cuh, csrc/combination.cuh) instead of evaluated one by
    one: every Merkle path, every colinearity test and every opened point of the combination of every proof, tagged with the proof it
    belongs to, then ONE device call per kind (`run`; the combination: one per AIR and domain).
    A row the device format cannot hold (a leaf that is not a residue below 2^128, a path that is not 64-byte digests, a root that is
    not a 64-byte string, a value that is not a residue of the main field) is decided here, by the host function it replaces."""

    def __init__(self, count):
        self.ok = [True] * count                 # host checks (and exceptions) per proof
        # Merkle rows as columns (starkcore.merkle_rows), the digests their paths index, the root table
        self.m_position, self.m_path, self.m_root, self.m_depth, self.m_kind, self.m_leaf, self.m_owner = [], [], [], [], [], [], []
        self.digests, self.n_digests = [], 0
        self.roots, self.root_index = [], {}
        # colinearity rows as columns (starkcore.colinearity_rows) and the round table, 48 bytes per entry
        self.c_a, self.c_b, self.c_round, self.c_y, self.c_owner, self.rounds = [], [], [], [], [], []
        self.col_points = []                     # per colinearity row: its points, for test_colinearity if the device leaves it undecided
        self.truncations = []                    # (values list, its length before round 0, round 0's colinearity references)
        self._refs = []                          # the current round's colinearity references: ("row", row index) or ("host", verdict)
        self.combinations = {}                   # key of an (AIR, domain) group -> its CombinationRows
        self.combination_device_rows = 0         # rows sent to sc_stark_combination_batch by `run`

    # Every check answers "go on" (True): a batch walk never stops at a failed check, the verdicts come from `run`.
    def reject(self, owner, *lines):
        """the walk gives up on proof `owner`; lines: what HostChecks.reject prints"""
        self.ok[owner] = False
        return False

    def root(self, root):
        """index of a 64-byte root in the root table, or None when the device cannot compare with it"""
        if type(root) is not bytes or len(root) != 64:
            return None
        index = self.root_index.get(root)
        if index is None:
            index = self.root_index[root] = len(self.roots)
            self.roots.append(root)
        return index

    def merkle(self, owner, root, index, path, data_element, leaf_digest=None):
        """Merkle.verify(root, index, path, data_element) as a row; leaf_digest (64 bytes, computed by the caller: a row commitment's
        leaf, Merkle.row_leaf) stands in for the element's hash: Merkle.verify_(root, index, path, leaf_digest)"""
        r = self.root(root)
        try:
            joined = b"".join(path)
            depth = len(path)
            device = (r is not None and type(index) is int and 0 <= index < (1 << depth) and depth <= 64 and len(joined) == 64 * depth
                      and (depth == 0 or max(map(len, path)) == 64))
        except Exception:
            device = False
        if device:
            if leaf_digest is not None:
                kind, leaf = _sc.LEAF_DIGEST, self.n_digests.to_bytes(16, "little")
                self.digests.append(leaf_digest)
                self.n_digests += 1
            elif type(data_element) is FieldElement and type(data_element.value) is int and 0 <= data_element.value < (1 << 128):
                kind, leaf = _sc.LEAF_RESIDUE, data_element.value.to_bytes(16, "little")
            else:
                try:
                    digest = Merkle.H(bytes(data_element)).digest()
                except Exception:
                    self.ok[owner] = False
                    return True
                kind, leaf = _sc.LEAF_DIGEST, self.n_digests.to_bytes(16, "little")
                self.digests.append(digest)
                self.n_digests += 1
            self.m_position.append(index)
            self.m_path.append(self.n_digests)
            self.m_root.append(r)
            self.m_depth.append(depth)
            self.m_kind.append(kind)
            self.m_leaf.append(leaf)
            self.m_owner.append(owner)
            self.digests.append(joined)
            self.n_digests += depth
            return True
        try:
            accepted = Merkle.verify(root, index, path, data_element) if leaf_digest is None else Merkle.verify_(root, index, path, leaf_digest)
        except Exception:
            accepted = False
        if not accepted:
            self.ok[owner] = False
        return True

    def round(self, offset, omega, alpha):
        """a round begins: its round-table entry (offset_r, omega_r, alpha_r); None when they are not residues of the main field"""
        self._refs = []
        if not all(type(e) is FieldElement and type(e.value) is int and 0 <= e.value < Field.P_MAIN and e.field.p == Field.P_MAIN
                   for e in (offset, omega, alpha)):
            return None
        self.rounds.append(offset.value.to_bytes(16, "little") + omega.value.to_bytes(16, "little") + alpha.value.to_bytes(16, "little"))
        return len(self.rounds) - 1

    def colinearity(self, owner, round_index, offset, omega, a, b, alpha, ya, yb, yc):
        """test_colinearity([(offset * omega^a, ya), (offset * omega^b, yb), (alpha, yc)]) as a row; where its verdict will be found is
        kept with the round's references, for `truncate`"""
        ys = (ya, yb, yc)
        if round_index is not None and all(type(y) is FieldElement and type(y.value) is int and 0 <= y.value < Field.P_MAIN
                                           and y.field.p == Field.P_MAIN for y in ys) and 0 <= a < (1 << 64) and 0 <= b < (1 << 64):
            self.c_a.append(a)
            self.c_b.append(b)
            self.c_round.append(round_index)
            self.c_y.append(ya.value.to_bytes(16, "little") + yb.value.to_bytes(16, "little") + yc.value.to_bytes(16, "little"))
            self.c_owner.append(owner)
            self.col_points.append((offset, omega, a, b, alpha, ya, yb, yc))
            self._refs.append(("row", len(self.c_a) - 1))
            return True
        try:
            accepted = test_colinearity([(offset * (omega ^ a), ya), (offset * (omega ^ b), yb), (alpha, yc)])
        except Exception:
            accepted = False
        if not accepted:
            self.ok[owner] = False
        self._refs.append(("host", accepted))
        return True

    def combination_group(self, key, make):
        """the CombinationRows of the (AIR, domain) group `key`, made by make() when the batch meets the group for the first time"""
        group = self.combinations.get(key)
        if group is None:
            group = self.combinations[key] = make()
        return group

    def combination(self, owner, group, member, index, claimed, randomizer, zerofier, current, following, host):
        """one opened point of proof `owner` -- the recomputed combination equals `claimed` (the loop body of FastStark.verify) -- as a
        row of `group`; a row the format cannot hold is decided by host() in `run`"""
        group.add(owner, member, index, claimed, randomizer, zerofier, current, following, host)

    def _run_combinations(self, ok):
        def on_host(owner, host):
            if ok[owner]:                        # (a proof that has failed already needs no further verdict)
                try:
                    accepted = host()
                except Exception:
                    accepted = False
                if not accepted:
                    ok[owner] = False
        for group in self.combinations.values():
            if not group:                        # (a group whose AIR the format does not hold: its proofs ran the host loop)
                continue
            for owner, host in group.host_only:
                on_host(owner, host)
            if not group.rows:
                continue
            if len(group.rows) < group.min_rows:
                for owner, host in zip(group.owners, group.hosts):
                    on_host(owner, host)
                continue
            verdicts = group.verdicts()
            self.combination_device_rows += len(group.rows)
            for t, verdict in enumerate(verdicts):
                if verdict == _sc.UNDECIDED:
                    on_host(group.owners[t], group.hosts[t])      # (the reference's own exception makes it False)
                elif verdict != 1:
                    ok[group.owners[t]] = False

    def run(self):
        """the device calls, then a proof's verdict: its host checks passed and every row of it passes"""
        import numpy as np
        ok = np.array(self.ok, dtype=bool)
        if self.m_position:
            rows = _sc.merkle_rows(self.m_position, self.m_path, self.m_root, self.m_depth, self.m_kind, b"".join(self.m_leaf))
            verdicts = _sc.merkle_verify_batch(rows, b"".join(self.digests), b"".join(self.roots))
            ok[np.asarray(self.m_owner, dtype=np.int64)[verdicts != 1]] = False
        col_verdicts = None
        if self.c_a:
            rows = _sc.colinearity_rows(self.c_a, self.c_b, self.c_round, b"".join(self.c_y))
            col_verdicts = _sc.colinearity_batch(rows, b"".join(self.rounds))
            for t in np.flatnonzero(col_verdicts == _sc.UNDECIDED):
                offset, omega, a, b, alpha, ya, yb, yc = self.col_points[t]
                try:
                    col_verdicts[t] = 1 if test_colinearity([(offset * (omega ^ int(a)), ya), (offset * (omega ^ int(b)), yb), (alpha, yc)]) else 0
                except Exception:
                    col_verdicts[t] = 0
            ok[np.asarray(self.c_owner, dtype=np.int64)[col_verdicts != 1]] = False
        self._run_combinations(ok)
        # Fri.verify appends round 0's pairs test by test and stops at the first failed colinearity test: the same prefix here
        for values, base, refs in self.truncations:
            for t, (where, what) in enumerate(refs):
                if not (col_verdicts[what] == 1 if where == "row" else what):
                    del values[base + 2 * (t + 1):]
                    break
        return [bool(v) for v in ok]

    def truncate(self, values, base):
        """round 0 (begun with `round`) appends its pairs to `values` from position `base` on: its tests' references, filled in place as
        `colinearity` records them (a walk that raises half-way leaves the tests recorded so far)"""
        self.truncations.append((values, base, self._refs))


class HostChecks:
    """BatchChecks' twin for one proof on the host: the same methods, every check decided at once by the function a row of BatchChecks
    stands for.  A check answers whether the walk goes on: False ends it there, before the next pull.  What raises inside a check
    propagates to the walk's caller."""

    def reject(self, owner, *lines):
        for line in lines:
            print(line)
        return False

    def merkle(self, owner, root, index, path, data_element, leaf_digest=None):
        return Merkle.verify(root, index, path, data_element) if leaf_digest is None else Merkle.verify_(root, index, path, leaf_digest)

    def round(self, offset, omega, alpha):
        return None

    def colinearity(self, owner, round_index, offset, omega, a, b, alpha, ya, yb, yc):
        return test_colinearity([(offset * (omega ^ a), ya), (offset * (omega ^ b), yb), (alpha, yc)])

    def truncate(self, values, base):
        pass

    def combination_group(self, key, make):
        return None                              # (no rows: the walk decides every opened point itself, in order, and stops at the first that fails)


class Fri:
    def __init__(self, offset, omega, initial_domain_length, expansion_factor, num_colinearity_tests, grinding_bits=0, pair_leaves=False):
        """grinding_bits (not in the reference; 0 = the reference's protocol, byte for byte): a proof of work of that many bits on
        the transcript between the last codeword and the query indices (grinding.py) -- the prover pushes the smallest accepted
        nonce, the verifier checks it, and the indices are sampled from the transcript with it
        pair_leaves (not in the reference; False = the reference's protocol, byte for byte): every round's codeword
        is committed under the tree of its pairs (Merkle.commit_pairs: leaf i holds cw[i] and cw[i + n/2]), so a colinearity test
        carries the pair (y_a, y_b) and ONE path; y_c is never opened -- the verifier reads it from the next round's pair or from the
        last codeword.  Same colinearity relation, same indices, same seeds."""
        self.offset, self.omega, self.field = offset, omega, omega.field
        self.domain_length = initial_domain_length
        self.expansion_factor, self.num_colinearity_tests = expansion_factor, num_colinearity_tests
        assert(type(grinding_bits) is int and 0 <= grinding_bits <= _grinding.MAX_BITS), "grinding_bits must be an integer of 0 .. %d" % _grinding.MAX_BITS
        self.grinding_bits = grinding_bits
        self.pair_leaves = bool(pair_leaves)
        assert(self.num_rounds() >= 1), "cannot do FRI with less than one round"

    def num_rounds(self):
        """commitments made by `commit`: the codeword is halved while it is longer than the expansion factor and than four times
        the number of colinearity tests (fri.py:22-28)"""
        rounds, length = 0, self.domain_length
        while length > self.expansion_factor and length > 4 * self.num_colinearity_tests:
            rounds, length = rounds + 1, length / 2
        return rounds

    def sample_index(byte_array, size):
        # fri.py:30-34 folds the bytes in with acc = (acc << 8) ^ b: the big-endian integer of the array
        # (only for byte strings: bytes(n) of an int n would be n zero bytes, where the reference's loop raises TypeError)
        if isinstance(byte_array, (bytes, bytearray, memoryview)):
            return int.from_bytes(byte_array, "big") % size
        acc = 0
        for b in byte_array:
            acc = (acc << 8) ^ int(b)
        return acc % size

    def sample_indices(self, seed, size, reduced_size, number):
        """`number` indices below `size`, pairwise distinct modulo `reduced_size` (they must not collide in the last codeword),
        drawn from blake2b(seed + counter zero bytes) for counter = 0, 1, ... (fri.py:36-51)"""
        assert(number <= reduced_size), f"cannot sample more indices than available in last codeword; requested: {number}, available: {reduced_size}"
        assert(number <= 2 * reduced_size), "not enough entropy in indices wrt last codeword"
        chosen, residues, counter = [], set(), 0
        while len(chosen) < number:
            # bytes(counter) is `counter` zero bytes (fri.py:44), not an encoding of the counter
            candidate = Fri.sample_index(blake2b(seed + bytes(counter)).digest(), size)
            counter += 1
            if candidate % reduced_size in residues:
                continue
            residues.add(candidate % reduced_size)
            chosen.append(candidate)
        return chosen

    def _round_positions(self, top_level_indices, r):
        """the `a` positions of round r's colinearity tests: the top-level indices reduced to half of codeword r's length (fri.py:126)"""
        half = self.domain_length >> (r + 1)
        return [index % half for index in top_level_indices]

    def eval_domain(self):
        # offset * omega^i, i < domain_length, by running product
        points, x = [], self.offset
        for _ in range(self.domain_length):
            points.append(x)
            x = x * self.omega
        return points

    def _check_omega_order(self, length):
        """fri.py:68 asserts omega_r^(N_r - 1) == omega_r^-1, i.e. omega_r^(N_r) == 1, in every round; omega_r = omega^(2^r) and
        N_r = N / 2^r, so every round's condition is omega^N == 1: checked once per (omega, length) -- a power and an inversion in
        Python integers are 0.1 ms, a twentieth of a 2^22 proof"""
        key = (self.omega.value, length)
        if getattr(self, "_order_checked", None) != key:
            assert(self.omega ^ (length - 1) == self.omega.inverse()), "error in commit: omega does not have the right order!"
            self._order_checked = key

    def _on_device(self, codeword):
        if isinstance(codeword, DeviceCodeword):
            return codeword
        return DeviceCodeword.from_list(codeword, self.field)

    def commit(self, codeword, proof_stream, round_index=0):
        """fri.py:66-94.  The chain root -> alpha -> fold -> next root is strictly serial.  When the proof stream holds nothing but
        digests so far (always the case for Fri.prove on its own and inside FastStark.prove) the whole round loop -- trees, the
        Fiat-Shamir step of ip.py:18-25, folds -- is ONE library call (sc_fri_commit_dev): nothing crosses the language boundary
        between a root arriving and the next launch.  Otherwise (_commit_rounds) a round's fold and tree are enqueued in one call
        and only the Fiat-Shamir step sits between a root arriving and the next launch."""
        codeword = self._on_device(codeword)
        rounds = self.num_rounds()
        self._check_omega_order(len(codeword))             # (before anything is enqueued)
        codewords = None
        if len(codeword) >= 2 and codeword._tree is None and library_transcript(proof_stream, rounds) is not None:
            codewords = self._commit_in_library(codeword, proof_stream, rounds)
        if codewords is None:
            codewords = self._commit_rounds(codeword, proof_stream, rounds)
        # the last codeword goes out in the clear, as a plain list (it is pickled into the transcript) -- described, not built,
        # when the stream can hold it that way (proof_objects: the transcript bytes are the same)
        lazy = _po.lazy_objects(proof_stream) if _po.eligible(codewords[-1]) else None
        if lazy is not None:
            lazy.add(_po.ElementList(codewords[-1], codewords[-1].vec.to_bytes()))
        else:
            proof_stream.push(codewords[-1].tolist())
        return codewords

    def _commit_in_library(self, codeword, proof_stream, rounds):
        import ctypes
        prior = proof_stream.objects
        k = len(prior)
        vecs = (ctypes.c_void_p * max(1, rounds - 1))()
        trees = (ctypes.c_void_p * rounds)()
        roots = ctypes.create_string_buffer(64 * rounds)
        alphas = (ctypes.c_uint64 * max(2, 2 * (rounds - 1)))()
        rc = _sc.lib().sc_fri_commit_dev(codeword.vec.ptr, len(codeword), _sc.fe_bytes(self.offset.value), _sc.fe_bytes(self.omega.value), rounds,
                                         b"".join(prior), (ctypes.c_uint32 * max(1, k))(*map(len, prior)), k, vecs, trees, roots, alphas, None)
        if rc == _sc.SC_ERR_UNSUPPORTED:
            return None                                  # a transcript shape the library does not write: the caller runs _commit_rounds
        _sc._check(rc)
        codewords, cur, raw = [], codeword, roots.raw
        for r in range(rounds):
            n = len(codeword) >> r
            if r > 0:
                cur = DeviceCodeword(DeviceVector.adopt(vecs[r - 1], n), self.field)
            root = raw[64 * r:64 * r + 64]
            cur._tree = _sc.MerkleTree(ctypes.c_void_p(trees[r]), root, n)
            proof_stream.push(root)
            codewords.append(cur)
        return codewords

    def _commit_rounds(self, codeword, proof_stream, rounds, pairs=False):
        """the same loop with the Fiat-Shamir step in Python (any proof stream): a round's fold and tree are ENQUEUED in one library
        call (sc_fri_fold_commit_dev; pairs: over pair trees, sc_fri_fold_pairs_commit_dev) and everything the host can do without
        the root (the next output vector) happens while the device hashes"""
        start_tree, tree, fold_commit = ("start_pair_tree", "pair_tree", "fold_pairs_commit") if pairs else ("start_tree", "tree", "fold_commit")
        omega, offset = self.omega, self.offset
        codewords = []
        getattr(codeword, start_tree)()
        for r in range(rounds):
            folded = DeviceVector(len(codeword) // 2) if r < rounds - 1 else None
            # Merkle root of this round's codeword (waits for the device); the tree stays in HBM for the query phase
            proof_stream.push(getattr(codeword, tree)().root)
            if r == rounds - 1:
                break
            alpha = self.field.sample(proof_stream.prover_fiat_shamir())
            codewords.append(codeword)
            codeword = getattr(codeword, fold_commit)(alpha, offset, omega, folded)
            omega, offset = omega ^ 2, offset ^ 2
        codewords.append(codeword)
        return codewords

    def query(self, current_codeword, next_codeword, c_indices, proof_stream):
        """one round of the query phase (fri.py:98-113): the s colinear triples (current[c], current[c + half], next[c]), then their
        authentication paths; returns the opened positions of the current codeword"""
        current, following = self._on_device(current_codeword), self._on_device(next_codeword)
        s, half = self.num_colinearity_tests, len(current) // 2
        lower = list(c_indices)
        upper = [c + half for c in lower]
        # one round trip per codeword: opened entries and their authentication paths together
        entries, paths = current.query(lower[:s] + upper[:s])
        next_entries, next_paths = following.query(lower[:s])
        for t in range(s):
            proof_stream.push((entries[t], entries[s + t], next_entries[t]))
        for t in range(s):
            for path in (paths[t], paths[s + t], next_paths[t]):
                proof_stream.push(path)
        return lower + upper

    def prove(self, codeword, proof_stream, also_open=None):
        """also_open (optional, an AlsoOpen): further device codewords to open at positions that depend on the sampled indices --
        FastStark's committed codewords (fast_stark.py:154-175) -- fetched in the SAME device round trip as the query phase"""
        assert(self.domain_length == len(codeword)), "initial codeword length does not match length of initial codeword"
        if self.pair_leaves:
            top_level_indices = self._prove_pairs_in_library(codeword, proof_stream, also_open) if Fri.PAIRS_IN_LIBRARY else None
            if top_level_indices is not None:
                return top_level_indices
            return self._prove_pairs(codeword, proof_stream, also_open)
        top_level_indices = self._prove_in_library(codeword, proof_stream, also_open)
        if top_level_indices is not None:
            return top_level_indices
        codewords = self.commit(codeword, proof_stream)
        self.grind(proof_stream)
        top_level_indices = self.sample_indices(proof_stream.prover_fiat_shamir(), len(codewords[0]) // 2, len(codewords[-1]), self.num_colinearity_tests)
        self._query_all(codewords, top_level_indices, proof_stream, also_open)
        return top_level_indices

    def grind(self, proof_stream):
        """the proof of work between the commit phase and the query indices: the smallest nonce accepted with the seed over the
        stream so far (searched on the GPU), pushed as a plain int; nothing at all at grinding_bits == 0"""
        if self.grinding_bits:
            nonce = _grinding.grind(proof_stream.prover_fiat_shamir(), self.grinding_bits)
            assert(nonce is not None), "no nonce is accepted"
            proof_stream.push(nonce)

    def _check_grinding(self, proof_stream):
        """the verifier's side: the seed over what it has read so far, then the nonce"""
        if not self.grinding_bits:
            return True
        seed = proof_stream.verifier_fiat_shamir()
        return _grinding.check(seed, proof_stream.pull(), self.grinding_bits)

    def _batchable(self, codewords):
        """what the forest path serves: the main field, at least two rounds (fri.py:122 reads codewords[1]), a power-of-two length,
        and members that are device codewords or sequences of residues below 2^128"""
        N, rounds, s = self.domain_length, self.num_rounds(), self.num_colinearity_tests
        if self.pair_leaves:                                     # (pair forests are not built: member by member through `prove`)
            return False
        if self.field.p != Field.P_MAIN or rounds < 2 or N < 2 or N & (N - 1) != 0 or s < 1 or s > (N >> (rounds - 1)):
            return False
        for cw in codewords:
            if isinstance(cw, DeviceCodeword):
                if cw.field.p != Field.P_MAIN:
                    return False
            elif not (type(cw[0]) is FieldElement and cw[0].field.p == Field.P_MAIN):       # (as Merkle._tree judges a list)
                return False
        return True

    def prove_batch(self, codewords, proof_streams, also_open=None):
        """[self.prove(codeword, stream) for ...] -- the same top-level indices, and after it every stream holds exactly what `prove`
        would have pushed (serialize() is byte-identical, member by member) -- with the members' work on the device done together:
        per round ONE Merkle forest over all members' codewords (csrc/merkle_forest.cuh; from the second round on its leaf stage
        computes every member's fold with that member's alpha) and ONE wait for all roots; then one kernel for every opening of
        every member.  The Fiat-Shamir step goes through each stream's own push / prover_fiat_shamir, so any ProofStream subclass
        and streams that already hold objects are served.  Shapes the forest path does not serve go member by member through `prove`.
        also_open (optional, an AlsoOpenForests): committed codewords in forests of their own, opened per member at the positions
        its sampled indices give -- in the launch that fetches a chunk's FRI openings; member by member, in one launch of their own.
        The streams hold what they hold without it."""
        codewords, proof_streams = list(codewords), list(proof_streams)
        assert(len(codewords) == len(proof_streams)), "prove_batch needs one proof stream per codeword"
        for codeword in codewords:
            assert(self.domain_length == len(codeword)), "initial codeword length does not match length of initial codeword"
        if also_open is not None:
            also_open._check(self.domain_length, len(codewords))  # (before any work)
            also_open.answers, also_open.positions = [None] * len(codewords), [None] * len(codewords)
        if not codewords:
            return []
        if not self._batchable(codewords):
            indices = [self.prove(codeword, stream) for codeword, stream in zip(codewords, proof_streams)]
            if also_open is not None:
                everyone = range(len(codewords))
                also_open.positions = [also_open._positions(top, self.domain_length) for top in indices]
                also_open._take(everyone, _sc.query_forests(also_open.forests, also_open._requests(everyone)))
            return indices
        self._check_omega_order(self.domain_length)              # (before anything is enqueued)
        step = max(1, _sc.FOREST_MAX_LEAVES // self.domain_length)
        indices = []
        for lo in range(0, len(codewords), step):
            indices += self._prove_forest(codewords[lo:lo + step], proof_streams[lo:lo + step], also_open, lo)
        return indices

    def _prove_forest(self, members, streams, also_open=None, member0=0):
        """members / streams: a chunk of the batch, whose member 0 is member `member0` of the batch (also_open counts in the batch)"""
        rounds, s, N, K = self.num_rounds(), self.num_colinearity_tests, self.domain_length, len(members)
        # commit phase (fri.py:66-94) for all members: forest r holds the members' r-th codewords
        forests = [_sc.MerkleForest.build(_sc.CodewordMatrix.from_members(members))]
        omega, offset = self.omega, self.offset
        for r in range(rounds):
            roots = forests[r].roots                             # one wait for K roots
            for stream, root in zip(streams, roots):
                stream.push(root)
            if r == rounds - 1:
                break
            alphas = [self.field.sample(stream.prover_fiat_shamir()).value for stream in streams]
            forests.append(_sc.MerkleForest.fold_build(forests[r].matrix, alphas, offset.value, omega.value))
            omega, offset = omega ^ 2, offset ^ 2
        # entries are created once per (member, codeword, index): the transcript is pickled by object identity (DeviceCodeword._entries)
        n_last = N >> (rounds - 1)
        last_raw = forests[-1].matrix.to_bytes()
        holders, top = [], []
        for m, (codeword, stream) in enumerate(zip(members, streams)):
            first = codeword if isinstance(codeword, DeviceCodeword) else DeviceCodeword(None, self.field, elements=list(codeword))
            middle = [DeviceCodeword(None, self.field) for _ in range(rounds - 2)]
            last = DeviceCodeword(None, self.field, elements=[FieldElement(v, self.field) for v in _sc.unpack(last_raw[16 * n_last * m:16 * n_last * (m + 1)], n_last)])
            holders.append([first] + middle + [last])
            stream.push(last._full)                              # the last codeword in the clear (fri.py:91)
        if self.grinding_bits:
            # the members' proofs of work in shared launches: every member's seed through its own stream, one search for all
            nonces = _grinding.grind_batch([stream.prover_fiat_shamir() for stream in streams], self.grinding_bits)
            assert(None not in nonces), "no nonce is accepted"
            for stream, nonce in zip(streams, nonces):
                stream.push(nonce)
        for stream in streams:
            top.append(self.sample_indices(stream.prover_fiat_shamir(), N // 2, n_last, s))
        # query phase (fri.py:124-128): codeword j opens its round's a and b positions and the c positions of the round before
        requests = [[] for _ in range(rounds)]
        for m in range(K):
            mine = [self._round_positions(top[m], j) for j in range(rounds - 1)]
            for j in range(rounds):
                request = []
                if j < rounds - 1:
                    request += mine[j] + [index + (N >> (j + 1)) for index in mine[j]]
                if j > 0:
                    request += mine[j - 1]
                requests[j] += [(m, index) for index in request]
        extra = []
        if also_open is not None:
            chunk = range(member0, member0 + K)
            for m in chunk:
                also_open.positions[m] = also_open._positions(top[m - member0], N)
            extra = also_open._requests(chunk)
        # ONE launch for every opening of every member, the further forests' included
        fetched = _sc.query_forests(forests + (also_open.forests if also_open is not None else []), requests + extra)
        if also_open is not None:
            also_open._take(chunk, fetched[rounds:])
        for m, stream in enumerate(streams):
            opened = []
            for j in range(rounds):
                values, paths = fetched[j]
                k = len(requests[j]) // K
                request = [index for _, index in requests[j][k * m:k * (m + 1)]]
                opened.append((holders[m][j]._entries(request, values[k * m:k * (m + 1)]), paths[k * m:k * (m + 1)]))
            for i in range(rounds - 1):
                entries, paths = opened[i]
                next_entries, next_paths = opened[i + 1]
                c_at = 2 * s if i + 2 < rounds else 0
                for triple in zip(entries[:s], entries[s:2 * s], next_entries[c_at:c_at + s]):
                    stream.push(triple)
                for trio in zip(paths[:s], paths[s:2 * s], next_paths[c_at:c_at + s]):
                    for path in trio:
                        stream.push(path)
        return top

    def _library_route(self, codeword, proof_stream, also_open, pairs=False):
        """What the two one-call routes (_prove_in_library, _prove_pairs_in_library) share before the call: None when the stream or
        the codewords are not of the kind the library serves -- the caller's phases then run one by one, with the same bytes -- else
        (prior, extra, extra_trees, roots, last_raw, top, quad): the stream's byte strings so far, also_open's codewords and their
        trees, and the buffers the call fills (the roots, the last codeword's residues, the top-level and the quadrupled indices)."""
        import ctypes
        rounds, s = self.num_rounds(), self.num_colinearity_tests
        N = self.domain_length
        if not (isinstance(codeword, DeviceCodeword) and _po.eligible(codeword) and codeword._tree is None and N >= 2 and N & (N - 1) == 0):
            return None
        if rounds < 2:                  # (fri.py:122 reads codewords[1]: the reference itself has no proof with fewer than two codewords)
            return None
        if pairs and (N >> (rounds - 1)) < 2:                    # (a pair tree needs a last codeword of two elements)
            return None
        if self.field.p != Field.P_MAIN or s > (N >> (rounds - 1)) or s < 1 or library_transcript(proof_stream, rounds) is None:
            return None
        extra = []
        if also_open is not None:
            extra = also_open.codewords
            if extra is None or also_open.shift is None or not all(isinstance(cw, DeviceCodeword) and _po.eligible(cw) and len(cw) == N for cw in extra):
                return None
        if rounds + len(extra) > 32:
            return None
        self._check_omega_order(N)
        return (list(proof_stream.objects), extra, [cw.tree() for cw in extra], ctypes.create_string_buffer(64 * rounds),
                ctypes.create_string_buffer(16 * (N >> (rounds - 1))), (ctypes.c_uint64 * s)(), (ctypes.c_uint64 * (4 * s))())

    def _library_arguments(self, codeword, also_open, route, answers):
        """the arguments the two calls share (include/starkcore.h).  No handle of the commit phase comes back (vecs_out = trees_out =
        NULL): nothing reads the folded codewords or their trees once the openings are on the host, and the library hands their
        memory back before it returns"""
        import ctypes
        prior, extra, extra_trees, roots, last_raw, top, quad = route
        k, ne = len(prior), len(extra)
        return (codeword.vec.ptr, self.domain_length, _sc.fe_bytes(self.offset.value), _sc.fe_bytes(self.omega.value), self.num_rounds(),
                self.num_colinearity_tests, b"".join(prior), (ctypes.c_uint32 * max(1, k))(*map(len, prior)), k,
                ne, (ctypes.c_void_p * max(1, ne))(*[t._h for t in extra_trees]),
                (ctypes.c_void_p * max(1, ne))(*[cw.vec.ptr for cw in extra]), int(also_open.shift) if ne else 0,
                None, None, roots, None, last_raw, top, quad, answers.ptr, answers.nbytes, None)

    def _push_library_commit(self, proof_stream, codeword, field, roots, last_raw, nonce):
        """What comes back from either call, pushed as the reference pushes the commit phase (fri.py:71, :91): the roots, the last
        codeword in the clear (described: proof_objects.ElementList), and the nonce the library found and hashed into the seed of
        the indices.  field: the field object of the folded codewords' entries (a proof is pickled by identity).  Returns the entry
        holders per codeword and the stream's described objects, for the query phase's description."""
        raw = roots.raw
        rounds = len(raw) // 64
        for r in range(rounds):
            proof_stream.push(raw[64 * r:64 * r + 64])
        holders = [_po.entries_of(codeword)] + [_po.DetachedEntries(field) for _ in range(rounds - 1)]
        lazy = _po.lazy_objects(proof_stream)
        lazy.add(_po.ElementList(holders[-1], last_raw.raw))
        if self.grinding_bits:
            lazy.append(int(nonce.value))
        return holders, lazy

    def _take_library_openings(self, also_open, count, data, values_at, paths_at, where):
        """also_open's answers as views of the pinned buffer `data`: per codeword 4 s residues from byte values_at on, 4 s paths of
        log2 N digests from byte paths_at on, and the positions as the library wrote them (`where`)"""
        c, stride = 4 * self.num_colinearity_tests, 64 * (self.domain_length.bit_length() - 1)
        also_open.answers = [(data[values_at + 16 * c * e:values_at + 16 * c * (e + 1)],
                              data[paths_at + c * stride * e:paths_at + c * stride * (e + 1)].reshape(c, stride)) for e in range(count)]
        also_open.position_arrays = [where[c * e:c * (e + 1)] for e in range(count)]

    def _prove_in_library(self, codeword, proof_stream, also_open):
        """fri.py:115-130 as ONE library call (sc_fri_prove_dev): commit phase, the challenge over the transcript with the last
        codeword, the sampled indices, and one kernel that writes every opening of the proof into pinned host memory.  What comes
        back is pushed as the reference pushes it -- roots, the last codeword, per round s triples and 3 s paths -- in described
        form (proof_objects); None when the stream or the codewords are not of the kind the library serves (_library_route)."""
        import ctypes
        import numpy as np
        route = self._library_route(codeword, proof_stream, also_open)
        if route is None:
            return None
        rounds, s, N = self.num_rounds(), self.num_colinearity_tests, self.domain_length
        _, extra, _, roots, last_raw, top, _ = route
        ne = len(extra)
        # openings per pair (see include/starkcore.h): codeword j: the 2 s of its own round (j < rounds - 1) -- the c positions of the round
        # before are among them -- and the last codeword the s of the round before
        counts = [2 * s if j + 1 < rounds else (s if j > 0 else 0) for j in range(rounds)] + [4 * s] * ne
        depths = [(N >> j).bit_length() - 1 for j in range(rounds)] + [N.bit_length() - 1] * ne
        total = sum(counts)
        el_bytes = (16 * total + 255) & ~255
        path_bytes = sum(64 * c * d for c, d in zip(counts, depths))
        # Lifetime: `answers` is pinned host memory from the library's pool; the segments added to the stream below (and
        # also_open.answers) are VIEWS of it, so it stays page-locked for as long as the stream's described objects live and goes
        # back to the pool when the stream is dropped after serialize().  A caller that keeps streams calls
        # proof_stream.objects.detach() (proof_objects.LazyProofObjects.detach) to hold plain objects instead.
        answers = _sc.HostBuffer(el_bytes + path_bytes + 8 * total)
        nonce = ctypes.c_uint64(0)
        arguments = self._library_arguments(codeword, also_open, route, answers)
        if self.grinding_bits:                                   # the same call with the proof of work between the last codeword and the indices
            rc = _sc.lib().sc_fri_prove_grind_dev(*arguments, self.grinding_bits, ctypes.byref(nonce))
        else:
            rc = _sc.lib().sc_fri_prove_dev(*arguments)
        if rc == _sc.SC_ERR_UNSUPPORTED:
            return None
        _sc._check(rc)
        holders, lazy = self._push_library_commit(proof_stream, codeword, self.field, roots, last_raw, nonce)
        # the query phase's objects (fri.py:104-113): described by the answers as they lie in the pinned buffer
        data = answers.array
        own = sum(counts[:rounds])                               # openings of the commit phase's codewords; the caller's come behind them
        own_paths = sum(64 * c * d for c, d in zip(counts[:rounds], depths[:rounds]))
        where = data[el_bytes + path_bytes:el_bytes + path_bytes + 8 * total].view(np.uint64)
        lazy.add(_po.FriQueryPhase(holders, s, counts[:rounds], depths[:rounds], data[:16 * own], data[el_bytes:el_bytes + own_paths], where[:own]))
        if also_open is not None:
            self._take_library_openings(also_open, ne, data, 16 * own, el_bytes + own_paths, where[own:])
        return list(top)

    def _query_all(self, codewords, top_level_indices, proof_stream, also_open=None):
        """The query phase of fri.py:124-128 with ONE device round trip for all rounds: everything a codeword has to open
        (its a/b entries for its own round, the c entries of the previous round) is fetched together, then pushed in the
        reference's order (per round: s triples, then 3*s paths as a, b, c)."""
        s = self.num_colinearity_tests
        rounds = len(codewords) - 1
        halves = [len(cw) // 2 for cw in codewords]           # (len() of a device codeword is a call into the binding: once each)
        per_round = [self._round_positions(top_level_indices, i) for i in range(rounds)]
        requests = []
        for j in range(len(codewords)):
            request = []
            if j < rounds:
                half = halves[j]
                request += per_round[j][:s] + [index + half for index in per_round[j][:s]]
            if j > 0:
                request += per_round[j - 1][:s]
            requests.append(request)
        lazy = _po.lazy_objects(proof_stream) if all(_po.eligible(cw) for cw in codewords) else None
        if lazy is not None:
            # the device's answers go into the stream as they are: residues and paths stay packed, the transcript is pickled from
            # their description (proof_objects.FriRound); the reference's objects exist only if somebody reads them
            more_codewords, more_requests = also_open.requests(top_level_indices) if also_open is not None else ([], [])
            fetched = _sc.query_codewords_raw(list(codewords) + list(more_codewords), requests + list(more_requests))
            if also_open is not None:
                also_open.answers = fetched[len(codewords):]
            for i in range(rounds):
                values, paths = fetched[i]
                next_values, next_paths = fetched[i + 1]
                c_at = 2 * s if i + 1 < rounds else 0
                a = per_round[i][:s]
                half = halves[i]
                lazy.add(_po.FriRound(codewords[i], codewords[i + 1], a, [index + half for index in a], a,
                                      values[:16 * s], values[16 * s:32 * s], next_values[16 * c_at:16 * (c_at + s)],
                                      paths[:s], paths[s:2 * s], next_paths[c_at:c_at + s]))
            return
        if all(isinstance(cw, DeviceCodeword) for cw in codewords):
            fetched = query_codewords(codewords, requests)          # every round's openings in one device round trip
        else:
            fetched = [cw.query(request) for cw, request in zip(codewords, requests)]
        # pushes in the reference's order (fri.py:104-113 per round: s triples, then per test the paths of a, b, c); a ProofStream's
        # `push` is `objects.append`, so a whole round goes in with two list extensions instead of 4 s method calls
        objects = proof_stream.objects if type(proof_stream) is ProofStream else None
        for i in range(rounds):
            entries, paths = fetched[i]
            next_entries, next_paths = fetched[i + 1]
            c_at = 2 * s if i + 1 < rounds else 0
            triples = list(zip(entries[:s], entries[s:2 * s], next_entries[c_at:c_at + s]))
            openings = [p for trio in zip(paths[:s], paths[s:2 * s], next_paths[c_at:c_at + s]) for p in trio]
            if objects is not None:
                objects.extend(triples)
                objects.extend(openings)
            else:
                for obj in triples + openings:
                    proof_stream.push(obj)

    # -- pair leaves --------------------------------------------------------------------
    PAIRS_IN_LIBRARY = True          # False: `prove` with pair_leaves always takes the round-by-round route (_prove_pairs); tests and tools compare the two

    def _prove_pairs_in_library(self, codeword, proof_stream, also_open):
        """`prove` with pair_leaves as ONE library call (sc_fri_prove_pairs_dev): commit phase over pair trees (the persistent tail
        kernel's pair form from 2^16 elements down), last codeword, proof of work, indices, and one kernel that writes every pair,
        every path and also_open's openings into pinned host memory.  What comes back is pushed as _prove_pairs pushes it -- roots,
        the last codeword, the nonce, per round s pairs and s paths -- in described form (proof_objects.FriPairsQueryPhase).  Served
        under the conditions of _prove_in_library (_library_route); None otherwise, and _prove_pairs then runs with the same bytes."""
        import ctypes
        import numpy as np
        route = self._library_route(codeword, proof_stream, also_open, pairs=True)
        if route is None:
            return None
        rounds, s, N = self.num_rounds(), self.num_colinearity_tests, self.domain_length
        _, extra, _, roots, last_raw, top, _ = route
        ne = len(extra)
        # the four sections of `answers` (include/starkcore.h): pairs, also_open's elements, paths, positions
        opened = rounds - 1
        depths = [(N >> (j + 1)).bit_length() - 1 for j in range(opened)]                  # log2 of codeword j's n_j / 2 pair leaves
        pair_bytes = (32 * s * opened + 255) & ~255
        element_bytes = (16 * 4 * s * ne + 255) & ~255
        own_paths = 64 * s * sum(depths)
        path_bytes = (own_paths + 64 * 4 * s * (N.bit_length() - 1) * ne + 255) & ~255
        total = s * opened + 4 * s * ne
        # (lifetime of the pinned buffer: see _prove_in_library -- the segments and also_open.answers are views of it)
        answers = _sc.HostBuffer(pair_bytes + element_bytes + path_bytes + 8 * total)
        nonce = ctypes.c_uint64(0)
        rc = _sc.lib().sc_fri_prove_pairs_dev(*self._library_arguments(codeword, also_open, route, answers), self.grinding_bits, ctypes.byref(nonce))
        if rc == _sc.SC_ERR_UNSUPPORTED:
            return None
        _sc._check(rc)
        # (the folded codewords' entries carry the FIELD OBJECT of the codeword they were folded from, as DeviceCodeword.fold_pairs_commit's do)
        holders, lazy = self._push_library_commit(proof_stream, codeword, codeword.field, roots, last_raw, nonce)
        data = answers.array
        paths_at, where_at = pair_bytes + element_bytes, pair_bytes + element_bytes + path_bytes
        where = data[where_at:where_at + 8 * total].view(np.uint64)
        lazy.add(_po.FriPairsQueryPhase(holders[:opened], s, depths, data[:32 * s * opened], data[paths_at:paths_at + own_paths], where[:s * opened]))
        if also_open is not None:
            self._take_library_openings(also_open, ne, data, pair_bytes, paths_at + own_paths, where[s * opened:])
        return list(top)

    def _prove_pairs(self, codeword, proof_stream, also_open=None):
        """`prove` with pair_leaves: the round-by-round route of _commit_rounds over pair trees (round 0's tree is started first, then
        per round one sc_fri_fold_pairs_commit_dev with the Fiat-Shamir step in Python, so any ProofStream subclass is served), the
        last codeword in the clear, the proof of work, and a query phase of ONE device round trip (sc_fri_pairs_query_dev): per round
        r < rounds - 1 the s pairs (cw_r[a], cw_r[a + half]), then the s paths of leaf a in cw_r's pair tree.  Nothing of cw_{r+1} is
        pushed for round r.  also_open's openings travel in a call of their own."""
        codeword = self._on_device(codeword)
        rounds, s = self.num_rounds(), self.num_colinearity_tests
        N = len(codeword)
        assert(N & (N - 1) == 0 and (N >> (rounds - 1)) >= 2), "pair leaves need power-of-two codewords of at least two elements in every round"
        self._check_omega_order(N)                             # (before anything is enqueued)
        codewords = self._commit_rounds(codeword, proof_stream, rounds, pairs=True)
        proof_stream.push(codewords[-1].tolist())              # the last codeword in the clear
        self.grind(proof_stream)
        top_level_indices = self.sample_indices(proof_stream.prover_fiat_shamir(), N // 2, len(codewords[-1]), s)
        requests = [self._round_positions(top_level_indices, r) for r in range(rounds - 1)]
        for pairs, paths in _sc.query_pairs(codewords[:-1], requests):
            for pair in pairs:
                proof_stream.push(pair)
            for path in paths:
                proof_stream.push(path)
        if also_open is not None:
            more_codewords, more_requests = also_open.requests(top_level_indices)
            also_open.answers = _sc.query_codewords_raw(list(more_codewords), list(more_requests))
        return top_level_indices

    def _pair_shape(self, pair):
        """a pulled pair as two elements of the field below p, else None"""
        if type(pair) not in (tuple, list) or len(pair) != 2:
            return None
        p = self.field.p
        for y in pair:
            if not (type(y) is FieldElement and type(y.value) is int and 0 <= y.value < p and getattr(y.field, "p", None) == p):
                return None
        return (pair[0], pair[1])

    @staticmethod
    def _path_shape(path, depth):
        return type(path) in (list, tuple) and len(path) == depth and all(type(d) is bytes and len(d) == 64 for d in path)

    def _last_codeword_degree(self, last_codeword, last_omega, last_offset):
        """Degree of the interpolant of the last codeword on its coset: intt + unscale (the route the
        reference's fri.py:165-166 / docs describe) -- same unique polynomial as Lagrange at fri.py:164."""
        coefficients = intt(last_omega, last_codeword)
        poly = Polynomial(coefficients).scale(last_offset.inverse())
        assert(fast_coset_evaluate(poly, last_offset, last_omega, len(last_codeword)) == last_codeword), "re-evaluated codeword does not match original!"
        return poly.degree()

    def verify(self, proof_stream, polynomial_values):
        return self._walk(proof_stream, polynomial_values, HostChecks(), None)

    def verify_batch(self, proof_streams, polynomial_values_lists):
        """[self.verify(stream, values) for ...] with every Merkle path and colinearity test of the batch checked in one device call
        per kind (csrc/merkle_verify.cuh); a proof on which `verify` raises is reported False, and never affects the others"""
        checks = BatchChecks(len(proof_streams))
        for owner, (proof_stream, polynomial_values) in enumerate(zip(proof_streams, polynomial_values_lists)):
            try:
                if not self._walk(proof_stream, polynomial_values, checks, owner):
                    checks.reject(owner)
            except Exception:
                checks.reject(owner)
        return checks.run()

    def _walk(self, proof_stream, polynomial_values, checks, owner):
        """THE verifier (fri.py:132-231): one walk over a proof, pull by pull, whose checks go to `checks` -- a HostChecks decides each
        at once and ends the walk at the first that fails (`verify`); a BatchChecks records it as a row for proof `owner` and always
        goes on (`verify_batch`, FastStark.verify_batch).  False: rejected on the way; True: nothing failed so far."""
        rounds, s = self.num_rounds(), self.num_colinearity_tests
        # the commit phase replayed: per round a root and the challenge it determines, then the last codeword in the clear
        roots, alphas = [], []
        for _ in range(rounds):
            roots.append(proof_stream.pull())
            alphas.append(self.field.sample(proof_stream.verifier_fiat_shamir()))
        last_codeword = proof_stream.pull()
        if self.pair_leaves:                                     # (a last codeword no pair tree can be built over is rejected ...
            try:
                well_formed = Merkle.commit_pairs(last_codeword) == roots[-1]
            except Exception:
                well_formed = False
        else:                                                    # ... one no decimal tree can be built over raises, as in the reference)
            well_formed = Merkle.commit(last_codeword) == roots[-1]
        if not well_formed:
            return checks.reject(owner, "last codeword is not well formed")
        # the last codeword lives on the coset after rounds - 1 squarings; it must be of low degree there
        squarings = 1 << (rounds - 1)
        last_omega, last_offset = self.omega ^ squarings, self.offset ^ squarings
        assert(last_omega.inverse() == last_omega ^ (len(last_codeword) - 1)), "omega does not have right order"
        allowed = len(last_codeword) // self.expansion_factor - 1
        observed = self._last_codeword_degree(last_codeword, last_omega, last_offset)
        if observed > allowed:
            return checks.reject(owner, "last codeword does not correspond to polynomial of low enough degree", "observed degree: %s" % observed,
                                 "but should be: %s" % allowed)
        if not self._check_grinding(proof_stream):
            return checks.reject(owner, "proof of work fails")
        # the query phase: consistency of consecutive codewords at the sampled positions
        top_level_indices = self.sample_indices(proof_stream.verifier_fiat_shamir(), self.domain_length >> 1, self.domain_length >> (rounds - 1), s)
        query_phase = self._walk_pairs if self.pair_leaves else self._walk_triples
        return query_phase(proof_stream, polynomial_values, checks, owner, roots, alphas, last_codeword, top_level_indices)

    def _walk_triples(self, proof_stream, polynomial_values, checks, owner, roots, alphas, last_codeword, top_level_indices):
        """decimal leaves: per round the s triples (y_a, y_b, y_c), their tests, then 3 s paths, each pulled right before its check"""
        omega, offset = self.omega, self.offset
        for r in range(len(roots) - 1):
            half = self.domain_length >> (r + 1)
            lower = self._round_positions(top_level_indices, r)
            triples = [proof_stream.pull() for _ in lower]
            round_index = checks.round(offset, omega, alphas[r])
            if r == 0:        # registered before the tests: a later triple that raises must not keep pairs `verify` would not have appended
                checks.truncate(polynomial_values, len(polynomial_values))
            for a, (ya, yb, yc) in zip(lower, triples):
                if r == 0:
                    polynomial_values += [(a, ya), (a + half, yb)]
                # (x_a, y_a), (x_b, y_b) and (alpha, y_c) lie on one line: that is the fold of fri.py:85 read backwards
                if not checks.colinearity(owner, round_index, offset, omega, a, a + half, alphas[r], ya, yb, yc):
                    return checks.reject(owner, "colinearity check failure")
            for a, (ya, yb, yc) in zip(lower, triples):
                for root, position, leaf, label in ((roots[r], a, ya, "aa"), (roots[r], a + half, yb, "bb"), (roots[r + 1], a, yc, "cc")):
                    if not checks.merkle(owner, root, position, proof_stream.pull(), leaf):
                        return checks.reject(owner, "merkle authentication path verification fails for " + label)
            omega, offset = omega ^ 2, offset ^ 2
        return True

    def _walk_pairs(self, proof_stream, polynomial_values, checks, owner, roots, alphas, last_codeword, top_level_indices):
        """pair leaves: per round s pairs (y_a, y_b) and s paths, one per pair (a row whose leaf digest, Merkle.row_leaf, is computed
        here).  y_c of round r is never in the proof: it is the member of the next round's pair at a % (half / 2) that lies at
        position a, or last_codeword[a] in the last queried round -- so every round's pairs and paths are pulled before the first test.
        A pair that is not two field elements below p, or a path that is not log2(half) digests of 64 bytes, rejects before anything is
        appended to polynomial_values."""
        rounds, s = len(roots), self.num_colinearity_tests
        pairs, paths = [], []
        for r in range(rounds - 1):
            depth = (self.domain_length >> (r + 1)).bit_length() - 1
            pairs.append([self._pair_shape(proof_stream.pull()) for _ in range(s)])
            paths.append([proof_stream.pull() for _ in range(s)])
            if None in pairs[r]:
                return checks.reject(owner, "a pair is not two field elements")
            if not all(Fri._path_shape(path, depth) for path in paths[r]):
                return checks.reject(owner, "an authentication path has the wrong shape")
        omega, offset = self.omega, self.offset
        for r in range(rounds - 1):
            half = self.domain_length >> (r + 1)
            lower = self._round_positions(top_level_indices, r)
            if r + 2 < rounds:
                y_c = [pairs[r + 1][t][0 if a < half // 2 else 1] for t, a in enumerate(lower)]
            else:
                y_c = [last_codeword[a] for a in lower]
            round_index = checks.round(offset, omega, alphas[r])
            if r == 0:
                checks.truncate(polynomial_values, len(polynomial_values))
            for a, (ya, yb), yc in zip(lower, pairs[r], y_c):
                if r == 0:
                    polynomial_values += [(a, ya), (a + half, yb)]
                if not checks.colinearity(owner, round_index, offset, omega, a, a + half, alphas[r], ya, yb, yc):
                    return checks.reject(owner, "colinearity check failure")
            for a, pair, path in zip(lower, pairs[r], paths[r]):
                if not checks.merkle(owner, roots[r], a, path, None, leaf_digest=Merkle.row_leaf(pair)):
                    return checks.reject(owner, "merkle authentication path verification fails for a pair")
            omega, offset = omega ^ 2, offset ^ 2
        return True

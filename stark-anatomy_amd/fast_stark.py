"""NTT-based STARK prover / verifier -- the main CALLER of the GPU hot path.

Host mirror of the interface of reference code/fast_stark.py:8-286:
`FastStark(field, expansion_factor, num_colinearity_checks, security_level, num_registers, num_cycles,
transition_constraints_degree=2)` with `preprocess / prove / verify` and the degree-bound helpers.  Every
`fast_zerofier`, `fast_interpolate`, `fast_coset_evaluate`, `fast_coset_divide`, `Merkle.commit/open` and
`Fri.prove` inside goes through ntt.py / merkle.py / fri.py to the MI355X.  The order of `os.urandom` draws and of
`proof_stream.push` calls is the reference's, so with a patched `fast_stark.os.urandom` the proof bytes are identical.
"""
from functools import reduce
import ctypes
import os

from fri import *
from univariate import *
from multivariate import *
from ntt import *
from ntt import _View, _shrink_order
import starkcore as _sc
import proof_objects as _po
from grinding import MAX_BITS as MAX_GRINDING_BITS


def draw_random_bytes(count, width=17):
    """`count` draws of os.urandom(width) as one byte string, in draw order.  Long runs are drawn in blocks: os.urandom(n) is
    the next n bytes of the stream, so the bytes and their order are those of the individual draws."""
    block = 4096
    return b"".join(os.urandom(width * min(block, count - i)) for i in range(0, count, block))


class DeviceTrace:
    """The execution trace as device-resident COLUMNS: one DeviceVector of `rows` field elements per register -- what the
    `trace` argument of FastStark.prove (a list of rows of FieldElements, fast_stark.py:76) is to a caller whose trace never
    was a Python list.  A 2^20-row trace of two registers is two million Python objects and seconds of marshalling as lists
    (SURVEY.md App. C); as columns it is 32 MiB in HBM."""

    def __init__(self, columns, field):
        assert len(columns) >= 1 and all(c.n == columns[0].n for c in columns), "columns of one length, one per register"
        self.columns, self.field = list(columns), field

    @classmethod
    def from_rows(cls, rows, field):
        """rows: the reference's list of rows (lists of FieldElement or ints)"""
        width = len(rows[0])
        cols = [DeviceVector.from_bytes(b"".join(int(getattr(row[s], "value", row[s])).to_bytes(16, "little") for row in rows)) for s in range(width)]
        return cls(cols, field)

    @classmethod
    def from_packed(cls, packed_columns, field):
        """packed_columns: per register, the column as packed bytes (16 little-endian bytes per element)"""
        return cls([DeviceVector.from_bytes(c) for c in packed_columns], field)

    def __len__(self):
        return self.columns[0].n

    def entry(self, cycle, register):
        """one cell as a FieldElement (boundary conditions are read from the trace: 16 bytes from HBM)"""
        return FieldElement(int.from_bytes(self.columns[register].to_bytes(cycle, 1), "little"), self.field)


def sampled_polynomial(raw, field, width=17):
    """Polynomial([field.sample(raw[17 i : 17 i + 17]) ...]) as a DevicePolynomial: Field.sample on the device (sc_sample_bytes_dev)"""
    count = len(raw) // width
    vec = DeviceVector(max(count, 1))
    _sc._check(_sc.lib().sc_sample_bytes_dev(raw, count, width, vec.ptr, None))
    return DevicePolynomial(vec, field, count)


def os_urandom_is_genuine():
    """is os.urandom the interpreter's own (the operating system's generator), not a seeded stand-in a test has put in its place?
    Only then may the draws be made anywhere but through os.urandom itself, in any order."""
    return type(os.urandom).__name__ == "builtin_function_or_method"


def random_polynomial(count, field, width=17):
    """Polynomial([field.sample(os.urandom(17)) for i in range(count)]) (fast_stark.py:116-117) as a DevicePolynomial.  With the
    operating system's os.urandom the library makes the draws itself -- getrandom(2), several host threads, straight into a
    pinned buffer (sc_sample_urandom_dev); a patched os.urandom is called draw by draw in the reference's order."""
    if not os_urandom_is_genuine():
        return sampled_polynomial(draw_random_bytes(count, width), field, width)
    vec = DeviceVector(max(count, 1))
    _sc._check(_sc.lib().sc_sample_urandom_dev(count, width, vec.ptr, None))
    return DevicePolynomial(vec, field, count)


def prefetch_random_polynomial(count, width=17):
    """start the draws of a later random_polynomial(count, ...) on the library's host threads and return (a no-op under a patched
    os.urandom, whose draws must be made one by one in the reference's order)"""
    if count > 0 and os_urandom_is_genuine():
        _sc._check(_sc.lib().sc_urandom_prefetch(count, width))


def _collect_verdicts(pending):
    """run every collected check, then raise what the first failing one raised: a check left unread would keep its pinned slot
    (shared with the asynchronous Merkle roots) for as long as the exception's traceback lives"""
    checks = iter(pending)
    try:
        for verdict in checks:
            verdict()
    finally:
        for verdict in checks:                 # only after a failure: the rest are still waited for, their own verdicts dropped
            try:
                verdict()
            except Exception:                  # noqa: BLE001
                pass


def _drop_verdicts(pending):
    """wait for collected checks nobody will read any more (something else has failed), their verdicts dropped"""
    for verdict in pending:
        try:
            verdict()
        except Exception:                      # noqa: BLE001
            pass


def device_powers(base, count):
    """base^i, i < count, as a DeviceVector (Polynomial.scale of the all-ones vector: no host loop)"""
    ones = DeviceVector.from_bytes((1).to_bytes(16, "little") * count)
    out = DeviceVector(count)
    _sc._check(_sc.lib().sc_scale_dev(ones.ptr, out.ptr, count, _sc.fe_bytes(base.value), None))
    _sc.synchronize()
    return out


class FastStark:
    def __init__(self, field, expansion_factor, num_colinearity_checks, security_level, num_registers, num_cycles, transition_constraints_degree=2, grinding_bits=0,
                 row_commitments=False, pair_leaves=False):
        """grinding_bits (not in the reference; 0 = the reference's protocol): bits of proof of work on the transcript before FRI's
        query indices (grinding.py, Fri(grinding_bits)); each bit stands in for half a colinearity check in the security level.
        row_commitments (not in the reference; False = the reference's protocol, byte for byte): the boundary-quotient codewords and the
        randomizer codeword are committed in ONE Merkle tree over their rows (Merkle.commit_rows) -- one root in front of
        FRI's objects, and per opened position one row of num_registers + 1 values and ONE authentication path -- instead of a tree, a
        root and a path each.  No challenge lies between those commitments, so nothing else of the protocol moves.  prove_batch serves
        the option too: the members' row trees are one row forest (starkcore.RowForest, _rows_batch_served).
        pair_leaves (not in the reference; False = the reference's protocol, byte for byte): Fri's option of the same name (DESIGN.md
        3.4e), passed through -- FRI's query phase carries one pair and one path per colinearity test.  It combines freely with the two
        above and does not enter the security-level test; prove_batch then goes member by member (Fri._batchable)."""
        assert(field.p.bit_length() >= security_level), "p must have at least as many bits as security level"
        assert(expansion_factor & (expansion_factor - 1) == 0), "expansion factor must be a power of 2"
        assert(expansion_factor >= 4), "expansion factor must be 4 or greater"
        assert(type(grinding_bits) is int and 0 <= grinding_bits <= MAX_GRINDING_BITS), "grinding_bits must be an integer of 0 .. %d" % MAX_GRINDING_BITS
        assert(num_colinearity_checks * 2 + grinding_bits >= security_level), "number of colinearity checks must be at least half of security level" + (" less the grinding bits" if grinding_bits else "")

        # parameters (names are the reference's, fast_stark.py:14-35: callers read them)
        self.field, self.security_level = field, security_level
        self.expansion_factor, self.num_colinearity_checks = expansion_factor, num_colinearity_checks
        self.grinding_bits = grinding_bits
        self.row_commitments = bool(row_commitments)
        self.pair_leaves = bool(pair_leaves)
        self.num_registers, self.original_trace_length = num_registers, num_cycles
        self.num_randomizers = 4 * num_colinearity_checks
        self.randomized_trace_length = num_cycles + self.num_randomizers

        # domains: the trace lives on <omicron>, the smallest power-of-two subgroup strictly larger than the degree of the AIR
        # substituted into the trace polynomials; FRI runs on the coset generator * <omega>, expansion_factor times larger
        self.omicron_domain_length = 1 << max(1, (self.randomized_trace_length * transition_constraints_degree).bit_length())
        self.fri_domain_length = self.omicron_domain_length * expansion_factor
        self.generator = field.generator()
        self.omega = field.primitive_nth_root(self.fri_domain_length)
        self.omicron = field.primitive_nth_root(self.omicron_domain_length)
        self._omicron_domain = None
        self._trace_domains = {}          # rows -> DeviceDomain of {omicron^i, i < rows} (progression tables, built once)
        self._lifted = {}                 # id(host Polynomial) -> (the Polynomial, its DevicePolynomial): lifted once, not per proof
        self._zerofier_values = {}        # transform order -> (the transition zerofier, its values on that order's coset)

        self.fri = Fri(self.generator, self.omega, self.fri_domain_length, expansion_factor, num_colinearity_checks, grinding_bits, pair_leaves=self.pair_leaves)

    @property
    def omicron_domain(self):
        """omicron^i for i < omicron_domain_length (fast_stark.py:33), by running product instead of one exponentiation per
        entry; built when first read (a 2^22-entry list of objects is seconds of host time the device-resident prover never needs)"""
        if self._omicron_domain is None:
            domain, power = [], self.field.one()
            for _ in range(self.omicron_domain_length):
                domain.append(power)
                power = power * self.omicron
            self._omicron_domain = domain
        return self._omicron_domain

    def _trace_domain(self, rows):
        """{omicron^i, i < rows} as a DeviceDomain: a geometric progression, so interpolation through it is a handful of
        convolutions (csrc/geoseq.cuh) instead of a subproduct tree"""
        domain = self._trace_domains.get(rows)
        if domain is None:
            if len(self._trace_domains) >= 4:
                self._trace_domains.clear()
            domain = self._trace_domains[rows] = DeviceDomain.geometric(self.field.one(), self.omicron, rows)
        return domain

    def _lift(self, polynomial):
        """a host Polynomial (or an already device-resident one) as a DevicePolynomial; the same object is lifted once"""
        if isinstance(polynomial, DevicePolynomial):
            return polynomial
        hit = self._lifted.get(id(polynomial))
        if hit is not None and hit[0] is polynomial:
            return hit[1]
        if len(self._lifted) >= 16:
            self._lifted.clear()
        dev = DevicePolynomial.from_polynomial(polynomial, self.field)
        self._lifted[id(polynomial)] = (polynomial, dev)
        return dev

    # -- preprocessing (fast_stark.py:36-40) ------------------------------------------------------
    def preprocess(self, device_resident=False):
        """device_resident=True: the transition zerofier comes back as a DevicePolynomial (prove() takes either form) and no
        host list of the omicron domain is ever built -- the zerofier of {omicron^i, i < T - 1} has a closed form on the device"""
        if device_resident:
            assert(self.field.p == Field.P_MAIN), "the device-resident prover works in the main field"
            count = self.original_trace_length - 1
            if count >= 2:
                zerofier_domain = DeviceDomain.geometric(self.field.one(), self.omicron, count)
                transition_zerofier = DevicePolynomial.from_codeword(fast_zerofier_device(zerofier_domain))
            else:
                transition_zerofier = DevicePolynomial.from_polynomial(fast_zerofier(self.omicron_domain[:count], self.omicron, self.omicron_domain_length), self.field)
            transition_zerofier_codeword = transition_zerofier.coset_evaluate(self.generator, self.omega, self.fri_domain_length)
            return transition_zerofier, transition_zerofier_codeword, Merkle.commit(transition_zerofier_codeword)
        transition_zerofier = fast_zerofier(self.omicron_domain[:(self.original_trace_length - 1)], self.omicron, len(self.omicron_domain))
        if self.randomized_trace_length >= FastStark.DEVICE_MIN and self.field.p == Field.P_MAIN:
            # long traces: the codeword is committed here and opened in prove() where it lies, in HBM (a DeviceCodeword is list-like)
            transition_zerofier_codeword = fast_coset_evaluate_device(transition_zerofier, self.generator, self.omega, self.fri_domain_length)
        else:
            transition_zerofier_codeword = self._lde(transition_zerofier)
        transition_zerofier_root = Merkle.commit(transition_zerofier_codeword)
        return transition_zerofier, transition_zerofier_codeword, transition_zerofier_root

    # Traces of at least this many rows (randomizers included) are proved with every polynomial resident in HBM (see prove());
    # shorter ones follow the reference's host-list data flow with the GPU behind each fast_* call.  Same polynomials, same
    # objects pushed in the same order -- the proofs are byte-identical either way (tests/test_gpu_stark.py runs both settings
    # against the reference's golden proofs).
    DEVICE_MIN = 32
    # True: every commitment waits for its root before the prover goes on (the reference's order of events; A/B of proof_objects.RootLater)
    EAGER_COMMITS = False
    # Traces of at least this many registers are proved in COLUMN BATCHES on the device data flow: the registers are the rows of one
    # matrix, and trace interpolation, the trace polynomials' degrees, the boundary-quotient LDEs and the trace's values on the
    # transition quotients' coset are one library call each for all registers instead of one per register.  Same polynomials, same
    # codewords, same pushes and draws in the same order: the proofs are byte-identical (tests/test_gpu_wide_stark.py).  Narrower
    # traces run the per-register code.  (Measured: tools/wide_trace_timing.py, profiles/column_batches/.)
    COLUMN_BATCH_MIN = 4
    # Two further steps of the column-batched path, each with its per-register form kept for comparison (tools/wide_trace_timing.py).
    # COLUMN_DIVIDE: the boundary quotients of all registers are one combination (trace_s - interpolant_s for every s) and one
    # columns-form coset division with ONE pending verdict, instead of a dozen launches and a pinned slot per register.
    # COLUMN_COMBINE: the nonlinear combination is one pass (sc_combine_columns_dev) instead of one axpy launch per term.
    # Same polynomials, same pushes and draws, same assertion messages: the proofs are byte-identical (tests/test_gpu_wide_stark_columns.py).
    # Both are on: with both, the 16-register proof's median is below the median with neither at FRI 2^16 and 2^20 (DESIGN.md 3.8b,
    # profiles/column_batches/).  False is the code as it was before them.
    COLUMN_DIVIDE = True
    COLUMN_COMBINE = True

    def _lde(self, polynomial):
        """Low-degree extension onto the FRI coset  generator * omega^i  (the LDE kernel)."""
        return fast_coset_evaluate(polynomial, self.generator, self.omega, self.fri_domain_length)

    # -- degree bookkeeping (fast_stark.py:42-56) ---------------------------------------------------
    def transition_degree_bounds(self, transition_constraints):
        """degree bound of every AIR polynomial once X (degree 1) and the 2 * num_registers trace polynomials (current and next
        row, degree randomized_trace_length - 1 each) are substituted for its variables: the worst monomial decides"""
        trace_degree = self.randomized_trace_length - 1
        variables = 1 + 2 * self.num_registers
        bounds = []
        for constraint in transition_constraints:
            offered = getattr(constraint, "degree_bound", None)
            if offered is not None:
                # a constraint with public columns (multivariate.XColumnsConstraint) has no dictionary to read: it knows its bound
                bounds.append(offered(trace_degree, self.num_registers))
                continue
            monomial_degrees = [sum(exponents[:1]) + trace_degree * sum(exponents[1:variables]) for exponents in constraint.dictionary]
            bounds.append(max(monomial_degrees))
        return bounds

    def transition_quotient_degree_bounds(self, transition_constraints):
        # the transition zerofier vanishes on the first original_trace_length - 1 points of <omicron>
        zerofier_degree = self.original_trace_length - 1
        return [bound - zerofier_degree for bound in self.transition_degree_bounds(transition_constraints)]

    def max_degree(self, transition_constraints):
        # one less than the next power of two above the largest quotient bound (fast_stark.py:50-52)
        largest = max(self.transition_quotient_degree_bounds(transition_constraints))
        return (1 << max(1, largest.bit_length())) - 1

    def _boundary_points(self, boundary, register):
        """(domain points, values) of the boundary conditions (cycle, register, value) that concern `register`"""
        mine = [(cycle, value) for cycle, reg, value in boundary if reg == register]
        return [self.omicron ^ cycle for cycle, _ in mine], [value for _, value in mine]

    def boundary_zerofiers(self, boundary):
        return [Polynomial.zerofier_domain(self._boundary_points(boundary, s)[0]) for s in range(self.num_registers)]

    def boundary_interpolants(self, boundary):
        return [Polynomial.interpolate_domain(*self._boundary_points(boundary, s)) for s in range(self.num_registers)]

    def boundary_quotient_degree_bounds(self, randomized_trace_length, boundary):
        return [(randomized_trace_length - 1) - zerofier.degree() for zerofier in self.boundary_zerofiers(boundary)]

    def sample_weights(self, number, randomness):
        # bytes(i) is i zero bytes (fast_stark.py:74)
        return [self.field.sample(blake2b(randomness + bytes(i)).digest()) for i in range(0, number)]

    # a list here turns on the per-phase breakdown: after each phase of prove() the device is waited for and (phase, seconds since
    # the previous mark) is appended -- measurement only (tools/stark_phase_compare.py); the phases are sharded_stark's
    phase_log = None

    def _mark(self, phase):
        if self.phase_log is None:
            return
        import time
        _sc.synchronize()
        now = time.perf_counter()
        if phase is not None:
            self.phase_log.append((phase, now - self._phase_t0))
        self._phase_t0 = now

    # -- prover (fast_stark.py:76-178) -------------------------------------------------------------
    def prove(self, trace, transition_constraints, boundary, transition_zerofier, transition_zerofier_codeword, proof_stream=None):
        if proof_stream == None:
            proof_stream = ProofStream()
        field, registers = self.field, range(self.num_registers)
        self._mark(None)

        # randomizer rows appended to the trace (draw order: row by row, register by register); one concatenation instead of one
        # per row -- the caller's list is not touched either way
        if isinstance(trace, DeviceTrace):
            assert(field.p == Field.P_MAIN), "a device-resident trace lives in the main field"
            # the randomizer polynomial's draws (fast_stark.py:116-117: one os.urandom(17) per coefficient, 36 MB at a 2^24 FRI
            # domain) start now and pass while the GPU works on the trace
            prefetch_random_polynomial(self.max_degree(transition_constraints) + 1)
            batched = self.num_registers >= FastStark.COLUMN_BATCH_MIN
            columns = self._randomized_columns(trace, draw_random_bytes(self.num_randomizers * self.num_registers), batched)
            trace_rows, on_device = len(trace) + self.num_randomizers, True
        else:
            trace = trace + [[field.sample(os.urandom(17)) for s in registers] for _ in range(self.num_randomizers)]
            trace_rows = len(trace)
            on_device = trace_rows >= FastStark.DEVICE_MIN and field.p == Field.P_MAIN
            batched = on_device and self.num_registers >= FastStark.COLUMN_BATCH_MIN
            if batched:
                # one upload: the registers are the rows of one matrix, each column a view of its row
                lists = [[row[s] for row in trace] for s in registers]
                matrix = DeviceVector.from_bytes(b"".join(_sc.pack(list(map(_sc._value_of, column))) for column in lists))
                columns = [DeviceCodeword(DeviceVector.wrap(matrix.ptr + 16 * trace_rows * s, trace_rows, matrix), field, elements=lists[s]) for s in registers]
            elif on_device:
                columns = [DeviceCodeword.from_list([row[s] for row in trace], field) for s in registers]
        interpolants = self.boundary_interpolants(boundary)
        zerofiers = self.boundary_zerofiers(boundary)
        # Checks the reference makes on the spot and nothing but an assertion reads -- a zero remainder of the boundary divisions
        # (univariate.py:99-103), "divide by zero" in the pointwise divisions (algebra.py:92) -- are decided on the device and COLLECTED
        # here; they are run where the prover has to wait for the device anyway, before the Fiat-Shamir challenge below, and raise
        # there what the reference raises at the division (the proof stream then holds the commitments pushed so far).
        pending = [] if on_device and not FastStark.EAGER_COMMITS else None
        if on_device:
            # Polynomials live in HBM from here on (DevicePolynomial): interpolation, boundary quotients (exact coset division,
            # exactness decided on the device), the AIR substitution in the value domain, the transition quotients, the LDEs and
            # the combination.  The host keeps what byte parity ties to it: os.urandom draws, Fiat-Shamir, the proof stream.
            trace_domain = self._trace_domain(trace_rows)
            if batched:
                # all registers in one set of launches, and their degrees in one host wait: minus() below and the transition
                # quotients find them known
                trace_polynomials = [DevicePolynomial.from_codeword(c) for c in fast_interpolate_columns_device(trace_domain, columns)]
                DevicePolynomial.degrees(trace_polynomials)
            else:
                trace_polynomials = [DevicePolynomial.from_codeword(fast_interpolate_device(trace_domain, column)) for column in columns]
            self._mark("trace interpolation")
            boundary_quotients = self._boundary_quotients_columns(trace_polynomials, interpolants, zerofiers, pending) if batched and FastStark.COLUMN_DIVIDE else None
            if boundary_quotients is None:
                zerofiers_dev = [DevicePolynomial.from_polynomial(z, field) for z in zerofiers]
                boundary_quotients = [coset_divide_device(trace_polynomials[s].minus(interpolants[s]), zerofiers_dev[s], self.generator, self.omicron,
                                                          self.omicron_domain_length, exact=True, later=pending) for s in registers]
            lde = lambda poly: poly.coset_evaluate(self.generator, self.omega, self.fri_domain_length)
        else:
            # trace polynomials through {omicron^i}
            trace_domain = [self.omicron ^ i for i in range(trace_rows)]
            trace_polynomials = [fast_interpolate(trace_domain, [row[s] for row in trace], self.omicron, self.omicron_domain_length) for s in registers]
            # boundary quotients (exact schoolbook division by the small boundary zerofiers)
            boundary_quotients = [(trace_polynomials[s] - interpolants[s]) / zerofiers[s] for s in registers]
            lde = self._lde

        self._mark("boundary quotients (division)")
        # commit to their low-degree extensions
        boundary_quotient_codewords = []
        # a commitment whose codeword lives on the device is pushed as "the root of this tree, once it is built" (proof_objects.RootLater):
        # the stream's first reader -- the Fiat-Shamir challenge below -- waits for it, the GPU queue never does
        later = _po.lazy_objects(proof_stream) if on_device and not FastStark.EAGER_COMMITS else None

        def commit(codeword):
            if self.row_commitments:
                return                                   # (committed together, in the row tree below the randomizer's LDE)
            if later is not None and isinstance(codeword, DeviceCodeword):
                later.add(_po.RootLater(codeword.start_tree()))
            else:
                proof_stream.push(Merkle.commit(codeword))
        if on_device and batched:
            boundary_quotient_codewords = self._lde_columns(boundary_quotients)
            for s in registers:
                commit(boundary_quotient_codewords[s])
        else:
            for s in registers:
                boundary_quotient_codewords.append(lde(boundary_quotients[s]))
                commit(boundary_quotient_codewords[s])
        self._mark("boundary quotient LDEs + commitments")

        # transition polynomials: AIR evaluated symbolically in (X, trace(X), trace(omicron X)), then quotients
        x = Polynomial([field.zero(), field.one()])
        point = [DevicePolynomial.from_polynomial(x, field) if on_device else x] + trace_polynomials + \
                [tp.scaled_later(self.omicron) if on_device else tp.scale(self.omicron) for tp in trace_polynomials]
        if on_device:
            transition_quotients = self._transition_quotients_on_device(transition_constraints, point, self._lift(transition_zerofier), pending, batched)
        else:
            if isinstance(transition_zerofier, DevicePolynomial):
                # preprocess(device_resident=True) with a trace shorter than DEVICE_MIN: the host-list data flow divides host polynomials
                transition_zerofier = transition_zerofier.to_polynomial()
            transition_polynomials = [a.evaluate_symbolic(point) for a in transition_constraints]
            transition_quotients = [fast_coset_divide(tp, transition_zerofier, self.generator, self.omicron, self.omicron_domain_length) for tp in transition_polynomials]

        self._mark("AIR substitution + transition quotients (value domain)")
        # randomizer polynomial
        max_degree = self.max_degree(transition_constraints)
        if on_device:
            # the same draws (max_degree + 1 times os.urandom(17), fast_stark.py:117), sampled into HBM without a Python object each
            randomizer_polynomial = random_polynomial(max_degree + 1, field)
        else:
            randomizer_polynomial = Polynomial([field.sample(os.urandom(17)) for i in range(max_degree + 1)])
        self._mark("randomizer polynomial: os.urandom / getrandom draws and Field.sample")
        randomizer_codeword = lde(randomizer_polynomial)
        commit(randomizer_codeword)
        row_tree = None
        if self.row_commitments:
            # ONE tree over the rows of [boundary quotients ..., randomizer]: one root, pushed where the randomizer's would be
            row_columns = boundary_quotient_codewords + [randomizer_codeword]
            if later is not None and all(isinstance(c, DeviceCodeword) for c in row_columns):
                row_tree = _sc.RowTree.start(row_columns)
                later.add(_po.RootLater(row_tree))
            elif Merkle._on_device(row_columns, len(randomizer_codeword)):
                row_tree = _sc.RowTree.build(row_columns)
                proof_stream.push(row_tree.root)
            else:
                proof_stream.push(Merkle.commit_rows(row_columns))
        self._mark("randomizer polynomial: LDE, commitment")

        _collect_verdicts(pending or ())                 # the collected checks: the device has long decided them
        # Fiat-Shamir weights: 1 randomizer + 2 per transition quotient + 2 per boundary quotient
        weights = self.sample_weights(1 + 2 * len(transition_quotients) + 2 * len(boundary_quotients), proof_stream.prover_fiat_shamir())
        tq_bounds = self.transition_quotient_degree_bounds(transition_constraints)
        assert([tq.degree() for tq in transition_quotients] == tq_bounds), "transition quotient degrees do not match with expectation"

        # nonlinear combination: each quotient and its degree-shifted copy
        bq_bounds = self.boundary_quotient_degree_bounds(trace_rows, boundary)
        shifted = [(randomizer_polynomial, None)]
        for i, tq in enumerate(transition_quotients):
            shifted.append((tq, max_degree - tq_bounds[i]))
        for i in registers:
            shifted.append((boundary_quotients[i], max_degree - bq_bounds[i]))
        if on_device:
            combined_codeword = self._combine_on_device(shifted, weights, max_degree, batched and FastStark.COLUMN_COMBINE)
            self._mark("weights, degree checks, nonlinear combination + its LDE")
        else:
            terms = []
            for poly, shift in shifted:
                terms += [poly] if shift is None else [poly, (x ^ shift) * poly]
            combination = reduce(lambda a, b: a + b, [Polynomial([weights[i]]) * terms[i] for i in range(len(terms))], Polynomial([]))
            combined_codeword = self._lde(combination)

        # low-degree test of the combination; the openings of the committed codewords depend on the same sampled indices, so they
        # are fetched in the query phase's own device round trip (AlsoOpen) when every codeword lives on the device
        N = self.fri.domain_length
        committed = boundary_quotient_codewords + [randomizer_codeword, transition_zerofier_codeword]
        if self.row_commitments:
            committed = [transition_zerofier_codeword]   # (the others open as rows of the row tree, in front of these)

        def opened_positions(indices):
            # the queried positions and their expansion_factor / half-domain companions (fast_stark.py:154-158)
            duplicated_indices = [i for i in indices] + [(i + self.expansion_factor) % N for i in indices]
            quadrupled_indices = [i for i in duplicated_indices] + [(i + (N // 2)) % N for i in duplicated_indices]
            quadrupled_indices.sort()
            return quadrupled_indices
        together = None
        if all(_po.eligible(codeword) for codeword in committed) and type(proof_stream) is ProofStream:
            together = AlsoOpen(lambda indices: (committed, [opened_positions(indices)] * len(committed)), codewords=committed, shift=self.expansion_factor)
        indices = self.fri.prove(combined_codeword, proof_stream, together) if together is not None else self.fri.prove(combined_codeword, proof_stream)
        self._mark("FRI: commit + query phases, openings fetched with them")

        quadrupled_indices = opened_positions(indices)
        if self.row_commitments:
            self._open_rows(row_tree, row_columns, quadrupled_indices, proof_stream)
        lazy = _po.lazy_objects(proof_stream) if all(_po.eligible(codeword) for codeword in committed) else None
        if lazy is not None:
            # the device's answers as they are (proof_objects.Openings): same transcript bytes, no object per digest
            answers = together.answers if together is not None and together.answers is not None else _sc.query_codewords_raw(committed, [quadrupled_indices] * len(committed))
            arrays = together.position_arrays if together is not None and together.answers is answers and together.position_arrays else [None] * len(committed)
            for codeword, (values, paths), where in zip(committed, answers, arrays):
                lazy.add(_po.Openings(codeword, quadrupled_indices, values, paths, where))
        elif all(isinstance(codeword, DeviceCodeword) for codeword in committed):
            # every codeword's openings in ONE device round trip; pushed leaf, path, leaf, path, ... codeword by codeword
            for entries, paths in query_codewords(committed, [quadrupled_indices] * len(committed)):
                self._push_openings(entries, paths, proof_stream)
        else:
            for codeword in committed:
                self._open_all(codeword, quadrupled_indices, proof_stream)

        self._mark("openings of the committed codewords")
        proof = proof_stream.serialize()
        self._mark("proof serialization (host pickle)")
        return proof

    # -- batched prover ----------------------------------------------------------------------------
    def _batch_served(self, traces, boundaries):
        """does prove_batch serve this batch with the members' work done together?  Decided from shapes alone, before any draw:
        the main field, traces of one length (long enough for the device data flow) and of one column per register, boundaries that
        name the same (cycle, register) pairs, an FRI shape the forest path serves, and a member's codewords within one forest"""
        if self.row_commitments:
            return False                                 # (served by the per-codeword forests; a row-committed batch: _rows_batch_served)
        return self._batch_shapes_served(traces, boundaries)

    def _rows_batch_served(self, traces, boundaries):
        """_batch_served for a prover with row_commitments: the same shape rules, and a row of R boundary quotients and the randomizer
        within a row tree's width.  Such a batch commits every member's codewords in ONE row forest (starkcore.RowForest)."""
        if not self.row_commitments or self.num_registers + 1 > _sc.ROWS_MAX_COLUMNS:
            return False
        return self._batch_shapes_served(traces, boundaries)

    def _batch_shapes_served(self, traces, boundaries):
        if self.field.p != Field.P_MAIN:
            return False
        rows = len(traces[0])
        if any(len(trace) != rows for trace in traces) or rows < 1 or rows + self.num_randomizers < FastStark.DEVICE_MIN:
            return False
        for trace in traces:
            if isinstance(trace, DeviceTrace):
                if len(trace.columns) != self.num_registers or trace.field.p != Field.P_MAIN:
                    return False
            elif any(len(row) != self.num_registers for row in trace):
                return False
        layout = [(cycle, register) for cycle, register, _ in boundaries[0]]
        if any([(cycle, register) for cycle, register, _ in boundary] != layout for boundary in boundaries):
            return False
        if self.num_registers * self.fri_domain_length > _sc.FOREST_MAX_LEAVES:
            return False
        return self.fri._batchable([])

    def prove_batch(self, traces, transition_constraints, boundaries, transition_zerofier, transition_zerofier_codeword, proof_streams=None):
        """[self.prove(traces[m], transition_constraints, boundaries[m], transition_zerofier, transition_zerofier_codeword,
        proof_streams[m]) for m ...] -- byte for byte under the same os.urandom, and afterwards every stream holds exactly the objects
        `prove` would have pushed -- with the members' work on the device done together: the randomized traces of all members are the
        K R columns of one matrix (sc_randomized_columns_dev: one launch copies the traces and samples the randomizer rows), and
        interpolation, the boundary quotients, the LDEs, the AIR, the nonlinear combination and FRI are one call each for all members
        (fast_interpolate_columns_device, combine_columns_device, coset_divide_columns_device, transition_quotients_batch,
        Fri.prove_batch with AlsoOpenForests); every commitment is a Merkle forest -- with row_commitments ONE row forest of K trees
        over the boundary-quotient and randomizer matrices (starkcore.RowForest) in place of the forests of those codewords, its rows
        opened by one launch behind FRI's.  traces[m]: a DeviceTrace or the reference's list of
        rows; proof_streams None: fresh ProofStreams.  The draws are made first, in the order of K sequential `prove` calls (per member
        num_randomizers * num_registers draws for the randomizer rows, then max_degree + 1 for the randomizer polynomial); with the
        operating system's os.urandom they are ONE os.urandom call.  A batch whose shape is not served (_batch_served, or
        _rows_batch_served with row_commitments) goes member by
        member through `prove`, before any draw.  A false witness raises what `prove` raises for the lowest-numbered failing member; no
        proofs are returned, and every stream then holds a prefix of what `prove` would have pushed.  COLUMN_BATCH_MIN is not consulted:
        K R columns always form a matrix."""
        traces, boundaries = list(traces), list(boundaries)
        proof_streams = [None] * len(traces) if proof_streams is None else list(proof_streams)
        assert(len(traces) == len(boundaries) == len(proof_streams)), "prove_batch needs one boundary and one proof stream per trace"
        if not traces:
            return []
        proof_streams = [ProofStream() if stream is None else stream for stream in proof_streams]
        if not (self._batch_served(traces, boundaries) or self._rows_batch_served(traces, boundaries)):
            return [self.prove(trace, transition_constraints, boundary, transition_zerofier, transition_zerofier_codeword, stream)
                    for trace, boundary, stream in zip(traces, boundaries, proof_streams)]
        K, R = len(traces), self.num_registers
        for_rows, for_polynomial = self.num_randomizers * R, self.max_degree(transition_constraints) + 1
        block = 17 * (for_rows + for_polynomial)
        if os_urandom_is_genuine():
            raw = os.urandom(K * block)
        else:
            raw = b"".join(draw_random_bytes(for_rows) + draw_random_bytes(for_polynomial) for _ in range(K))
        draws = (ctypes.c_char * (K * block)).from_buffer_copy(raw)
        step = max(1, _sc.FOREST_MAX_LEAVES // (R * self.fri_domain_length))
        proofs = []
        for lo in range(0, K, step):
            proofs += self._prove_chunk(traces[lo:lo + step], transition_constraints, boundaries[lo:lo + step], transition_zerofier,
                                        transition_zerofier_codeword, proof_streams[lo:lo + step], ctypes.addressof(draws) + lo * block, block)
        return proofs

    def _trace_matrix(self, traces, rows):
        """the traces of a chunk as one device matrix of K R columns: (holder of the device pointer, column pitch in elements).
        DeviceTraces whose columns already are equally spaced rows of one matrix (RescuePrime.trace_batch_device's output) are used where
        they lie; other DeviceTraces are copied into one matrix; host rows are packed and uploaded once."""
        R, lib = self.num_registers, _sc.lib()
        if all(isinstance(trace, DeviceTrace) for trace in traces):
            vectors = [column for trace in traces for column in trace.columns]
            places = [v.ptr for v in vectors]
            pitch = places[1] - places[0] if len(places) > 1 else 16 * rows
            if pitch >= 16 * rows and pitch % 16 == 0 and all(b - a == pitch for a, b in zip(places, places[1:])):
                return vectors[0], pitch // 16
        value = lambda x: int(getattr(x, "value", x))
        if not any(isinstance(trace, DeviceTrace) for trace in traces):
            return DeviceVector.from_bytes(b"".join(_sc.pack([value(row[s]) for row in trace]) for trace in traces for s in range(R))), rows
        matrix = DeviceVector(len(traces) * R * rows)
        for m, trace in enumerate(traces):
            if isinstance(trace, DeviceTrace):
                for s, column in enumerate(trace.columns):
                    _sc._check(lib.sc_memcpy_dev(matrix.ptr + 16 * rows * (m * R + s), column.ptr, rows, None))
            else:
                _sc._check(lib.sc_vec_upload(matrix._h, rows * m * R, b"".join(_sc.pack([value(row[s]) for row in trace]) for s in range(R)), rows * R))
        return matrix, rows

    def _zerofier_forest(self, codeword):
        """the count-1 Merkle forest over the transition zerofier's codeword (its root is Merkle.commit's), built once per codeword object"""
        kept = getattr(self, "_zerofier_forest_kept", None)
        if kept is None or kept[0] is not codeword:
            kept = self._zerofier_forest_kept = (codeword, _sc.MerkleForest.build(_sc.CodewordMatrix.from_members([codeword])))
        return kept[1]

    def _prove_chunk(self, traces, transition_constraints, boundaries, transition_zerofier, transition_zerofier_codeword, streams, draws, draws_stride):
        """prove_batch for members that share every forest.  draws: address of the first member's block of draws (host memory)"""
        field, lib, K, R = self.field, _sc.lib(), len(traces), self.num_registers
        rows, extra = len(traces[0]), self.num_randomizers
        trace_rows, cols, N = rows + extra, K * R, self.fri_domain_length
        max_degree = self.max_degree(transition_constraints)
        self._mark(None)
        pending = []
        try:
            # the randomized traces of all members as one matrix [K R][trace_rows], the randomizer polynomials as one [K][max_degree + 1]
            source, ld_trace = self._trace_matrix(traces, rows)
            randomized = DeviceVector(cols * trace_rows)
            _sc._check(lib.sc_randomized_columns_dev(source.ptr, rows, ld_trace, K, R, draws, draws_stride, extra, 17, randomized.ptr, trace_rows, None))
            sampled = DeviceVector(K * (max_degree + 1))
            _sc._check(lib.sc_randomized_columns_dev(None, 0, 0, K, 1, draws + 17 * extra * R, draws_stride, max_degree + 1, 17, sampled.ptr, max_degree + 1, None))
            randomizer_polynomials = [DevicePolynomial(DeviceVector.wrap(sampled.ptr + 16 * (max_degree + 1) * m, max_degree + 1, sampled), field, max_degree + 1)
                                      for m in range(K)]
            columns = [DeviceCodeword(DeviceVector.wrap(randomized.ptr + 16 * trace_rows * c, trace_rows, randomized), field) for c in range(cols)]
            trace_polynomials = [DevicePolynomial.from_codeword(c) for c in fast_interpolate_columns_device(self._trace_domain(trace_rows), columns)]
            DevicePolynomial.degrees(trace_polynomials)
            self._mark("trace interpolation")

            # boundary quotients of all K R columns: one combination, one columns-form division, one verdict
            interpolants = [interpolant for boundary in boundaries for interpolant in self.boundary_interpolants(boundary)]
            zerofiers = self.boundary_zerofiers(boundaries[0])
            boundary_quotients = self._boundary_quotients_columns(trace_polynomials, interpolants, zerofiers * K, pending)
            if boundary_quotients is None:
                zerofiers_dev = [DevicePolynomial.from_polynomial(z, field) for z in zerofiers]
                boundary_quotients = [coset_divide_device(trace_polynomials[c].minus(interpolants[c]), zerofiers_dev[c % R], self.generator, self.omicron,
                                                          self.omicron_domain_length, exact=True, later=pending) for c in range(cols)]
            self._mark("boundary quotients (division)")

            # commitments: one forest over the K R boundary-quotient codewords, one over the K randomizer codewords, the zerofier's own;
            # with row_commitments ONE row forest of K trees over both matrices, built behind the randomizer's LDE
            rows_on = self.row_commitments
            bq_matrix = self._lde_matrix(boundary_quotients)
            bq_forest = None if rows_on else _sc.MerkleForest.build(bq_matrix)
            self._mark("boundary quotient LDEs + commitments")
            x = DevicePolynomial.from_polynomial(Polynomial([field.zero(), field.one()]), field)
            points = [[x] + trace_polynomials[m * R:(m + 1) * R] + [tp.scaled_later(self.omicron) for tp in trace_polynomials[m * R:(m + 1) * R]] for m in range(K)]
            transition_quotients = self.transition_quotients_batch(transition_constraints, points, transition_zerofier, pending)
            self._mark("AIR substitution + transition quotients (value domain)")
            randomizer_matrix = self._lde_matrix(randomizer_polynomials)
            if rows_on:
                # tree m: the rows of [member m's R boundary-quotient codewords, its randomizer codeword] -- prove's row tree
                row_forest = _sc.RowForest.build([(bq_matrix, R), (randomizer_matrix, 1)], N, K)
            else:
                randomizer_forest = _sc.MerkleForest.build(randomizer_matrix)
            zerofier_forest = self._zerofier_forest(transition_zerofier_codeword)
            self._mark("randomizer polynomial: LDE, commitment")

            # per member: the commitments, the collected checks (once: they speak for the whole chunk), the weights, the degree check
            tq_bounds = self.transition_quotient_degree_bounds(transition_constraints)
            bq_bounds = self.boundary_quotient_degree_bounds(trace_rows, boundaries[0])
            if rows_on:
                row_roots = row_forest.roots
            else:
                bq_roots, randomizer_roots = bq_forest.roots, randomizer_forest.roots
            weights = []
            for m, stream in enumerate(streams):
                if rows_on:
                    stream.push(row_roots[m])            # (one root, where prove pushes its row tree's)
                else:
                    for s in range(R):
                        stream.push(bq_roots[m * R + s])
                    stream.push(randomizer_roots[m])
                checks, pending = pending, []
                _collect_verdicts(checks)
                weights.append(self.sample_weights(1 + 2 * len(transition_quotients[m]) + 2 * R, stream.prover_fiat_shamir()))
                assert([tq.degree() for tq in transition_quotients[m]] == tq_bounds), "transition quotient degrees do not match with expectation"
        except BaseException:
            _drop_verdicts(pending)                      # no check is left unread: none keeps its pinned slot
            raise

        # nonlinear combination of every member in one pass: every term is a K-row matrix, the weight row is the member's
        terms = [(randomizer_polynomials, None)]
        for i in range(len(transition_constraints)):
            terms.append(([transition_quotients[m][i] for m in range(K)], max_degree - tq_bounds[i]))
        for s in range(R):
            terms.append(([boundary_quotients[m * R + s] for m in range(K)], max_degree - bq_bounds[s]))
        width = max(max_degree + 1, max(len(p) + (shift or 0) for polynomials, shift in terms for p in polynomials))
        combined = self._lde_matrix(combine_columns_device(terms, weights, width))
        combined_codewords = [DeviceCodeword(DeviceVector.wrap(combined.vec.ptr + 16 * N * m, N, combined.vec), field) for m in range(K)]
        self._mark("weights, degree checks, nonlinear combination + its LDE")

        # FRI on all members; the committed codewords' openings travel in the launch that fetches the FRI openings
        if rows_on:
            # (the rows open from the row forest, in a launch of their own behind FRI's: below)
            also = AlsoOpenForests([zerofier_forest], [[[0]] * K], shift=self.expansion_factor)
        else:
            owners = [[list(range(m * R, (m + 1) * R)) for m in range(K)], [[m] for m in range(K)], [[0] for _ in range(K)]]
            also = AlsoOpenForests([bq_forest, randomizer_forest, zerofier_forest], owners, shift=self.expansion_factor)
        self.fri.prove_batch(combined_codewords, streams, also_open=also)
        self._mark("FRI: commit + query phases, openings fetched with them")

        if rows_on:
            # every member's rows at its positions in ONE launch; per member row, path, row, path, ... in front of the zerofier's openings
            w, at = R + 1, 0
            row_values, row_paths = row_forest.query_raw([(m, position) for m in range(K) for position in also.positions[m]])
            for m, stream in enumerate(streams):
                k = len(also.positions[m])
                self._push_rows(stream, also.positions[m], row_values[16 * w * at:16 * w * (at + k)], row_paths[at:at + k], w)
                at += k

        # openings in `committed` order; entries are made once per (member, codeword, index): the transcript is pickled by object identity
        proofs = []
        shared_elements = None if isinstance(transition_zerofier_codeword, DeviceCodeword) else list(transition_zerofier_codeword)
        for m, stream in enumerate(streams):
            holders = [DeviceCodeword(None, field) for _ in range(0 if rows_on else R + 1)] + [DeviceCodeword(None, field, elements=shared_elements)]
            for holder, (values, paths) in zip(holders, also.answers[m]):
                self._push_openings(holder._entries(also.positions[m], values), paths, stream)
        self._mark("openings of the committed codewords")
        for stream in streams:
            proofs.append(stream.serialize())
        self._mark("proof serialization (host pickle)")
        return proofs

    def _lde_matrix(self, polynomials):
        """the codewords of _lde_columns as the rows of one CodewordMatrix (no copy: what a MerkleForest is built over)"""
        codewords = self._lde_columns(polynomials)
        return _sc.CodewordMatrix(len(codewords), self.fri_domain_length, codewords[0].vec._keep)

    def _lde_columns(self, polynomials):
        """[p.coset_evaluate(generator, omega, fri_domain_length) for p in polynomials] as one call: the coefficient vectors are
        zero-padded to the longest in one matrix (the padding evaluates to the same values) and the codewords are views of the
        rows of one codeword matrix"""
        lib, count, order = _sc.lib(), len(polynomials), self.fri_domain_length
        m = max(max(len(p) for p in polynomials), 1)
        coefficients = DeviceVector.zeros(count * m)
        for c, p in enumerate(polynomials):
            if len(p):
                _sc._check(lib.sc_memcpy_dev(coefficients.ptr + 16 * m * c, p.vec.ptr, len(p), None))
        values = DeviceVector(count * order)
        _sc._check(lib.sc_coset_evaluate_columns_dev(coefficients.ptr, m, count, _sc.fe_bytes(self.generator.value), _sc.fe_bytes(self.omega.value), order, values.ptr, None))
        return [DeviceCodeword(DeviceVector.wrap(values.ptr + 16 * order * c, order, values), self.field) for c in range(count)]

    @staticmethod
    def _with_public_columns(constraints, points):
        """Constraints with public columns (multivariate.XColumnsConstraint) that all share ONE set of columns, as the value-domain AIR
        takes them: their inner polynomials (small exponents, a dictionary each) over points extended by the columns' DevicePolynomials
        -- every member's point by the same objects, so that a batch evaluates them once, like X.  The columns are then variables like
        any other: all constraints of an order share one evaluation of the point and, in a batch, one AIR launch.  Any other list of
        constraints, and its points, come back as they are."""
        columns = getattr(constraints[0], "columns", None) if constraints else None
        if columns is None or not points or any(getattr(a, "columns", None) is not columns for a in constraints):
            return constraints, points
        lifted = columns.device(points[0][0].field)
        return [a.inner for a in constraints], [list(point) + lifted for point in points]

    def _transition_quotients_on_device(self, constraints, point, tz_dev, pending=None, batched=False):
        """fast_stark.py:107-113 -- `a.evaluate_symbolic(point)` divided by the transition zerofier -- without ever building the
        transition polynomial: on the coset g * <root'> (root' of the order code/ntt.py:155-157 shrinks to, taken from the degree
        BOUND) the point polynomials are evaluated once for all constraints of that order, the AIR is evaluated value by value
        (mpoly_eval_kernel), divided pointwise by the zerofier's values, and one inverse transform per constraint returns the
        quotient's coefficients: 4 + 2 transforms for the two-register AIR instead of the 9 + 4 of "substitute, then divide".
        The same polynomial as the reference's: an exact division gives the same quotient on any coset that is large enough, and
        its list length is its degree + 1.  Exactness is DECIDED, not assumed: the interpolant Q of the pointwise quotient satisfies
        Q * Z = transition polynomial as polynomials whenever deg Q <= bound - deg Z (both sides then have degree below the order
        and agree on the coset); a longer interpolant means the division is not exact (a false witness), and the reference's
        result then depends on the transition polynomial's true degree -- that constraint goes the reference's way
        (evaluate_symbolic, then coset_divide_device), as does any shape the kernel does not take (sharded_stark.py does the same
        on slabs)."""
        field = self.field
        constraints, (point,) = self._with_public_columns(list(constraints), [point])
        reference_way = lambda a: coset_divide_device(a.evaluate_symbolic(point), tz_dev, self.generator, self.omicron, self.omicron_domain_length)
        degrees = [q.degree() for q in point]
        dr = tz_dev.degree()
        out, groups = [None] * len(constraints), {}
        for i, a in enumerate(constraints):
            plan = a.value_domain_terms(degrees)
            if plan is NotImplemented or dr < 0 or plan[0] < max(dr, MPolynomial.VALUE_DOMAIN_MIN_DEGREE):
                continue
            bound, terms = plan
            root, order = _shrink_order(self.omicron, self.omicron_domain_length, max(bound, dr))
            if len(tz_dev) > order or any(len(q) > order for q in point):
                continue
            groups.setdefault(order, (root, []))[1].append((i, bound, terms))
        lib, gen = _sc.lib(), _sc.fe_bytes(self.generator.value)
        for order, (root, members) in groups.items():
            nvars, rt = len(point), _sc.fe_bytes(root.value)
            used = [any(k[j] for _, _, terms in members for k, _ in terms) for j in range(nvars)]
            # q(root X) on the coset g <root> is q's codeword there, one place on: such a variable (the trace polynomials at
            # omicron X, fast_stark.py:105-106, whenever the coset's root is omicron itself) is read off its source's values
            # instead of being scaled and transformed
            turned = {}
            for j, q in enumerate(point):
                source = getattr(q, "scaled_from", None)
                if used[j] and source is not None and source[1].value == root.value:
                    k = next((k for k, other in enumerate(point) if other is source[0]), None)
                    if k is not None and getattr(point[k], "scaled_from", None) is None:
                        turned[j] = k
            stored = [(used[j] and j not in turned) or j in turned.values() for j in range(nvars)]
            vals = DeviceVector(nvars * order)
            in_runs = self._evaluate_runs(point, stored, rt, order, vals) if batched else ()
            for j, q in enumerate(point):
                if stored[j] and j not in in_runs:
                    source = getattr(q, "scaled_from", None)
                    if source is not None:
                        # q(f X) on g <root> is q on (g f) <root>: the transform's own offset does the scaling, the scaled
                        # coefficient vector is never made
                        shifted = _sc.fe_bytes((self.generator * source[1]).value)
                        _sc._check(lib.sc_coset_evaluate_dev(source[0].vec.ptr, degrees[j] + 1, shifted, rt, order, vals.ptr + 16 * j * order, None))
                    else:
                        _sc._check(lib.sc_coset_evaluate_dev(q.vec.ptr, degrees[j] + 1, gen, rt, order, vals.ptr + 16 * j * order, None))
            var_src = (ctypes.c_uint32 * nvars)(*[turned.get(j, j if stored[j] else 0xFFFFFFFF) for j in range(nvars)])
            var_rot = (ctypes.c_uint64 * nvars)(*[1 if j in turned else 0 for j in range(nvars)])
            kept = self._zerofier_values.get(order)
            if kept is not None and kept[0] is tz_dev:
                zvals = kept[1]
            else:
                zvals = DeviceVector(order)
                _sc._check(lib.sc_coset_evaluate_dev(tz_dev.vec.ptr, dr + 1, gen, rt, order, zvals.ptr, None))
                if len(self._zerofier_values) >= 4:
                    self._zerofier_values.clear()
                self._zerofier_values[order] = (tz_dev, zvals)
            converted = 0
            for i, bound, terms in members:
                exps = bytes(e for k, _ in terms for e in k)
                coefs = b"".join(v.to_bytes(16, "little") for _, v in terms)
                tvals, whole = DeviceVector(order), DeviceVector(order)
                _sc._check(lib.sc_mpoly_eval_rot_dev(vals.ptr, nvars, order, exps, coefs, len(terms), tvals.ptr, converted, var_src, var_rot, None))
                converted = 1
                self._pointwise_divide(tvals, zvals, order, pending)                                    # "divide by zero" like algebra.py:92
                _sc._check(lib.sc_ntt_dev(tvals.ptr, whole.ptr, order, rt, 1, None))
                _sc._check(lib.sc_scale_dev(whole.ptr, whole.ptr, order, _sc.fe_bytes(self.generator.inverse().value), None))
                quotient = DevicePolynomial(whole, field, order)
                degree = quotient.degree()
                if degree > bound - dr:
                    continue                                             # not exact: the reference's way decides what comes out
                out[i] = DevicePolynomial(whole, field, degree + 1) if degree >= 0 else DevicePolynomial(DeviceVector(1), field, 0)
                out[i]._degree = degree                                  # just read: the degree check of fast_stark.py:124 need not ask the device again
        return [q if q is not None else reference_way(a) for q, a in zip(out, constraints)]

    def transition_quotients_batch(self, transition_constraints, points, transition_zerofier, pending=None):
        """[self._transition_quotients_on_device(transition_constraints, point, zerofier, pending) for point in points] -- the same
        DevicePolynomials, coefficient for coefficient and degree for degree -- for the members of a batch of proofs (points[m]: X, the
        trace polynomials, their scaled_later(omicron) copies, as `prove` builds them), with the work of each value-domain order done
        for all members together: the stored variables evaluated by one sc_coset_evaluate_columns_dev per run of consecutive
        equal-length coefficient rows (ONE call for all members when their trace polynomials are the rows of one matrix), X -- the
        same object in every point -- and the zerofier once, the AIR of all members and constraints in ONE launch
        (sc_mpoly_eval_columns_dev), ONE pointwise division with one verdict (appended to `pending`, or waited for on the spot: "divide
        by zero"), ONE inverse transform, ONE scaling by g^-i and ONE degree call with one host wait.  The quotients are views of the
        rows of one matrix.  What the batched calls do not serve goes through the per-member method, unchanged: a (member, constraint)
        whose interpolant is longer than bound - deg Z (a false witness), a constraint of a shape or bound the value domain does not
        take, and members whose points differ in length or structure; members of different degrees are batched among their likes."""
        constraints, points = self._with_public_columns(list(transition_constraints), [list(point) for point in points])
        tz_dev = self._lift(transition_zerofier)
        in_runs = self.num_registers >= FastStark.COLUMN_BATCH_MIN          # (as `prove` decides it)
        one_member = lambda m, some: self._transition_quotients_on_device(some, points[m], tz_dev, pending, in_runs)
        DevicePolynomial.degrees([q for point in points for q in point if type(q) is DevicePolynomial])      # one wait for those not known yet
        out, alike = [None] * len(points), {}
        for m, point in enumerate(points):
            degrees = tuple(q.degree() for q in point)
            # where every variable comes from: (index of its unscaled source in the point, the factor), None for a polynomial of its own
            structure = []
            for q in point:
                source = getattr(q, "scaled_from", None)
                k = next((k for k, other in enumerate(point) if other is source[0]), None) if source is not None else None
                if source is not None and (k is None or getattr(point[k], "scaled_from", None) is not None):
                    structure = None                     # scaled off something outside the point: the per-member method knows what to do
                    break
                structure.append(None if source is None else (k, source[1].value))
            if structure is None or self.field.p != Field.P_MAIN:
                out[m] = one_member(m, constraints)
            else:
                alike.setdefault((degrees, tuple(structure)), []).append(m)
        for (degrees, structure), members in alike.items():
            for m, quotients in zip(members, self._transition_quotients_alike(constraints, points, members, degrees, structure, tz_dev, pending, one_member)):
                out[m] = quotients
        return out

    def _transition_quotients_alike(self, constraints, points, members, degrees, structure, tz_dev, pending, one_member):
        """transition_quotients_batch for members whose points have the same degrees and the same structure"""
        field, lib, gen = self.field, _sc.lib(), _sc.fe_bytes(self.generator.value)
        dr = tz_dev.degree()
        K, nvars = len(members), len(degrees)
        out, groups = [[None] * len(constraints) for _ in members], {}
        for i, a in enumerate(constraints):
            plan = a.value_domain_terms(list(degrees))
            if plan is NotImplemented or dr < 0 or plan[0] < max(dr, MPolynomial.VALUE_DOMAIN_MIN_DEGREE):
                continue
            bound, terms = plan
            root, order = _shrink_order(self.omicron, self.omicron_domain_length, max(bound, dr))
            if len(tz_dev) > order or any(len(q) > order for m in members for q in points[m]):
                continue
            groups.setdefault(order, (root, []))[1].append((i, bound, terms))
        for order, (root, group) in groups.items():
            rt, C = _sc.fe_bytes(root.value), len(group)
            used = [any(k[j] for _, _, terms in group for k, _ in terms) for j in range(nvars)]
            # a variable scaled by the coset's own root is its source's codeword, one place on (see _transition_quotients_on_device)
            turned = {j: s[0] for j, s in enumerate(structure) if used[j] and s is not None and s[1] == root.value}
            stored = [(used[j] and j not in turned) or j in turned.values() for j in range(nvars)]
            # a stored variable that is the same object in every point (X) has ONE row; the others a row per member, member after
            # member, so that coefficient rows that are consecutive in memory are evaluated into consecutive rows
            shared = [stored[j] and all(points[m][j] is points[members[0]][j] for m in members) for j in range(nvars)]
            own = [j for j in range(nvars) if stored[j] and not shared[j]]
            common = [j for j in range(nvars) if shared[j]]
            vals = DeviceVector((K * len(own) + len(common)) * order)
            row_of = lambda t, j: t * len(own) + own.index(j) if not shared[j] else K * len(own) + common.index(j)
            self._evaluate_rows([(row_of(t, j), points[m][j], degrees[j]) for t, m in enumerate(members) for j in own] +
                                [(row_of(0, j), points[members[0]][j], degrees[j]) for j in common], rt, order, vals)
            var_base = (ctypes.c_uint64 * nvars)(*[row_of(0, j) * order if stored[j] else 0 for j in range(nvars)])
            var_ld = (ctypes.c_uint64 * nvars)(*[len(own) * order if stored[j] and not shared[j] else 0 for j in range(nvars)])
            var_src = (ctypes.c_uint32 * nvars)(*[turned.get(j, j if stored[j] else 0xFFFFFFFF) for j in range(nvars)])
            var_rot = (ctypes.c_uint64 * nvars)(*[1 if j in turned else 0 for j in range(nvars)])
            kept = self._zerofier_values.get(order)
            if kept is not None and kept[0] is tz_dev:
                zvals = kept[1]
            else:
                zvals = DeviceVector(order)
                _sc._check(lib.sc_coset_evaluate_dev(tz_dev.vec.ptr, dr + 1, gen, rt, order, zvals.ptr, None))
                if len(self._zerofier_values) >= 4:
                    self._zerofier_values.clear()
                self._zerofier_values[order] = (tz_dev, zvals)
            cols = K * C
            tvals, whole = DeviceVector(cols * order), DeviceVector(cols * order)
            counts, exps, coefs = MPolynomial.pack_terms([terms for _, _, terms in group])
            nterms = (ctypes.c_uint64 * C)(*counts)
            _sc._check(lib.sc_mpoly_eval_columns_dev(vals.ptr, nvars, order, K, var_base, var_ld, var_src, var_rot, C, nterms, exps, coefs, tvals.ptr, order, None))
            handle = ctypes.c_void_p()
            rc = lib.sc_pointwise_div_columns_later_dev(tvals.ptr, order, zvals.ptr, 0, tvals.ptr, order, order, cols, ctypes.byref(handle), None)
            if rc == _sc.SC_ERR_UNSUPPORTED:
                continue                                     # no pinned slot for the verdict: these constraints go member by member below
            _sc._check(rc)
            check = _sc.Later(handle)

            def verdict(check=check):
                assert(not check.wait()[0]), "divide by zero"       # like algebra.py:92
            if pending is not None:
                pending.append(verdict)
            else:
                verdict()
            _sc._check(lib.sc_ntt_columns_dev(tvals.ptr, whole.ptr, order, cols, rt, 1, None))
            _sc._check(lib.sc_scale_columns_dev(whole.ptr, order, whole.ptr, order, order, cols, _sc.fe_bytes(self.generator.inverse().value), None))
            found = (ctypes.c_int64 * cols)()
            _sc._check(lib.sc_vec_degree_columns_dev(whole.ptr, order, order, cols, found, None))
            for t in range(K):
                for c, (i, bound, _) in enumerate(group):
                    degree = int(found[t * C + c])
                    if degree > bound - dr:
                        continue                             # not exact: the per-member method decides what comes out
                    if degree >= 0:
                        out[t][i] = DevicePolynomial(DeviceVector.wrap(whole.ptr + 16 * order * (t * C + c), degree + 1, whole), field, degree + 1)
                    else:
                        out[t][i] = DevicePolynomial(DeviceVector(1), field, 0)
                    out[t][i]._degree = degree
        for t, m in enumerate(members):
            left = [i for i in range(len(constraints)) if out[t][i] is None]
            if left:
                for i, quotient in zip(left, one_member(m, [constraints[i] for i in left])):
                    out[t][i] = quotient
        return out

    def _evaluate_rows(self, rows, rt, order, vals):
        """rows: [(row of `vals`, polynomial, its degree)] in the order of the rows.  Every polynomial -- q, or for q = source(f X)
        its source at the offset g f: the transform's own offset does the scaling -- is evaluated on the coset g <root> of `order`
        points into its row: ONE sc_coset_evaluate_columns_dev per maximal run of coefficient vectors of one length and one offset
        that lie one behind the other in memory and go to consecutive rows (what _evaluate_runs does inside one point)."""
        lib = _sc.lib()

        def place(q, degree):
            source = getattr(q, "scaled_from", None)
            poly, offset = (source[0], self.generator * source[1]) if source is not None else (q, self.generator)
            if type(poly) is DevicePolynomial and len(poly):
                return poly.vec.ptr, len(poly), offset.value       # (all len(poly) coefficients go in: those above the degree are zeros)
            return poly.vec.ptr, degree + 1, offset.value
        at = 0
        while at < len(rows):
            row, q, degree = rows[at]
            first = place(q, degree)
            run = 1
            while at + run < len(rows) and rows[at + run][0] == row + run:
                following = place(rows[at + run][1], rows[at + run][2])
                if following[1:] != first[1:] or following[0] != first[0] + 16 * first[1] * run:
                    break
                run += 1
            if run >= 2:
                _sc._check(lib.sc_coset_evaluate_columns_dev(first[0], first[1], run, _sc.fe_bytes(first[2]), rt, order, vals.ptr + 16 * row * order, None))
            else:
                _sc._check(lib.sc_coset_evaluate_dev(first[0], first[1], _sc.fe_bytes(first[2]), rt, order, vals.ptr + 16 * row * order, None))
            at += run

    def _evaluate_runs(self, point, stored, rt, order, vals):
        """The stored variables whose coefficient vectors are consecutive rows of one matrix -- trace_s(X) for consecutive s, and
        trace_s(omicron X) where they are not read off the former -- evaluated into their (consecutive) places of `vals` by ONE
        sc_coset_evaluate_columns_dev per maximal run of equal length and equal offset (g, or g * omicron: the transform's own
        offset does the scaling).  Returns the variables served."""
        lib, done = _sc.lib(), set()

        def place(j):
            """(where variable j's coefficients are, how many, the offset they are evaluated at), None if they are not plain rows"""
            source = getattr(point[j], "scaled_from", None)
            poly, offset = (source[0], self.generator * source[1]) if source is not None else (point[j], self.generator)
            if type(poly) is not DevicePolynomial or len(poly) == 0:
                return None                                 # (all len(poly) coefficients go in: those above the degree are zeros)
            return poly.vec.ptr, len(poly), offset.value
        j, nvars = 0, len(point)
        while j < nvars:
            first = place(j) if stored[j] else None
            run = 1
            if first is not None:
                while j + run < nvars and stored[j + run]:
                    following = place(j + run)
                    if following is None or following[1:] != first[1:] or following[0] != first[0] + 16 * first[1] * run:
                        break
                    run += 1
            if first is not None and run >= 2:
                _sc._check(lib.sc_coset_evaluate_columns_dev(first[0], first[1], run, _sc.fe_bytes(first[2]), rt, order, vals.ptr + 16 * j * order, None))
                done.update(range(j, j + run))
            j += run
        return done

    @staticmethod
    def _pointwise_divide(numerator, denominator, count, pending):
        """numerator[i] /= denominator[i] on the device; with a list of pending checks the "divide by zero" verdict is collected, not waited for"""
        lib = _sc.lib()
        if pending is not None:
            handle = ctypes.c_void_p()
            rc = lib.sc_pointwise_div_later_dev(numerator.ptr, denominator.ptr, numerator.ptr, count, ctypes.byref(handle), None)
            if rc != _sc.SC_ERR_UNSUPPORTED:
                _sc._check(rc)
                check = _sc.Later(handle)

                def verdict():
                    assert(not check.wait()[0]), "divide by zero"
                pending.append(verdict)
                return
        _sc._check(lib.sc_pointwise_div_dev(numerator.ptr, denominator.ptr, numerator.ptr, count, None))

    def _randomized_columns(self, trace, raw, together=False):
        """the columns of a DeviceTrace with the randomizer rows appended (fast_stark.py:79-81): `raw` holds the draws of
        os.urandom(17) in the reference's order -- row by row, register by register; 4 * num_colinearity_checks rows, sampled on
        the host and written behind each column's copy"""
        assert(len(trace.columns) == self.num_registers), "one column per register"
        width, rows, extra = self.num_registers, len(trace), self.num_randomizers
        # Field.sample (algebra.py:116-120: big-endian accumulate, then % p) of every 17-byte draw, without an object per draw
        p, big = self.field.p, int.from_bytes
        columns = []
        matrix = DeviceVector(width * (rows + extra)) if together else None      # together: the columns are views of the rows of one matrix
        for s in range(width):
            tail = b"".join((big(raw[17 * (r * width + s):17 * (r * width + s) + 17], "big") % p).to_bytes(16, "little") for r in range(extra))
            column = DeviceVector(rows + extra) if matrix is None else DeviceVector.wrap(matrix.ptr + 16 * (rows + extra) * s, rows + extra, matrix)
            _sc._check(_sc.lib().sc_memcpy_dev(column.ptr, trace.columns[s].ptr, rows, None))
            if extra:
                _sc._check(_sc.lib().sc_vec_upload(column._h, rows, tail, extra))
            columns.append(DeviceCodeword(column, self.field))
        return columns

    def _boundary_quotients_columns(self, trace_polynomials, interpolants, zerofiers, pending):
        """(trace_s - interpolant_s) / zerofier_s for every register s in two library calls: the differences as one combination with
        weights 1 and p - 1 (the interpolants uploaded as one zero-padded matrix), then one columns-form coset division with a
        zerofier and a quotient length per register and ONE pending verdict.  None where the shape is not the batched call's -- an
        interpolant not of lower degree than its trace polynomial, trace polynomials of different degrees -- and the caller's
        per-register loop runs instead."""
        field = self.field
        degree = trace_polynomials[0].degree()
        short = [p.degree() for p in interpolants]
        if degree < 0 or any(t.degree() != degree for t in trace_polynomials) or max(short) >= degree:
            return None
        width = max(len(t) for t in trace_polynomials)
        subtrahends = DevicePolynomial.rows_from_polynomials(interpolants, field)
        numerators = combine_columns_device([(trace_polynomials, None), (subtrahends, None)], [[1, field.p - 1]] * len(interpolants), width)
        for numerator in numerators:
            numerator._degree = degree                     # a subtrahend of lower degree leaves the degree alone (DevicePolynomial.minus)
        divisors = DevicePolynomial.rows_from_polynomials(zerofiers, field)       # one matrix, one upload: the division reads it in place
        return coset_divide_columns_device(numerators, divisors, self.generator, self.omicron, self.omicron_domain_length, later=pending)

    def _combine_on_device(self, shifted, weights, max_degree, one_pass=False):
        """sum_i weights[i] * terms[i] (fast_stark.py:130-145) as axpys over coefficient vectors in HBM, then the LDE straight from
        the accumulator: `Polynomial([w]) * t` scales t, `(x ^ k) * t` shifts it by k places.  The combination never visits the host."""
        return self._combination_on_device(shifted, weights, max_degree, one_pass).coset_evaluate(self.generator, self.omega, self.fri_domain_length)

    def _combination_on_device(self, shifted, weights, max_degree, one_pass=False):
        width = max(max_degree + 1, max(len(p) + (k or 0) for p, k in shifted))
        if one_pass:
            # every term in one launch that writes each coefficient once (COLUMN_COMBINE): no zeroed accumulator, no launch per term
            return combine_columns_device([([poly], shift) for poly, shift in shifted], [weights], width)[0]
        acc = DeviceVector.zeros(width)
        w = iter(weights)
        for poly, shift in shifted:
            for k in ([0] if shift is None else [0, shift]):
                weight = next(w)
                if len(poly):
                    acc.axpy_shift(_View(poly.vec, len(poly)), k, weight.value)
        return DevicePolynomial(acc, self.field, width)

    def _open_all(self, codeword, indices, proof_stream):
        """leaf, path, leaf, path, ... for one codeword -- one resident tree, one batched gather of all paths."""
        if isinstance(codeword, DeviceCodeword):
            entries, paths = codeword.query(indices)          # entries and paths in one device round trip
        else:
            entries, paths = [codeword[i] for i in indices], Merkle._tree(codeword).open_batch(indices)
        self._push_openings(entries, paths, proof_stream)

    def _open_rows(self, row_tree, columns, indices, proof_stream):
        """row, path, row, path, ... of the row commitment: per position the list of every column's value there and ONE path.  A
        resident tree answers in one launch (RowTree.query), described to the stream without objects where the stream takes
        descriptions; the host-list data flow opens position by position (Merkle.open_rows)."""
        lazy = _po.lazy_objects(proof_stream) if row_tree is not None and all(_po.eligible(c) for c in columns) else None
        if lazy is not None:
            # the device's answers as they are (proof_objects.RowOpenings): no object per value or digest
            values, paths = row_tree.query_raw(indices)
            lazy.add(_po.RowOpenings(columns, indices, values, paths))
            return
        if row_tree is not None:
            rows, paths = row_tree.query(indices)
            field = self.field
            rows = [[FieldElement(v, field) for v in row] for row in rows]
        else:
            rows, paths = zip(*[Merkle.open_rows(i, columns) for i in indices]) if indices else ((), ())
        for row, path in zip(rows, paths):
            proof_stream.push(row)
            proof_stream.push(path)

    def _push_rows(self, proof_stream, indices, values, paths, width):
        """_open_rows for one member of a row-committed batch, over its slice of RowForest.query_raw's answer (values: uint8 array of
        [k][width] residues, paths: uint8 array [k][64 * depth]): the same pushes -- a description where the stream takes
        descriptions (the columns were never Python objects: detached holders name them), else a list of FieldElements and a list of
        digests per position"""
        field = self.field
        lazy = _po.lazy_objects(proof_stream)
        if lazy is not None:
            lazy.add(_po.RowOpenings([_po.DetachedEntries(field) for _ in range(width)], indices, values, paths))
            return
        k = len(indices)
        ints = _sc.unpack(values.tobytes(), k * width)
        digests = _sc._path_lists(memoryview(paths.tobytes()), 0, paths.shape[1] // 64, k)
        for j in range(k):
            proof_stream.push([FieldElement(v, field) for v in ints[j * width:(j + 1) * width]])
            proof_stream.push(digests[j])

    @staticmethod
    def _push_openings(entries, paths, proof_stream):
        if type(proof_stream) is ProofStream:            # push == objects.append: one list extension for the whole codeword
            proof_stream.objects.extend(x for pair in zip(entries, paths) for x in pair)
            return
        for entry, path in zip(entries, paths):
            proof_stream.push(entry)
            proof_stream.push(path)

    # -- verifier (fast_stark.py:180-286) -----------------------------------------------------------
    def verify(self, proof, transition_constraints, boundary, transition_zerofier_root, proof_stream=None):
        return self._walk(proof, transition_constraints, boundary, transition_zerofier_root, proof_stream, HostChecks(), None)

    def verify_batch(self, proofs, transition_constraints, boundaries, transition_zerofier_root, proof_streams=None):
        """[self.verify(proofs[i], transition_constraints, boundaries[i], transition_zerofier_root, proof_streams[i]) for i ...] with
        every Merkle path and FRI colinearity test of the whole batch checked in one device call per kind (csrc/merkle_verify.cuh).
        The walk over each proof is `verify`'s (_walk); the checks that are cheap on the host (the last codeword, its degree) run in
        it, the rest become rows -- the combination at the opened points too (COMBINATION_ON_DEVICE; one more device call for the
        batch).  A proof on which `verify` raises is reported False."""
        if proof_streams is None:
            proof_streams = [None] * len(proofs)
        checks = BatchChecks(len(proofs))
        for owner, (proof, boundary, proof_stream) in enumerate(zip(proofs, boundaries, proof_streams)):
            try:
                if not self._walk(proof, transition_constraints, boundary, transition_zerofier_root, proof_stream, checks, owner):
                    checks.reject(owner)
            except Exception:
                checks.reject(owner)
        return checks.run()

    def _walk(self, proof, transition_constraints, boundary, transition_zerofier_root, proof_stream, checks, owner):
        """THE verifier: one walk over a proof whose checks go to `checks` (fri.HostChecks: decided at once, the first failure ends
        the walk; fri.BatchChecks: rows of proof `owner` for the batch's device calls, the walk goes on), as Fri._walk's do.  False:
        rejected on the way."""
        stream = (ProofStream() if proof_stream == None else proof_stream).deserialize(proof)
        registers = range(self.num_registers)
        trace_rows = 1 + max(cycle for cycle, _, _ in boundary) + self.num_randomizers

        # the commitments, and the combination weights they determine
        if self.row_commitments:
            row_root = stream.pull()                     # one tree over the rows of [boundary quotients ..., randomizer]
        else:
            quotient_roots = [stream.pull() for _ in registers]
            randomizer_root = stream.pull()
        weights = self.sample_weights(1 + 2 * len(transition_constraints) + 2 * self.num_registers, stream.verifier_fiat_shamir())

        # low-degree test of the combination; it reports the combination's values at the points it opened
        opened = []
        accepted = self.fri._walk(stream, opened, checks, owner)
        opened.sort(key=lambda index_value: index_value[0])
        if not accepted:
            return False

        # every committed codeword opened at those points and at their successors on the trace domain
        N, step = self.fri.domain_length, self.expansion_factor
        positions = sorted([i for i, _ in opened] + [(i + step) % N for i, _ in opened])
        if self.row_commitments:
            opened_rows = self._pull_row_openings(stream, row_root, positions, checks, owner)
            if opened_rows is None:
                return False
            quotient_leaves = [{position: row[s] for position, row in opened_rows.items()} for s in registers]
            randomizer = {position: row[-1] for position, row in opened_rows.items()}
        else:
            quotient_leaves = []
            for root in quotient_roots + [randomizer_root]:
                quotient_leaves.append(self._pull_openings(stream, root, positions, checks, owner))
                if quotient_leaves[-1] is None:
                    return False
            randomizer = quotient_leaves.pop()
        zerofier_values = self._pull_openings(stream, transition_zerofier_root, positions, checks, owner)
        if zerofier_values is None:
            return False

        # the combination recomputed from the openings must agree with FRI's view of it at every queried point
        zerofiers, interpolants = self.boundary_zerofiers(boundary), self.boundary_interpolants(boundary)
        max_degree = self.max_degree(transition_constraints)
        transition_shifts = [max_degree - bound for bound in self.transition_quotient_degree_bounds(transition_constraints)]
        boundary_shifts = [max_degree - bound for bound in self.boundary_quotient_degree_bounds(trace_rows, boundary)]
        constraint_at = [constraint.evaluator() for constraint in transition_constraints]      # term lists extracted once, not per point

        def trace_row(index, x):
            # undo the boundary quotient: trace = quotient * zerofier + interpolant
            return [quotient_leaves[s][index] * zerofiers[s].evaluate(x) + interpolants[s].evaluate(x) for s in registers]

        def holds(index, claimed):
            successor = (index + step) % N
            x = self.generator * (self.omega ^ index)
            point = [x] + trace_row(index, x) + trace_row(successor, self.generator * (self.omega ^ successor))
            weight = iter(weights)
            total = randomizer[index] * next(weight)
            for evaluate, shift in zip(constraint_at, transition_shifts):
                quotient = evaluate(point) / zerofier_values[index]
                total = total + quotient * next(weight) + quotient * (x ^ shift) * next(weight)
            for s, shift in zip(registers, boundary_shifts):
                quotient = quotient_leaves[s][index]
                total = total + quotient * next(weight) + quotient * (x ^ shift) * next(weight)
            return bool(total == claimed)

        # in a batch the opened points become rows of one device call for the whole batch (csrc/combination.cuh), and `holds` decides
        # what the rows cannot hold or the device leaves undecided; without a group of rows -- host checks, or a batch whose
        # combination stays on the host -- `holds` decides every point here, in order, and the first that fails ends the walk
        group = self._combination_group(checks, transition_constraints, transition_shifts, boundary_shifts) if FastStark.COMBINATION_ON_DEVICE else None
        if group is None:
            return all(holds(index, claimed) for index, claimed in opened)
        member = group.member(weights, zerofiers, interpolants)
        for index, claimed in opened:
            successor = (index + step) % N
            checks.combination(owner, group, member, index, claimed, randomizer[index], zerofier_values[index], [quotient_leaves[s][index] for s in registers],
                               [quotient_leaves[s][successor] for s in registers], lambda index=index, claimed=claimed: holds(index, claimed))
        return True

    # The combination at the opened points of verify_batch (fast_stark.py:236-284 per point and proof) as rows of ONE device call for
    # the whole batch: the trace rows rebuilt from the boundary quotients, the AIR under the prover's Horner plan (csrc/mpoly_plan.h),
    # the transition quotients, the shifts, the weighted sum (csrc/combination.cuh).  False: the host loop, as before.
    COMBINATION_ON_DEVICE = True
    # Batches of fewer opened points than this keep the host loop (the three launches and the wait have a price).  Unmeasured so far:
    # 0 until tools/verify_timing.py has found a crossover.
    COMBINATION_DEVICE_MIN_ROWS = 0

    def _combination_tables(self, transition_constraints):
        """the constraints as sc_stark_combination_batch takes them (MPolynomial.pack_terms over 1 + 2 registers variables), None when
        one has no dictionary, a coefficient that is not a residue of the main field, an exponent above 255 or too many variables"""
        nvars = 1 + 2 * self.num_registers
        try:
            term_lists = []
            for constraint in transition_constraints:
                dictionary = getattr(constraint, "dictionary", None)
                if type(dictionary) is not dict or nvars > 255:
                    return None
                for v in dictionary.values():
                    if not (type(v) is FieldElement and type(v.value) is int and 0 <= v.value < Field.P_MAIN and v.field.p == Field.P_MAIN):
                        return None
                plan = constraint.value_domain_terms([1] * nvars)
                if plan is NotImplemented:
                    return None
                term_lists.append(plan[1])
            return MPolynomial.pack_terms(term_lists)
        except Exception:
            return None

    def _combination_group(self, checks, transition_constraints, transition_shifts, boundary_shifts):
        """the rows of this AIR on this domain in `checks` (made when the batch's first proof gets here), None when the check cannot
        be a device call at all: another field, constraints or shifts the format does not hold"""
        if self.field.p != Field.P_MAIN:
            return None
        key = ("stark", id(self), id(transition_constraints), tuple(transition_shifts), tuple(boundary_shifts))

        def make():
            tables = self._combination_tables(transition_constraints)
            N = self.fri.domain_length
            fits = (tables is not None and all(type(k) is int and 0 <= k < (1 << 64) for k in list(transition_shifts) + list(boundary_shifts))
                    and N >= 1 and N & (N - 1) == 0 and all(type(e.value) is int and 0 <= e.value < (1 << 128) for e in (self.generator, self.omega)))
            if not fits:
                return False
            return CombinationRows(self.num_registers, tables, self.generator.value, self.omega.value, N, self.expansion_factor, transition_shifts, boundary_shifts,
                                   FastStark.COMBINATION_DEVICE_MIN_ROWS, keep=transition_constraints)
        return checks.combination_group(key, make) or None

    def _pull_row_openings(self, stream, root, positions, checks, owner):
        """{position: row} from the (row, authentication path) pairs of a row commitment, in the order of `positions`; None as soon as
        a row is not a list of num_registers + 1 elements of this field with values below p, a path is not log2 N digests of 64
        bytes, the root is not a byte string, or `checks` says that the path does not lead from the row's leaf (Merkle.row_leaf,
        computed here) to `root`"""
        p, width, depth = self.field.p, self.num_registers + 1, self.fri.domain_length.bit_length() - 1
        rows = {}
        for position in positions:
            row, path = stream.pull(), stream.pull()
            if type(row) is not list or len(row) != width or not all(
                    type(v) is FieldElement and type(v.value) is int and 0 <= v.value < p and getattr(v.field, "p", None) == p for v in row):
                return None
            if type(path) is not list or len(path) != depth or not all(type(d) is bytes and len(d) == 64 for d in path):
                return None
            if type(root) is not bytes or not checks.merkle(owner, root, position, path, None, leaf_digest=Merkle.row_leaf(row)):
                return None
            rows[position] = row
        return rows

    @staticmethod
    def _pull_openings(stream, root, positions, checks, owner):
        """{position: leaf} from the (leaf, authentication path) pairs the prover pushed for one commitment, in the order of
        `positions`; None as soon as `checks` says that a path does not lead to `root`"""
        leaves = {}
        for position in positions:
            leaf, path = stream.pull(), stream.pull()
            if not checks.merkle(owner, root, position, path, leaf):
                return None
            leaves[position] = leaf
        return leaves

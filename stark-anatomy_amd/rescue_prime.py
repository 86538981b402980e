"""The Rescue-Prime hash of the tutorial's signature scheme (interface of reference code/rescue_prime.py:5-155).

`RescuePrime()` with `hash`, `trace`, `boundary_constraints`, `round_constants_polynomials` and `transition_constraints`, the
reference's call signatures and results.  The default parameters (state width m = 2, capacity 1, N = 27 rounds, alpha = 3) are the
reference's; `RescuePrime(m, capacity, rounds, security_level)` is the same construction at any width 2 .. 8 (rate = m - capacity;
the round count is the caller's).  The constants are DERIVED here the way the public Rescue-Prime specification defines them, not copied:

- round constants: SHAKE-256(b"Rescue-XLIX(p,m,capacity,security_level)") read as 2 m N chunks of ceil(128 / 8) + 1 = 17 bytes,
  each a little-endian integer mod p;
- MDS: with g the smallest element of order p - 1, the m x 2m matrix V[i][j] = g^(i j) in reduced row echelon form; MDS is the
  transpose of its right m x m half, MDSinv its inverse; alphainv = alpha^-1 mod (p - 1).

`hash` and `trace` are the host mirror of the reference (the same results for any caller).  The batched forms run on the MI355X
(csrc/rescue_prime.cuh through sc_rescue_prime_hash_dev / sc_rescue_prime_trace_dev): `hash_batch`, `hash_device`, `trace_device`
(a DeviceTrace FastStark.prove takes as it is) and `trace_batch_device`.  At any other width, or with more than one input element,
they go through the generic-width entries (sc_rescue_prime_permute_dev / _sponge_dev / _trace_states_dev), as do
`permutation_device`, `sponge_device`, `sponge_batch` and `compress`; `permutation` and `sponge` are their host model on plain
integers.  The sponge pads every message with a single 1, then zeros up to a multiple of the rate.

`transition_constraints` returns the reference's MPolynomial dictionaries (the prover's byte parity depends on them), cached per
omicron, as RescueConstraint objects whose `evaluator()` -- what FastStark.verify and verify_batch call at every opened point --
computes the constraint in its structured form instead of term by term.
"""
from hashlib import shake_256

from algebra import Field, FieldElement
from univariate import Polynomial
from multivariate import MPolynomial


def _order_is_full(g, p, prime_factors):
    return all(pow(g, (p - 1) // q, p) != 1 for q in prime_factors)


def _prime_factors(n):
    out, d = [], 2
    while d * d <= n:
        if n % d == 0:
            out.append(d)
            while n % d == 0:
                n //= d
        d += 1
    if n > 1:
        out.append(n)
    return out


def _row_echelon(matrix, p):
    """reduced row echelon form over F_p (rows swapped to find pivots)"""
    rows = [list(r) for r in matrix]
    pivot_row = 0
    for c in range(len(rows[0])):
        if pivot_row == len(rows):
            break
        pivot = next((i for i in range(pivot_row, len(rows)) if rows[i][c] % p), None)
        if pivot is None:
            continue
        rows[pivot_row], rows[pivot] = rows[pivot], rows[pivot_row]
        inv = pow(rows[pivot_row][c], -1, p)
        rows[pivot_row] = [v * inv % p for v in rows[pivot_row]]
        for i in range(len(rows)):
            if i != pivot_row and rows[i][c] % p:
                f = rows[i][c]
                rows[i] = [(a - f * b) % p for a, b in zip(rows[i], rows[pivot_row])]
        pivot_row += 1
    return rows


def _inverse_matrix(matrix, p):
    n = len(matrix)
    reduced = _row_echelon([list(row) + [int(i == j) for j in range(n)] for i, row in enumerate(matrix)], p)
    return [row[n:] for row in reduced]


def derive_parameters(p, m, capacity, security_level, rounds, alpha):
    """(MDS, MDSinv, round constants, alphainv) as Python ints, from the public specification (see the module's docstring)"""
    bytes_per_int = -(-security_level // 8) + 1
    count = 2 * m * rounds
    stream = shake_256(b"Rescue-XLIX(%d,%d,%d,%d)" % (p, m, capacity, security_level)).digest(count * bytes_per_int)
    round_constants = [int.from_bytes(stream[bytes_per_int * i:bytes_per_int * (i + 1)], "little") % p for i in range(count)]
    odd = p - 1                                   # p - 1 = 407 * 2^119 = 11 * 37 * 2^119: the odd part is small
    while odd % 2 == 0:
        odd //= 2
    factors = [2] + _prime_factors(odd)
    g = 2
    while not _order_is_full(g, p, factors):
        g += 1
    vandermonde = [[pow(g, i * j, p) for j in range(2 * m)] for i in range(m)]
    echelon = _row_echelon(vandermonde, p)
    mds = [[echelon[j][m + i] for j in range(m)] for i in range(m)]
    return mds, _inverse_matrix(mds, p), round_constants, pow(alpha, -1, p - 1)


class RescueConstraint(MPolynomial):
    """One Rescue-Prime transition constraint: the reference's MPolynomial (same dictionary), evaluated in its structured form
        sum_k MDS[i][k] s_k^3 + c1_i(x) - (sum_k MDSinv[i][k] (t_k - c2_k(x)))^3
    at point = [x, s_0 .. s_(m-1), t_0 .. t_(m-1)], the round-constant polynomials c1, c2 by Horner on residues -- the same value as
    MPolynomial.evaluate of the dictionary (272 terms per constraint at the tutorial's parameters)."""

    def __init__(self, dictionary, row, mds, mds_inv, first, second, alpha, p):
        MPolynomial.__init__(self, dictionary)
        self._shape = (row, mds, mds_inv, first, second, alpha, p)

    def evaluator(self):
        i, mds, mds_inv, first, second, alpha, p = self._shape
        m = len(mds)
        mds_row, inv_row, c1 = mds[i], mds_inv[i], first[i]

        def horner(coefficients, x):
            acc = 0
            for c in reversed(coefficients):
                acc = (acc * x + c) % p
            return acc

        def run(point):
            field = point[0].field
            x = point[0].value
            vals = [q.value for q in point]
            lhs = horner(c1, x)
            for k in range(m):
                lhs += mds_row[k] * pow(vals[1 + k], alpha, p)
            rhs = 0
            for k in range(m):
                rhs += inv_row[k] * (vals[1 + m + k] - horner(second[k], x))
            return FieldElement((lhs - pow(rhs % p, alpha, p)) % p, field)
        return run


class RescuePrime:
    def __init__(self, m=2, capacity=1, rounds=27, security_level=128):
        assert 2 <= m <= 8 and 1 <= capacity < m and 1 <= rounds <= 27, "state width 2 .. 8, capacity 1 .. m - 1, 1 .. 27 rounds"
        self.p = 407 * (1 << 119) + 1
        self.field = Field(self.p)
        self.m = m
        self.rate = m - capacity
        self.capacity = capacity
        self.N = rounds
        self.alpha = 3
        self.security_level = security_level
        mds, mds_inv, constants, self.alphainv = derive_parameters(self.p, self.m, self.capacity, self.security_level, self.N, self.alpha)
        fe = lambda v: FieldElement(v, self.field)
        self.MDS = [[fe(v) for v in row] for row in mds]
        self.MDSinv = [[fe(v) for v in row] for row in mds_inv]
        self.round_constants = [fe(v) for v in constants]
        self._mds, self._mds_inv, self._constants = mds, mds_inv, constants
        self._params = b"".join(v.to_bytes(16, "little") for v in [x for row in mds for x in row] + constants)
        self._constraints = {}

    # ---- the host mirror (code/rescue_prime.py:25-104), on residues
    def _residues(self, inputs, limit):
        """one element or a list of up to `limit` elements (FieldElements or ints) as residues"""
        values = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs]
        assert 1 <= len(values) <= limit, "1 .. %d elements expected" % limit
        return [int(getattr(v, "value", v)) % self.p for v in values]

    def _round(self, state, r):
        """round r on a state of residues: cube, mix, constants; inverse cube, mix, constants"""
        p, m, mds, rc = self.p, self.m, self._mds, self._constants
        for exponent, offset in ((self.alpha, 2 * r * m), (self.alphainv, 2 * r * m + m)):
            powered = [pow(s, exponent, p) for s in state]
            state = [(sum(mds[i][j] * powered[j] for j in range(m)) + rc[offset + i]) % p for i in range(m)]
        return state

    def _states(self, inputs):
        """the N + 1 states from the rate part `inputs` (one residue or up to `rate` of them; the other registers start at zero)"""
        values = self._residues(inputs, self.rate)
        state = values + [0] * (self.m - len(values))
        yield state
        for r in range(self.N):
            state = self._round(state, r)
            yield state

    def permutation(self, state):
        """the N rounds on a whole state of m plain integers"""
        state = self._residues(state, self.m)
        assert len(state) == self.m, "a state of m elements"
        for r in range(self.N):
            state = self._round(state, r)
        return state

    def pad(self, elements):
        """the message, a single 1, then zeros up to a multiple of the rate -- always at least the 1, so that messages of different
        lengths never share a padded form"""
        values = [int(getattr(v, "value", v)) % self.p for v in elements] + [1]
        return values + [0] * (-len(values) % self.rate)

    def sponge(self, elements, out_len=1):
        """the digest (out_len plain integers, 1 <= out_len <= rate) of a message of any length: padded, absorbed `rate` elements
        per permutation into a zero state, registers 0 .. out_len - 1 squeezed"""
        assert 1 <= out_len <= self.rate, "1 <= out_len <= rate"
        padded = self.pad(elements)
        state = [0] * self.m
        for b in range(0, len(padded), self.rate):
            block = padded[b:b + self.rate]
            state = self.permutation([(s + v) % self.p for s, v in zip(state, block)] + state[self.rate:])
        return state[:out_len]

    def hash(self, input_element):
        last = None
        for last in self._states(input_element):
            pass
        return FieldElement(last[0], self.field)

    def trace(self, input_element):
        return [[FieldElement(s, self.field) for s in state] for state in self._states(input_element)]

    def boundary_constraints(self, output_element):
        # at the start the capacity is zero; at the end the first rate element is the given output element.  (FastStark wants at
        # least one condition per register: at a rate above 1 the caller adds (0, s, input s) for the inputs that are public.)
        return [(0, s, self.field.zero()) for s in range(self.rate, self.m)] + [(self.N, 0, output_element)]

    def round_constants_polynomials(self, omicron):
        domain = [omicron ^ r for r in range(0, self.N)]
        first_step_constants, second_step_constants = [], []
        for offset, out in ((0, first_step_constants), (self.m, second_step_constants)):
            for i in range(self.m):
                values = [self.round_constants[2 * r * self.m + offset + i] for r in range(self.N)]
                out.append(MPolynomial.lift(Polynomial.interpolate_domain(domain, values), 0))
        return first_step_constants, second_step_constants

    def transition_constraints(self, omicron):
        key = (omicron.field.p, omicron.value)
        cached = self._constraints.get(key)
        if cached is None:
            cached = self._constraints[key] = self._transition_constraints(omicron)
        return list(cached)

    def _transition_constraints(self, omicron):
        # the reference's construction (code/rescue_prime.py:134-155), operation for operation: the dictionaries are the prover's input
        first_step_constants, second_step_constants = self.round_constants_polynomials(omicron)
        variables = MPolynomial.variables(1 + 2 * self.m, self.field)
        previous_state = variables[1:(1 + self.m)]
        next_state = variables[(1 + self.m):(1 + 2 * self.m)]
        # the univariate coefficients of the round-constant polynomials (variable 0 only), for the structured evaluator
        first = [_univariate(c, self.p) for c in first_step_constants]
        second = [_univariate(c, self.p) for c in second_step_constants]
        air = []
        for i in range(self.m):
            lhs = MPolynomial.constant(self.field.zero())
            for k in range(self.m):
                lhs = lhs + MPolynomial.constant(self.MDS[i][k]) * (previous_state[k] ^ self.alpha)
            lhs = lhs + first_step_constants[i]
            rhs = MPolynomial.constant(self.field.zero())
            for k in range(self.m):
                rhs = rhs + MPolynomial.constant(self.MDSinv[i][k]) * (next_state[k] - second_step_constants[k])
            rhs = rhs ^ self.alpha
            air.append(RescueConstraint((lhs - rhs).dictionary, i, self._mds, self._mds_inv, first, second, self.alpha, self.p))
        return air

    def randomizer_freedom(self, omicron, num_randomizers):
        # code/rescue_prime.py:269-273: the zerofier of {omicron^i, N <= i < N + num_randomizers}, lifted to variable 0
        domain = [omicron ^ i for i in range(self.N, self.N + num_randomizers)]
        return MPolynomial.lift(Polynomial.zerofier_domain(domain), 0)

    # ---- batched on the MI355X (sc_rescue_prime_hash_dev / sc_rescue_prime_trace_dev; any other width: the generic-width entries)
    def _launch(self, entry, vec, out):
        import starkcore as sc
        sc._check(getattr(sc.lib(), entry)(vec.ptr if vec.n else None, vec.n, self._params, self.N, out.ptr if out.n else None, None))
        return out

    def hash_device(self, vec):
        """DeviceVector of n inputs -> DeviceVector of their n hashes (enqueued on the library stream)"""
        import starkcore as sc
        if self.m != 2:                             # register 0 of the permuted states (input, 0 .. 0)
            out = self.permutation_device(self._initial_states(vec, vec.n), vec.n)
            return sc.DeviceVector.wrap(out.ptr, vec.n, out)
        return self._launch("sc_rescue_prime_hash_dev", vec, sc.DeviceVector(vec.n))

    def hash_batch(self, elements):
        """[self.hash(e) for e in elements], on the device"""
        import starkcore as sc
        elements = list(elements)
        if not elements:
            return []
        out = self.hash_device(sc.DeviceVector.from_bytes(sc.pack([e.value for e in elements])))
        return [FieldElement(v, self.field) for v in sc.unpack(out.to_bytes())]

    def permutation_device(self, matrix, n):
        """n states as a DeviceVector of m n elements, register s of state k at s n + k -> their permutations, laid out the same"""
        import starkcore as sc
        assert matrix.n == self.m * n, "m rows of n elements"
        out = sc.DeviceVector(self.m * n)
        sc._check(sc.lib().sc_rescue_prime_permute_dev(matrix.ptr if n else None, n, out.ptr if n else None, n, n, self.m, self._params, self.N, None))
        return out

    def sponge_device(self, matrix, n, blocks, out_len=1):
        """n padded messages of `blocks` blocks as a DeviceVector of blocks * rate * n elements, element j of message k at j n + k
        -> their digests as out_len * n elements, element j of digest k at j n + k"""
        import starkcore as sc
        assert matrix.n == blocks * self.rate * n, "blocks * rate rows of n elements"
        out = sc.DeviceVector(out_len * n)
        sc._check(sc.lib().sc_rescue_prime_sponge_dev(matrix.ptr if n else None, n, blocks, out.ptr if n else None, n, out_len, n, self.m, self.rate,
                                                      self._params, self.N, None))
        return out

    def sponge_batch(self, messages, out_len=1):
        """[self.sponge(msg, out_len) for msg in messages] for messages of one length, in one launch"""
        import starkcore as sc
        padded = [self.pad(msg) for msg in messages]
        if not padded:
            return []
        n, rows = len(padded), len(padded[0])
        assert all(len(msg) == rows for msg in padded), "messages of one length"
        assert 1 <= out_len <= self.rate, "1 <= out_len <= rate"
        matrix = sc.DeviceVector.from_bytes(sc.pack([msg[j] for j in range(rows) for msg in padded]))
        got = sc.unpack(self.sponge_device(matrix, n, rows // self.rate, out_len).to_bytes())
        return [[got[j * n + k] for j in range(out_len)] for k in range(n)]

    def compress(self, left, right):
        """two-to-one: [self.sponge([l, r]) for l, r in zip(left, right)] in one launch"""
        assert self.rate >= 2, "compressing two elements into one needs a rate of at least 2"
        left, right = list(left), list(right)
        assert len(left) == len(right), "as many left as right elements"
        return self.sponge_batch([[l, r] for l, r in zip(left, right)])

    def _initial_states(self, vec, n):
        """rows of n rate elements each (a DeviceVector of rows * n, 1 <= rows <= rate) -> the m n initial states: the other registers zero"""
        import starkcore as sc
        rows = vec.n // n if n else 1
        assert vec.n == rows * n and 1 <= rows <= self.rate, "1 .. rate rows of n elements"
        states = sc.DeviceVector.zeros(self.m * n)
        if n:
            sc._check(sc.lib().sc_memcpy_dev(states.ptr, vec.ptr, vec.n, None))
        return states

    def trace_batch_device(self, vec, n=None):
        """the traces of n inputs as one DeviceVector of m n (N + 1) elements: register s of input k's state t at
        (m k + s) (N + 1) + t -- one input's column is one run.  vec: the n inputs; with `n` given, 1 .. rate rows of n elements
        (element j of input k at j n + k) that fill registers 0 .. rows - 1"""
        import starkcore as sc
        if self.m == 2 and n is None:
            return self._launch("sc_rescue_prime_trace_dev", vec, sc.DeviceVector(2 * vec.n * (self.N + 1)))
        n = vec.n if n is None else n
        states = self._initial_states(vec, n)
        out = sc.DeviceVector(self.m * n * (self.N + 1))
        sc._check(sc.lib().sc_rescue_prime_trace_states_dev(states.ptr if n else None, n, n, self.m, self._params, self.N, out.ptr if n else None, None))
        return out

    def trace_device(self, input_element):
        """self.trace(input_element) as a DeviceTrace (m columns of N + 1 rows in HBM): what FastStark.prove takes as its trace.
        input_element: one element or a list of up to `rate` elements"""
        import starkcore as sc
        from fast_stark import DeviceTrace
        rows = self.N + 1
        values = self._residues(input_element, self.rate)
        vec = sc.DeviceVector.from_bytes(sc.pack(values))
        whole = self.trace_batch_device(vec) if len(values) == 1 else self.trace_batch_device(vec, 1)
        base = whole.ptr
        columns = [sc.DeviceVector.wrap(base + 16 * rows * s, rows, whole) for s in range(self.m)]
        return DeviceTrace(columns, self.field)


def _univariate(mp, p):
    """coefficients (low to high, ints) of an MPolynomial in variable 0 alone (MPolynomial.lift of a univariate polynomial)"""
    degree = max((k[0] for k in mp.dictionary), default=-1)
    out = [0] * (degree + 1)
    for k, v in mp.dictionary.items():
        assert not any(k[1:]), "a polynomial in variable 0 alone"
        out[k[0]] = (out[k[0]] + v.value) % p
    return out

"""NTT-based polynomial arithmetic -- host shim over the HIP kernels (libstarkcore.so).

Same callables, argument meaning, assertion messages and list-length conventions as the reference's
code/ntt.py (ntt :3, intt :20, fast_multiply :32, fast_zerofier :66, fast_evaluate :82,
fast_interpolate :102, fast_coset_evaluate :132, fast_coset_divide :137); the transforms, the coset
scaling, the Hadamard product / pointwise division and the truncations run on the MI355X.  fast_divide is
Polynomial.divide (code/univariate.py:80-97) -- division WITH remainder, by any divisor -- on the same transforms.

`list[FieldElement]` in -> new `list[FieldElement]` out (arguments are never mutated).  The *_device
variants take/return `DeviceCodeword` (data stays in HBM; no per-element marshalling) and are what
fri.py / bench.py use for large domains.
"""
import ctypes

from univariate import *
import starkcore as _sc
from starkcore import DeviceCodeword, DeviceVector

_ROOT_ORDER_MSG = "supplied root does not have supplied order"
_ROOT_PRIM_MSG = "supplied root is not primitive root of supplied order"


_FIELD_MSG = "the MI355X polynomial core implements the field p = 1 + 407 * 2^119 only"


def _require_main_field(field):
    """The kernels are hard-wired to p = 1 + 407*2^119 (the only field whose primitive_nth_root the reference supports,
    algebra.py:104-114).  There is no CPU fallback, so any other modulus is refused loudly instead of being mis-reduced."""
    assert(field.p == Field.P_MAIN), _FIELD_MSG


def _pack(elements):
    return _sc.pack(list(map(_sc._value_of, elements)))


def _unpack(raw, count, field):
    return [FieldElement(v, field) for v in _sc.unpack(raw, count)]


_verified_roots = set()       # (p, root, order) triples that already passed the two assertions below


def _check_root(primitive_root, root_order):
    key = (primitive_root.field.p, primitive_root.value, root_order)
    if key in _verified_roots:
        return
    assert(primitive_root ^ root_order == primitive_root.field.one()), _ROOT_ORDER_MSG
    assert(primitive_root ^ (root_order // 2) != primitive_root.field.one()), _ROOT_PRIM_MSG
    if len(_verified_roots) < 4096:
        _verified_roots.add(key)


def _transform(primitive_root, values, inverse):
    n = len(values)
    field = values[0].field
    _require_main_field(field)
    if isinstance(values, DeviceCodeword):
        out = DeviceVector(n)
        _sc._check(_sc.lib().sc_ntt_dev(values.vec.ptr, out.ptr, n, _sc.fe_bytes(primitive_root.value), inverse, None))
        return DeviceCodeword(out, field)
    out = ctypes.create_string_buffer(16 * n)
    _sc._check(_sc.lib().sc_ntt(_pack(values), out, n, _sc.fe_bytes(primitive_root.value), inverse))
    return _unpack(out.raw, n, field)


def ntt(primitive_root, values):
    assert(len(values) & (len(values) - 1) == 0), "cannot compute ntt of non-power-of-two sequence"
    if len(values) <= 1:
        return values
    field = values[0].field
    assert(primitive_root ^ len(values) == field.one()), "primitive root must be nth root of unity, where n is len(values)"
    assert(primitive_root ^ (len(values) // 2) != field.one()), "primitive root is not primitive nth root of unity, where n is len(values)"
    return _transform(primitive_root, values, 0)


def intt(primitive_root, values):
    assert(len(values) & (len(values) - 1) == 0), "cannot compute intt of non-power-of-two sequence"
    if len(values) == 1:
        return values
    field = values[0].field
    # the reference runs ntt(root^-1, .) and so inherits its root checks (ntt.py:27-29, :10-11)
    assert(primitive_root ^ len(values) == field.one()), "primitive root must be nth root of unity, where n is len(values)"
    assert(primitive_root ^ (len(values) // 2) != field.one()), "primitive root is not primitive nth root of unity, where n is len(values)"
    return _transform(primitive_root, values, 1)


def _transform_columns(primitive_root, columns, inverse):
    columns = list(columns)
    if not columns:
        return []
    n = len(columns[0])
    assert(all(len(c) == n for c in columns)), "the columns of one call have one length"
    assert(n & (n - 1) == 0), "cannot compute intt of non-power-of-two sequence" if inverse else "cannot compute ntt of non-power-of-two sequence"
    if n == 1 or (n == 0 and not inverse):
        return columns                                    # ntt / intt hand a sequence of this length back as it is
    field = columns[0][0].field
    assert(primitive_root ^ n == field.one()), "primitive root must be nth root of unity, where n is len(values)"
    assert(primitive_root ^ (n // 2) != field.one()), "primitive root is not primitive nth root of unity, where n is len(values)"
    _require_main_field(field)
    cols = len(columns)
    src = DeviceVector.from_bytes(b"".join(_pack(c) for c in columns))
    out = DeviceVector(cols * n)
    _sc._check(_sc.lib().sc_ntt_columns_dev(src.ptr, out.ptr, n, cols, _sc.fe_bytes(primitive_root.value), inverse, None))
    flat = _unpack(out.to_bytes(), cols * n, field)
    return [flat[c * n:(c + 1) * n] for c in range(cols)]


def ntt_columns(primitive_root, columns):
    """[ntt(primitive_root, c) for c in columns] for equal-length lists, as ONE call (sc_ntt_columns_dev): one upload, one set of
    launches for all columns, one download"""
    return _transform_columns(primitive_root, columns, 0)


def intt_columns(primitive_root, columns):
    """[intt(primitive_root, c) for c in columns], likewise"""
    return _transform_columns(primitive_root, columns, 1)


def _shrink_order(root, order, degree):
    # smallest power-of-two transform that still holds `degree+1` coefficients (ntt.py:47-49, :155-157)
    while degree < order // 2:
        root = root ^ 2
        order = order // 2
    return root, order


def fast_multiply(lhs, rhs, primitive_root, root_order):
    _check_root(primitive_root, root_order)
    if lhs.is_zero() or rhs.is_zero():
        return Polynomial([])
    field = lhs.coefficients[0].field
    dl, dr = lhs.degree(), rhs.degree()
    degree = dl + dr
    if degree < 8:
        return lhs * rhs
    _require_main_field(field)
    root, order = _shrink_order(primitive_root, root_order, degree)
    out = ctypes.create_string_buffer(16 * (degree + 1))
    _sc._check(_sc.lib().sc_poly_mul(_pack(lhs.coefficients[:dl + 1]), dl + 1, _pack(rhs.coefficients[:dr + 1]), dr + 1,
                                     _sc.fe_bytes(root.value), order, out, degree + 1))
    return Polynomial(_unpack(out.raw, degree + 1, field))


# Domains of at least this many points go to the device -- the level-batched subproduct tree (csrc/polytree.cuh), or, when the
# points are a geometric progression, a handful of convolutions (csrc/geoseq.cuh); smaller ones follow the reference's
# recursion below.  Zerofier, values and interpolant are unique, so all three give the same lists.
DEVICE_TREE_MIN_POINTS = 16

_tree_memo = {}           # points (as packed bytes) -> PolyTree; fast_interpolate / fast_evaluate revisit the same domains


def _device_tree(domain):
    _require_main_field(domain[0].field)
    key = _pack(domain)
    tree = _tree_memo.get(key)
    if tree is None:
        # a tree keeps ~1 KiB of HBM per point (all levels and their transforms): bound what the memo retains
        if len(_tree_memo) >= 8 or sum(t.k for t in _tree_memo.values()) + len(domain) > (1 << 22):
            for t in _tree_memo.values():
                t.free()
            _tree_memo.clear()
        # a geometric progression (the trace domain {omicron^i}, fast_stark.py:84-90) gets the progression tables, anything
        # else the subproduct tree: same zerofier, values and interpolant either way
        tree = _tree_memo[key] = _sc.domain_tables(key)
    return tree


# The reference recomputes the zerofier of every sub-domain at every node of fast_evaluate / fast_interpolate
# (ntt.py:92-93, :115-116); the polynomials are the same each time, so they are remembered per call tree.
_zerofier_memo = {}


def fast_zerofier(domain, primitive_root, root_order):
    _check_root(primitive_root, root_order)
    if len(domain) == 0:
        return Polynomial([])
    if len(domain) == 1:
        return Polynomial([-domain[0], primitive_root.field.one()])
    if len(domain) >= DEVICE_TREE_MIN_POINTS:
        return Polynomial(_unpack(_device_tree(domain).zerofier().to_bytes(), len(domain) + 1, primitive_root.field))
    key = (primitive_root.value, root_order, tuple(d.value for d in domain))
    hit = _zerofier_memo.get(key)
    if hit is not None:
        return hit
    half = len(domain) // 2
    result = fast_multiply(fast_zerofier(domain[:half], primitive_root, root_order),
                           fast_zerofier(domain[half:], primitive_root, root_order), primitive_root, root_order)
    if len(_zerofier_memo) >= 8192:
        _zerofier_memo.clear()
    _zerofier_memo[key] = result
    return result


def fast_evaluate(polynomial, domain, primitive_root, root_order):
    _check_root(primitive_root, root_order)
    if len(domain) == 0:
        return []
    if len(domain) == 1:
        return [polynomial.evaluate(domain[0])]
    if len(domain) >= DEVICE_TREE_MIN_POINTS:
        coeffs = DeviceVector.from_bytes(_pack(polynomial.coefficients))
        return _unpack(_device_tree(domain).evaluate(coeffs).to_bytes(), len(domain), primitive_root.field)
    half = len(domain) // 2
    lower, upper = domain[:half], domain[half:]
    lower_rem = polynomial % fast_zerofier(lower, primitive_root, root_order)
    upper_rem = polynomial % fast_zerofier(upper, primitive_root, root_order)
    return fast_evaluate(lower_rem, lower, primitive_root, root_order) + fast_evaluate(upper_rem, upper, primitive_root, root_order)


def fast_interpolate(domain, values, primitive_root, root_order):
    _check_root(primitive_root, root_order)
    assert(len(domain) == len(values)), "cannot interpolate over domain of different length than values list"
    if len(domain) == 0:
        return Polynomial([])
    if len(domain) == 1:
        return Polynomial([values[0]])
    if len(domain) >= DEVICE_TREE_MIN_POINTS:
        # a repeated point raises AssertionError("divide by zero") like the field division at ntt.py:124-125
        out = _device_tree(domain).interpolate(DeviceVector.from_bytes(_pack(values)))
        return Polynomial(_unpack(out.to_bytes(), len(domain), primitive_root.field))
    half = len(domain) // 2
    lower, upper = domain[:half], domain[half:]
    lower_zerofier = fast_zerofier(lower, primitive_root, root_order)
    upper_zerofier = fast_zerofier(upper, primitive_root, root_order)
    # each half is interpolated against values divided by the OTHER half's zerofier there (ntt.py:121-125)
    lower_offset = fast_evaluate(upper_zerofier, lower, primitive_root, root_order)
    upper_offset = fast_evaluate(lower_zerofier, upper, primitive_root, root_order)
    if not all(not v.is_zero() for v in lower_offset):
        print("left_offset:", " ".join(str(v) for v in lower_offset))
    lower_targets = [n / d for (n, d) in zip(values[:half], lower_offset)]
    upper_targets = [n / d for (n, d) in zip(values[half:], upper_offset)]
    lower_interpolant = fast_interpolate(lower, lower_targets, primitive_root, root_order)
    upper_interpolant = fast_interpolate(upper, upper_targets, primitive_root, root_order)
    return lower_interpolant * upper_zerofier + upper_interpolant * lower_zerofier


class DeviceDomain:
    """A list of evaluation points resident in HBM together with its subproduct tree (built once): the device-resident form
    of the `domain` argument of fast_zerofier / fast_evaluate / fast_interpolate for domains too large to marshal per call."""

    def __init__(self, points, field=None):
        """points: DeviceCodeword, DeviceVector (give `field`) or list[FieldElement]"""
        if isinstance(points, DeviceCodeword):
            vec, field = points.vec, points.field
        elif isinstance(points, DeviceVector):
            vec = points
        else:
            vec, field = DeviceVector.from_bytes(_pack(points)), points[0].field
        assert(vec.n > 0), "empty domain"
        _require_main_field(field)
        self.field = field
        self.tree = _sc.domain_tables(vec)

    @classmethod
    def geometric(cls, first, ratio, count):
        """the domain first * ratio^i, i < count (FieldElements), without materialising or inspecting the points: the trace
        domain of fast_stark.py:84-90 is {omicron^i}.  Falls back to the general tree where the progression tables do not apply."""
        field = ratio.field
        _require_main_field(field)
        tables = _sc.GeoDomain.create(first.value, ratio.value, count) if count >= 2 else None
        if tables is None:
            ones = DeviceVector.from_bytes((first.value).to_bytes(16, "little") * count)
            points = DeviceVector(count)
            _sc._check(_sc.lib().sc_scale_dev(ones.ptr, points.ptr, count, _sc.fe_bytes(ratio.value), None))
            return cls(points, field)
        domain = cls.__new__(cls)
        domain.field, domain.tree = field, tables
        return domain

    def __len__(self):
        return self.tree.k

    def points_vector(self):
        """the points themselves as a DeviceVector: the tree's own copy, or -- a progression keeps none -- first * ratio^i made once"""
        points = getattr(self.tree, "points", None) or getattr(self, "_points", None)
        if points is None:
            n = len(self)
            firsts = DeviceVector.from_bytes(self.tree.first.to_bytes(16, "little") * n)
            points = self._points = DeviceVector(n)
            _sc._check(_sc.lib().sc_scale_dev(firsts.ptr, points.ptr, n, _sc.fe_bytes(self.tree.ratio), None))
        return points


class DevicePolynomial:
    """A coefficient list resident in HBM: what `Polynomial` is to the host path.  `len(p)` is the reference's LIST length
    (trailing zeros count, like `polynomial.coefficients`); `degree()` is Polynomial.degree (code/univariate.py:7-17), computed
    on the device once and cached.  Used by the callers that keep their polynomials on the device (fast_stark.py)."""

    def __init__(self, vec, field, length=None):
        self.vec, self.field = vec, field
        self.n = vec.n if length is None else int(length)
        self._degree = None

    @classmethod
    def from_polynomial(cls, polynomial, field=None):
        coeffs = polynomial.coefficients
        field = field if field is not None else coeffs[0].field
        _require_main_field(field)
        out = cls(DeviceVector.from_bytes(_pack(coeffs)) if coeffs else DeviceVector(1), field, len(coeffs))
        out._degree = polynomial.degree()                  # known on the host: no round trip to the device for it later
        return out

    @classmethod
    def rows_from_polynomials(cls, polynomials, field):
        """host Polynomials -> DevicePolynomials that are the rows of ONE zero-padded matrix (one upload): every row holds as many
        coefficients as the longest polynomial has up to its degree (at least one), and knows its degree"""
        _require_main_field(field)
        degrees = [p.degree() for p in polynomials]
        m = max(max(degrees) + 1, 1)
        matrix = DeviceVector.from_bytes(b"".join(_pack(p.coefficients[:d + 1]) + bytes(16 * (m - d - 1)) for p, d in zip(polynomials, degrees)))
        rows = []
        for c, d in enumerate(degrees):
            row = cls(DeviceVector.wrap(matrix.ptr + 16 * m * c, m, matrix), field, m)
            row._degree = d
            rows.append(row)
        return rows

    @classmethod
    def from_codeword(cls, codeword):
        return cls(codeword.vec, codeword.field)

    def __len__(self):
        return self.n

    def to_polynomial(self):
        return Polynomial(_unpack(self.vec.to_bytes(0, self.n), self.n, self.field))

    def degree(self):
        if self._degree is None:
            deg = ctypes.c_int64(-1)
            _sc._check(_sc.lib().sc_vec_degree_dev(self.vec.ptr, self.n, ctypes.byref(deg), None))
            self._degree = int(deg.value)
        return self._degree

    @staticmethod
    def degrees(polynomials):
        """[p.degree() for p in polynomials], with ONE device call and one host wait (sc_vec_degree_columns_dev) for the members
        that do not know their degree yet when those are equally spaced rows of one matrix -- the trace polynomials of a wide
        trace; anything else is asked one by one"""
        unknown = [p for p in polynomials if p._degree is None and type(p) is DevicePolynomial]
        if len(unknown) >= 2 and unknown[0].n > 0 and all(p.n == unknown[0].n for p in unknown):
            n, places = unknown[0].n, [p.vec.ptr for p in unknown]
            pitch = places[1] - places[0]
            if pitch >= 16 * n and pitch % 16 == 0 and all(b - a == pitch for a, b in zip(places, places[1:])):
                found = (ctypes.c_int64 * len(unknown))()
                _sc._check(_sc.lib().sc_vec_degree_columns_dev(places[0], n, pitch // 16, len(unknown), found, None))
                for p, degree in zip(unknown, found):
                    p._degree = int(degree)
        return [p.degree() for p in polynomials]

    def is_zero(self):
        return self.degree() == -1

    def copy(self, length=None):
        length = self.n if length is None else length
        out = DeviceVector.zeros(max(length, 1))
        if min(length, self.n):
            out.axpy_shift(_View(self.vec, min(length, self.n)), 0, 1)
        return DevicePolynomial(out, self.field, length)

    def minus(self, polynomial):
        """self - polynomial for a (short) host Polynomial: list length max(len, len), like Polynomial.__sub__"""
        coeffs = polynomial.coefficients
        out = self.copy(max(self.n, len(coeffs)))
        if coeffs:
            out.vec.axpy_shift(DeviceVector.from_bytes(_pack(coeffs)), 0, self.field.p - 1)
        # a subtrahend of lower degree leaves the degree alone: asked of `self` (once, and remembered there -- the prover needs the
        # trace polynomials' degrees again for the transition quotients) instead of of the difference
        if polynomial.degree() < self.degree():
            out._degree = self._degree
        return out

    def scale(self, factor):
        """Polynomial.scale (code/univariate.py:153-154): coefficient i times factor^i"""
        out = DeviceVector(max(self.n, 1))
        if self.n:
            _sc._check(_sc.lib().sc_scale_dev(self.vec.ptr, out.ptr, self.n, _sc.fe_bytes(factor.value), None))
        scaled = DevicePolynomial(out, self.field, self.n)
        if factor.value % self.field.p != 0:
            scaled._degree = self._degree                  # coefficient i times factor^i: the same coefficients vanish (None stays None)
        return scaled

    def scaled_later(self, factor):
        """`scale(factor)` whose coefficients are only computed if somebody asks for them: a caller that evaluates the result on the
        coset g <factor> never does -- q(factor X) there is q's own codeword, one place on (fast_stark.py:105-113)"""
        return ScaledLater(self, factor)

    def divmod(self, divisor):
        """Polynomial.divide (code/univariate.py:80-97) on resident vectors (sc_poly_divmod_dev) -> (quotient, remainder) as
        DevicePolynomials of degree(self) - degree(divisor) + 1 and degree(divisor) coefficients; a numerator of lower degree:
        (the empty polynomial, self), like the reference.  A zero divisor raises fast_coset_divide's assertion."""
        dn, dd = DevicePolynomial.degrees([self, divisor])
        assert(dd != -1), "cannot divide by zero polynomial"
        if dn < dd:
            return DevicePolynomial(DeviceVector(1), self.field, 0), self
        _require_main_field(self.field)
        quo, rem = DeviceVector(dn - dd + 1), DeviceVector(max(dd, 1))
        _sc._check(_sc.lib().sc_poly_divmod_dev(self.vec.ptr, dn + 1, divisor.vec.ptr, dd + 1, quo.ptr, rem.ptr, None))
        quotient = DevicePolynomial(quo, self.field, dn - dd + 1)
        quotient._degree = dn - dd                         # the leading coefficient is self's over the divisor's: not zero
        return quotient, DevicePolynomial(rem, self.field, dd)

    def multiply(self, other):
        """Polynomial.__mul__ (code/univariate.py:48-57) on resident vectors (sc_poly_mul_dev): len(self) + len(other) - 1
        coefficients, trailing zeros included; the empty polynomial if either operand is.  Nothing is waited for; `other is self`
        (a square) is transformed once."""
        if self.n == 0 or other.n == 0:
            return DevicePolynomial(DeviceVector(1), self.field, 0)
        _require_main_field(self.field)
        out = DeviceVector(self.n + other.n - 1)
        _sc._check(_sc.lib().sc_poly_mul_dev(self.vec.ptr, self.n, other.vec.ptr, other.n, out.ptr, None))
        product = DevicePolynomial(out, self.field, self.n + other.n - 1)
        if self._degree is not None and other._degree is not None:
            product._degree = -1 if min(self._degree, other._degree) < 0 else self._degree + other._degree    # a field: no zero divisors
        return product

    def power(self, exponent):
        """Polynomial.__xor__ (code/univariate.py:140-150) on a resident vector (sc_poly_pow_dev): exponent * (len(self) - 1) + 1
        coefficients -- one forward transform, one pointwise power, one inverse transform instead of ~2 log2(exponent) products;
        the empty polynomial for the zero polynomial, like the reference (that asks for the degree: one host wait unless it is known)."""
        assert(exponent >= 0), "negative exponent"
        if self.is_zero():
            return DevicePolynomial(DeviceVector(1), self.field, 0)
        _require_main_field(self.field)
        length = exponent * (self.n - 1) + 1
        out = DeviceVector(length)
        _sc._check(_sc.lib().sc_poly_pow_dev(self.vec.ptr, self.n, exponent, out.ptr, None))
        result = DevicePolynomial(out, self.field, length)
        result._degree = exponent * self._degree
        return result

    def evaluate_points(self, points):
        """[self.evaluate(x) for x in points] (Polynomial.evaluate_domain, code/univariate.py:104-105) as ONE library call that only
        enqueues (sc_poly_eval_points_dev: len(self) * len(points) modular products, no tree, no transform) -> DeviceVector of
        len(points) values.  points: a list of FieldElements or a DeviceDomain; they may repeat."""
        _require_main_field(self.field)
        xs = points.points_vector() if isinstance(points, DeviceDomain) else DeviceVector.from_bytes(_pack(points))
        out = DeviceVector(max(xs.n, 1))
        _sc._check(_sc.lib().sc_poly_eval_points_dev(self.vec.ptr if self.n else None, self.n, self.n, 1, xs.ptr, xs.n, out.ptr, xs.n, None))
        return out if xs.n else DeviceVector(0)

    def evaluate(self, point):
        """Polynomial.evaluate (code/univariate.py:99-102) of a polynomial that stays in HBM -> FieldElement: one call of the
        evaluation kernel and one 16-byte read (a resident quotient at one out-of-domain point; nothing else is downloaded)"""
        return FieldElement(_sc.unpack(self.evaluate_points([point]).to_bytes(0, 1), 1)[0], point.field)

    def coset_evaluate(self, offset, generator, order):
        """fast_coset_evaluate (code/ntt.py:132-135) -> DeviceCodeword"""
        out = DeviceVector(order)
        # (enqueued, not waited for: whatever reads the codeword next runs on the same stream, and vectors freed meanwhile are parked
        # behind an event -- sc_vec_free never hands memory back while a stream may still use it)
        _sc._check(_sc.lib().sc_coset_evaluate_dev(self.vec.ptr, self.n, _sc.fe_bytes(offset.value), _sc.fe_bytes(generator.value), order, out.ptr, None))
        return DeviceCodeword(out, self.field)


class ScaledLater(DevicePolynomial):
    """source.scale(factor), made when `vec` is first read; `scaled_from` = (source, factor) for whoever can do without"""

    def __init__(self, source, factor):
        self.field, self.n = source.field, source.n
        self.scaled_from = (source, factor)
        self._made = None
        self._degree = source._degree if factor.value % source.field.p != 0 else None

    @property
    def vec(self):
        if self._made is None:
            source, factor = self.scaled_from
            self._made = DevicePolynomial.scale(source, factor)
            if self._degree is None:
                self._degree = self._made._degree
        return self._made.vec

    @vec.setter
    def vec(self, value):
        # (DevicePolynomial.__init__ is deliberately not run: there is no vector until somebody reads it)
        raise AttributeError("ScaledLater.vec is derived from scaled_from; wrap a new vector in a DevicePolynomial instead")

    def degree(self):
        if self._degree is None and self.scaled_from[1].value % self.field.p != 0:
            self._degree = self.scaled_from[0].degree()      # the same coefficients vanish
        return DevicePolynomial.degree(self)


class _View:
    """the first n elements of a DeviceVector (for axpy_shift sources)"""

    def __init__(self, vec, n):
        self.ptr, self.n = vec.ptr, n


def coset_divide_device(lhs, rhs, offset, primitive_root, root_order, exact=False, later=None):
    """fast_coset_divide (code/ntt.py:137-176) on DevicePolynomials: lhs.degree() - rhs.degree() + 1 coefficients, in HBM.
    exact=True additionally asserts what Polynomial.__truediv__ asserts (a zero remainder), decided on the device.
    later (a list, with exact=True): the division is only enqueued and a check is appended to the list -- a callable that waits for
    the device's verdict and raises what this call would have raised ("divide by zero", a non-zero remainder); the caller runs its
    checks where it has to wait anyway.  The quotient's degree is what an exact division leaves, which the check confirms."""
    _check_root(primitive_root, root_order)
    assert(not rhs.is_zero()), "cannot divide by zero polynomial"
    field = lhs.field
    if lhs.is_zero():
        return DevicePolynomial(DeviceVector(1), field, 0)
    dl, dr = lhs.degree(), rhs.degree()
    assert(dr <= dl), "cannot divide by polynomial of larger degree"
    root, order = _shrink_order(primitive_root, root_order, max(dl, dr))
    n_out = dl - dr + 1
    out = DeviceVector(n_out)
    if exact and later is not None:
        handle = ctypes.c_void_p()
        rc = _sc.lib().sc_coset_divide_later_dev(lhs.vec.ptr, dl + 1, rhs.vec.ptr, dr + 1, _sc.fe_bytes(offset.value), _sc.fe_bytes(root.value), order,
                                                 out.ptr, n_out, ctypes.byref(handle), None)
        if rc != _sc.SC_ERR_UNSUPPORTED:
            _sc._check(rc)
            check = _sc.Later(handle)

            def verdict():
                zero_divisor, remainder = check.wait()
                assert(not zero_divisor), "divide by zero"
                assert(not remainder), "cannot perform polynomial division because remainder is not zero"
            later.append(verdict)
            quotient = DevicePolynomial(out, field, n_out)
            quotient._degree = dl - dr
            return quotient
    flag = ctypes.c_int(0)
    _sc._check(_sc.lib().sc_coset_divide_dev(lhs.vec.ptr, dl + 1, rhs.vec.ptr, dr + 1, _sc.fe_bytes(offset.value), _sc.fe_bytes(root.value), order,
                                             out.ptr, n_out, ctypes.byref(flag) if exact else None, None))
    quotient = DevicePolynomial(out, field, n_out)
    if exact:
        assert(flag.value == 1), "cannot perform polynomial division because remainder is not zero"
        quotient._degree = dl - dr                         # an exact quotient's leading coefficient is lhs's over rhs's: not zero
    return quotient


def _divide_lengths(numerator, denominator, dn, dd):
    """list lengths of Polynomial.divide's results for dn >= dd >= 0: the quotient's, and the one the reference's running remainder
    ends with (it grows to the subtractee's list length when the denominator list carries trailing zeros)"""
    return dn - dd + 1, max(len(numerator.coefficients), dn - dd + len(denominator.coefficients))


def fast_divide(numerator, denominator):
    """Polynomial.divide (code/univariate.py:80-97) on the GPU (sc_poly_divmod): the same (quotient, remainder) -- values and list
    lengths -- None for a zero denominator, (Polynomial([]), numerator) for a numerator of lower degree.  Any divisor: no coset,
    no transform order, a remainder.  Numerators of degree < 8 are left to the long division."""
    dd = denominator.degree()
    if dd == -1:
        return None
    dn = numerator.degree()
    if dn < dd:
        return (Polynomial([]), numerator)
    if dn < 8:
        return numerator._schoolbook_divide(denominator)
    field = denominator.coefficients[0].field
    _require_main_field(field)
    n_quo, n_rem = _divide_lengths(numerator, denominator, dn, dd)
    quo, rem = ctypes.create_string_buffer(16 * n_quo), ctypes.create_string_buffer(16 * max(dd, 1))
    _sc._check(_sc.lib().sc_poly_divmod(_pack(numerator.coefficients[:dn + 1]), dn + 1, _pack(denominator.coefficients[:dd + 1]), dd + 1, quo, rem))
    return Polynomial(_unpack(quo.raw, n_quo, field)), Polynomial(_unpack(rem.raw, dd, field) + [field.zero()] * (n_rem - dd))


def fast_divide_columns(numerators, denominator):
    """[fast_divide(n, denominator) for n in numerators]: one upload, ONE division of all columns by the one divisor
    (sc_poly_divmod_columns_dev: its series is inverted once), one download.  Numerators of lower degree than the longest get their
    quotient's zero top coefficients stripped again; those below the divisor's degree (and a zero divisor, a short longest
    numerator) are answered on the host as fast_divide answers them."""
    numerators = list(numerators)
    dd = denominator.degree()
    dns = [n.degree() for n in numerators]
    batch = [c for c, dn in enumerate(dns) if dn >= dd]
    if dd == -1 or not batch or max(dns) < 8:
        return [fast_divide(n, denominator) for n in numerators]
    field = denominator.coefficients[0].field
    _require_main_field(field)
    na, nb = max(dns) + 1, dd + 1
    m, ld_r = na - nb + 1, max(dd, 1)
    cols = len(batch)
    src = DeviceVector.from_bytes(b"".join(_pack(numerators[c].coefficients[:dns[c] + 1]) + bytes(16 * (na - dns[c] - 1)) for c in batch))
    divisor = DeviceVector.from_bytes(_pack(denominator.coefficients[:nb]))
    quo, rem = DeviceVector(cols * m), DeviceVector(cols * ld_r)
    _sc._check(_sc.lib().sc_poly_divmod_columns_dev(src.ptr, na, na, cols, divisor.ptr, nb, quo.ptr, m, rem.ptr, ld_r, None))
    quos = _unpack(quo.to_bytes(), cols * m, field)
    rems = _unpack(rem.to_bytes(), cols * ld_r, field) if dd else []
    out = [(Polynomial([]), n) for n in numerators]
    for k, c in enumerate(batch):
        n_quo, n_rem = _divide_lengths(numerators[c], denominator, dns[c], dd)
        out[c] = (Polynomial(quos[k * m:k * m + n_quo]), Polynomial(rems[k * ld_r:k * ld_r + dd] + [field.zero()] * (n_rem - dd)))
    return out


# divide_columns_device hands fewer columns than this to DevicePolynomial.divmod one by one (tools/divide_timing.py)
DIVIDE_COLUMNS_MIN = 2


def divide_columns_device(numerators, divisor, quotients=True, remainders=True):
    """[n.divmod(divisor) for n in numerators] for DevicePolynomials and ONE divisor as one library call
    (sc_poly_divmod_columns_dev) -> (quotients, remainders): lists of DevicePolynomials that are rows of one matrix each, or None
    for the list not asked for (quotients=False / remainders=False; without remainders the product q * b is never formed).  Every
    column is divided as a numerator of the LONGEST numerator's degree (shorter ones are zero-padded into the matrix, unless the
    numerators already are equally spaced rows of one), so every quotient has the same number of coefficients -- zero on top for a
    shorter numerator, one zero coefficient if no numerator reaches the divisor's degree -- and every remainder deg(divisor)."""
    numerators = list(numerators)
    assert(quotients or remainders), "neither quotients nor remainders asked for"
    assert(not divisor.is_zero()), "cannot divide by zero polynomial"
    if not numerators:
        return ([] if quotients else None), ([] if remainders else None)
    field = divisor.field
    _require_main_field(field)
    dd = divisor.degree()
    dns = DevicePolynomial.degrees(numerators)
    nb = dd + 1
    na = max(max(dns) + 1, nb)
    m, cols = na - nb + 1, len(numerators)
    if cols < DIVIDE_COLUMNS_MIN and min(dns) >= dd:
        pairs = [n.divmod(divisor) for n in numerators]
        return ([q for q, _ in pairs] if quotients else None), ([r for _, r in pairs] if remainders else None)
    holder, ld_a = _as_matrix(numerators, na)
    ld_r = max(dd, 1)
    quo = DeviceVector(cols * m) if quotients else None
    rem = DeviceVector(cols * ld_r) if remainders else None
    _sc._check(_sc.lib().sc_poly_divmod_columns_dev(holder.ptr, na, ld_a, cols, divisor.vec.ptr, nb, quo.ptr if quotients else None, m,
                                                    rem.ptr if remainders else None, ld_r, None))
    rows = lambda matrix, ld, n: [DevicePolynomial(DeviceVector.wrap(matrix.ptr + 16 * ld * c, max(n, 1), matrix), field, n) for c in range(cols)]
    quos = rows(quo, m, m) if quotients else None
    if quotients:
        for q, dn in zip(quos, dns):
            q._degree = dn - dd if dn >= dd else -1        # the leading coefficient is the numerator's over the divisor's: not zero
    return quos, (rows(rem, ld_r, dd) if remainders else None)


def _pitch_of(vectors, n):
    """element pitch of DeviceVectors that are equally spaced rows (of at least n elements) of one matrix, else None; one vector: n"""
    places = [v.ptr for v in vectors]
    if len(places) == 1:
        return n
    pitch = places[1] - places[0]
    if pitch >= 16 * n and pitch % 16 == 0 and all(b - a == pitch for a, b in zip(places, places[1:])):
        return pitch // 16
    return None


def _as_matrix(polynomials, n):
    """(holder of the device pointer, pitch) of a matrix whose row c holds the first n coefficients of polynomials[c] (zero beyond its
    length): the polynomials' own memory when they are equally spaced rows of one matrix already and all hold n coefficients,
    else a zero-padded copy, as fast_interpolate_columns_device copies its columns"""
    if all(len(p) >= n for p in polynomials):
        pitch = _pitch_of([p.vec for p in polynomials], n)
        if pitch is not None:
            return polynomials[0].vec, pitch
    full = all(len(p) >= n for p in polynomials)
    matrix = DeviceVector(len(polynomials) * n) if full else DeviceVector.zeros(len(polynomials) * n)
    for c, p in enumerate(polynomials):
        if min(len(p), n):
            _sc._check(_sc.lib().sc_memcpy_dev(matrix.ptr + 16 * n * c, p.vec.ptr, min(len(p), n), None))
    return matrix, n


# multiply_columns_device hands fewer columns than this to DevicePolynomial.multiply one by one.  Measured (tools/multiply_timing.py,
# profiles/poly_multiply/): two resident columns in one call are x1.6 faster than two calls at 2^10, 2^12 and 2^16
# coefficients, shared multiplicand or one per column, and the gain grows with the number of columns -- so only a single column loops.
# fast_multiply_columns uses the same limit: on host lists both sides pack and unpack every coefficient in Python, which leaves
# x1.15 to x2.7 (never slower; below the x1.5 margin for operands of 1024 coefficients at every number of columns).
MULTIPLY_COLUMNS_MIN = 2


def multiply_columns_device(lhs_list, rhs):
    """[l.multiply(r_c) for l in lhs_list], r_c = rhs (one DevicePolynomial for every column, transformed once) or rhs[c], as ONE
    library call (sc_poly_mul_columns_dev) -> DevicePolynomials that are rows of one matrix.  Every column is multiplied as a
    polynomial of the LONGEST operand's length on either side (shorter ones are zero-padded into a matrix, unless the operands already
    are equally spaced rows of one), so every product has max(len lhs) + max(len rhs) - 1 coefficients, zero on top for a shorter
    operand; no coefficients at all if one side has none."""
    lhs_list = list(lhs_list)
    shared = isinstance(rhs, DevicePolynomial)
    rhs_list = [rhs] if shared else list(rhs)
    assert(shared or len(rhs_list) == len(lhs_list)), "one multiplicand, or one per column"
    if not lhs_list:
        return []
    field = lhs_list[0].field
    na, nb, cols = max(len(p) for p in lhs_list), max(len(p) for p in rhs_list), len(lhs_list)
    if na == 0 or nb == 0:
        return [DevicePolynomial(DeviceVector(1), field, 0) for _ in lhs_list]
    _require_main_field(field)
    if cols < MULTIPLY_COLUMNS_MIN and all(len(p) == na for p in lhs_list) and all(len(p) == nb for p in rhs_list):
        return [l.multiply(rhs if shared else rhs_list[c]) for c, l in enumerate(lhs_list)]
    n = na + nb - 1
    holder_a, ld_a = _as_matrix(lhs_list, na)
    holder_b, ld_b = (rhs.vec, 0) if shared else _as_matrix(rhs_list, nb)
    out = DeviceVector(cols * n)
    _sc._check(_sc.lib().sc_poly_mul_columns_dev(holder_a.ptr, na, ld_a, cols, holder_b.ptr, nb, ld_b, out.ptr, n, None))
    products = [DevicePolynomial(DeviceVector.wrap(out.ptr + 16 * n * c, n, out), field, n) for c in range(cols)]
    for c, (l, product) in enumerate(zip(lhs_list, products)):
        r = rhs if shared else rhs_list[c]
        if l._degree is not None and r._degree is not None:
            product._degree = -1 if min(l._degree, r._degree) < 0 else l._degree + r._degree
    return products


def _host_product_lengths(lhs, rhs):
    """list length of Polynomial.__mul__'s result: len + len - 1 (code/univariate.py:48-57), nothing if either list is empty"""
    return len(lhs.coefficients) + len(rhs.coefficients) - 1 if lhs.coefficients and rhs.coefficients else 0


def fast_multiply_columns(lhs_list, rhs):
    """[l * rhs for l in lhs_list] on host Polynomials -- the same values and list lengths -- as one upload, ONE library call
    (sc_poly_mul_columns_dev: the multiplicand is transformed once) and one download.  Zero operands, empty lists and products of
    degree below 8 throughout are answered on the host as fast_multiply answers them."""
    lhs_list = list(lhs_list)
    dr = rhs.degree()
    dls = [l.degree() for l in lhs_list]
    batch = [c for c, dl in enumerate(dls) if dl >= 0]
    if dr == -1 or len(batch) < MULTIPLY_COLUMNS_MIN or max(dls) + dr < 8:
        return [l * rhs for l in lhs_list]
    field = rhs.coefficients[0].field
    _require_main_field(field)
    na, nb, cols = max(dls) + 1, dr + 1, len(batch)
    n = na + nb - 1
    src = DeviceVector.from_bytes(b"".join(_pack(lhs_list[c].coefficients[:dls[c] + 1]) + bytes(16 * (na - dls[c] - 1)) for c in batch))
    multiplicand = DeviceVector.from_bytes(_pack(rhs.coefficients[:nb]))
    out = DeviceVector(cols * n)
    _sc._check(_sc.lib().sc_poly_mul_columns_dev(src.ptr, na, na, cols, multiplicand.ptr, nb, 0, out.ptr, n, None))
    flat = _unpack(out.to_bytes(), cols * n, field)
    # (a zero polynomial with a non-empty list: the schoolbook product's list of zeros)
    products = [Polynomial([field.zero()] * _host_product_lengths(l, rhs)) for l in lhs_list]
    for k, c in enumerate(batch):
        kept = dls[c] + dr + 1
        products[c] = Polynomial(flat[k * n:k * n + kept] + [field.zero()] * (_host_product_lengths(lhs_list[c], rhs) - kept))
    return products


def fast_power(polynomial, exponent):
    """Polynomial.__xor__ (code/univariate.py:140-150) on the GPU (sc_poly_pow_dev): the same values and the same list,
    exponent * (len - 1) + 1 long; the empty polynomial for the zero polynomial.  One forward transform, one pointwise power and one
    inverse transform instead of the binary method's ~2 log2(exponent) products.  Exponents below 2 and results of degree below 8
    are left to the binary method."""
    d = polynomial.degree()
    if d == -1 or exponent < 2 or d * exponent < 8:
        return polynomial._binary_power(exponent)
    field = polynomial.coefficients[0].field
    _require_main_field(field)
    kept, full = exponent * d + 1, exponent * (len(polynomial.coefficients) - 1) + 1
    base = DeviceVector.from_bytes(_pack(polynomial.coefficients[:d + 1]))
    out = DeviceVector(kept)
    _sc._check(_sc.lib().sc_poly_pow_dev(base.ptr, d + 1, exponent, out.ptr, None))
    return Polynomial(_unpack(out.to_bytes(), kept, field) + [field.zero()] * (full - kept))


def fast_product(polynomials):
    """the left-to-right product p_0 * p_1 * ... of host Polynomials -- the same values and the same list, sum(len - 1) + 1 long
    (empty if a member's list is) -- as one upload, ONE library call (sc_poly_product_dev: a balanced tree, every level one set
    of launches) and one download.  Shorter members are zero-padded into the matrix.  A zero member, a single member and
    products of degree below 8 are answered on the host."""
    polynomials = list(polynomials)
    assert(polynomials), "the product of no polynomials"
    degrees = [p.degree() for p in polynomials]
    if len(polynomials) == 1 or min(degrees) < 0 or sum(degrees) < 8:
        product = polynomials[0]
        for p in polynomials[1:]:
            product = product * p
        return product
    field = polynomials[0].coefficients[0].field
    _require_main_field(field)
    count, n = len(polynomials), max(degrees) + 1
    rows = DeviceVector.from_bytes(b"".join(_pack(p.coefficients[:d + 1]) + bytes(16 * (n - d - 1)) for p, d in zip(polynomials, degrees)))
    total, kept = count * (n - 1) + 1, sum(degrees) + 1
    out = DeviceVector(total)
    _sc._check(_sc.lib().sc_poly_product_dev(rows.ptr, n, n, count, out.ptr, None))
    full = sum(len(p.coefficients) - 1 for p in polynomials) + 1
    return Polynomial(_unpack(out.to_bytes(0, kept), kept, field) + [field.zero()] * (full - kept))


def _columns_verdict(handle):
    """the check of a columns-form division (sc_*_columns_later_dev): raises what the first failing check of the per-column loop raises"""
    check = _sc.Later(handle)

    def verdict():
        zero_divisor, remainder = check.wait()             # the words of the lowest failing column
        assert(not zero_divisor), "divide by zero"
        assert(not remainder), "cannot perform polynomial division because remainder is not zero"
    return verdict


def coset_divide_columns_device(lhs_list, rhs, offset, primitive_root, root_order, later=None):
    """[coset_divide_device(l, r_c, offset, primitive_root, root_order, exact=True, later=later) for l in lhs_list], r_c = rhs (one
    DevicePolynomial for every column) or rhs[c], as ONE library call (sc_coset_divide_columns_later_dev) with ONE verdict: appended to
    `later`, or waited for on the spot with later=None; it raises "divide by zero" or the non-zero remainder, whichever the lowest
    failing column met.  The quotients are views of one matrix.  The batched call serves numerators of one known degree, at least every
    divisor's, in the main field -- equally spaced rows of one matrix, or copied into one; anything else, and a library without a
    free slot for the verdict, goes column by column."""
    lhs_list = list(lhs_list)
    shared = isinstance(rhs, DevicePolynomial)
    divisors = [rhs] * len(lhs_list) if shared else list(rhs)
    assert(len(divisors) == len(lhs_list)), "one divisor, or one per column"
    one_by_one = lambda: [coset_divide_device(l, r, offset, primitive_root, root_order, exact=True, later=later) for l, r in zip(lhs_list, divisors)]
    if not lhs_list:
        return []
    _check_root(primitive_root, root_order)
    field = lhs_list[0].field
    dl = lhs_list[0]._degree
    if field.p != Field.P_MAIN or dl is None or dl < 0 or any(l._degree != dl for l in lhs_list):
        return one_by_one()
    drs = [r.degree() for r in ([rhs] if shared else divisors)]
    if min(drs) < 0 or max(drs) > dl:
        return one_by_one()                                # (raises what the reference raises)
    cols, na, nb = len(lhs_list), dl + 1, max(drs) + 1
    root, order = _shrink_order(primitive_root, root_order, dl)
    numerators, ld_a = _as_matrix(lhs_list, na)
    divisor_rows, ld_b = (rhs.vec, 0) if shared else _as_matrix(divisors, nb)
    n_out = [dl - dr + 1 for dr in (drs * cols if shared else drs)]
    ld_out = max(n_out)
    out = DeviceVector(cols * ld_out)
    handle = ctypes.c_void_p()
    rc = _sc.lib().sc_coset_divide_columns_later_dev(numerators.ptr, na, ld_a, divisor_rows.ptr, nb, ld_b, cols, _sc.fe_bytes(offset.value), _sc.fe_bytes(root.value),
                                                     order, out.ptr, (ctypes.c_uint64 * cols)(*n_out), ld_out, ctypes.byref(handle), None)
    if rc == _sc.SC_ERR_UNSUPPORTED:
        return one_by_one()
    _sc._check(rc)
    verdict = _columns_verdict(handle)
    if later is not None:
        later.append(verdict)
    else:
        verdict()
    quotients = []
    for c in range(cols):
        quotient = DevicePolynomial(DeviceVector.wrap(out.ptr + 16 * ld_out * c, n_out[c], out), field, n_out[c])
        quotient._degree = n_out[c] - 1                    # what an exact division leaves, which the verdict confirms
        quotients.append(quotient)
    return quotients


def fast_coset_divide_columns(lhs_list, rhs, offset, primitive_root, root_order):
    """[fast_coset_divide(l, r_c, offset, primitive_root, root_order) for l in lhs_list] on host Polynomials, r_c = rhs (one Polynomial)
    or rhs[c]: one upload, one columns-form division, one download.  Degenerate shapes (a zero numerator, degree < 8, numerators of
    different degrees) go column by column through fast_coset_divide."""
    lhs_list = list(lhs_list)
    shared = isinstance(rhs, Polynomial)
    divisors = [rhs] * len(lhs_list) if shared else list(rhs)
    assert(len(divisors) == len(lhs_list)), "one divisor, or one per column"
    one_by_one = lambda: [fast_coset_divide(l, r, offset, primitive_root, root_order) for l, r in zip(lhs_list, divisors)]
    if not lhs_list:
        return []
    _check_root(primitive_root, root_order)
    dls, drs = [l.degree() for l in lhs_list], [r.degree() for r in divisors]
    dl = dls[0]
    if dl < 8 or any(d != dl for d in dls) or min(drs) < 0 or max(drs) > dl or offset.field.p != Field.P_MAIN:
        return one_by_one()
    field = offset.field
    cols, na, nb = len(lhs_list), dl + 1, max(drs) + 1
    root, order = _shrink_order(primitive_root, root_order, dl)
    numerators = DeviceVector.from_bytes(b"".join(_pack(l.coefficients[:na]) for l in lhs_list))
    rows = [rhs] if shared else divisors
    divisor_rows = DeviceVector.from_bytes(b"".join(_pack(r.coefficients[:dr + 1]) + bytes(16 * (nb - dr - 1)) for r, dr in zip(rows, drs)))
    n_out = [dl - dr + 1 for dr in drs]
    ld_out = max(n_out)
    out = DeviceVector(cols * ld_out)
    handle = ctypes.c_void_p()
    rc = _sc.lib().sc_coset_divide_columns_later_dev(numerators.ptr, na, na, divisor_rows.ptr, nb, 0 if shared else nb, cols, _sc.fe_bytes(offset.value),
                                                     _sc.fe_bytes(root.value), order, out.ptr, (ctypes.c_uint64 * cols)(*n_out), ld_out, ctypes.byref(handle), None)
    if rc == _sc.SC_ERR_UNSUPPORTED:
        return one_by_one()
    _sc._check(rc)
    zero_divisor, _ = _sc.Later(handle).wait()             # (fast_coset_divide does not look at the remainder either: "clean division only")
    assert(not zero_divisor), "divide by zero"
    flat = _unpack(out.to_bytes(), cols * ld_out, field)
    return [Polynomial(flat[c * ld_out:c * ld_out + n_out[c]]) for c in range(cols)]


def combine_columns_device(terms, weights, width):
    """The nonlinear combination of code/fast_stark.py:130-145 for every column at once, in ONE pass (sc_combine_columns_dev).
    terms: [([DevicePolynomial per column], shift)]; shift None: the polynomials as they are (one weight), an int: as they are and
    shifted up by `shift` places (two weights, in that order).  weights: one list per column (FieldElements or ints), in the terms'
    order.  -> one DevicePolynomial of `width` coefficients per column, rows of one matrix: column c is what
    FastStark._combination_on_device builds from column c's terms and weights."""
    cols = len(weights)
    field = terms[0][0][0].field
    table, keep = [], []
    for polynomials, shift in terms:
        assert(len(polynomials) == cols), "one polynomial per column in every term"
        n = max(len(p) for p in polynomials)
        source, ld = _as_matrix(polynomials, n) if n else (None, 0)
        keep.append(source)
        for k in ([0] if shift is None else [0, shift]):
            assert(n + k <= width), "a shifted term does not fit the output"
            table.append(_sc.CombineTerm(source.ptr if n else None, ld, n, k))
    for row in weights:
        assert(len(row) == len(table)), "one weight per term (two for a shifted one)"
    out = DeviceVector(cols * width if cols * width else 1)
    packed = _sc.pack([getattr(w, "value", w) for row in weights for w in row])
    _sc._check(_sc.lib().sc_combine_columns_dev((_sc.CombineTerm * len(table))(*table), len(table), packed, cols, out.ptr, width, width, None))
    if cols == 1:
        return [DevicePolynomial(out, field, width)]
    return [DevicePolynomial(DeviceVector.wrap(out.ptr + 16 * width * c, width, out), field, width) for c in range(cols)]


def fast_zerofier_device(domain):
    """fast_zerofier (ntt.py:66-80) of a DeviceDomain -> DeviceCodeword of len(domain) + 1 coefficients"""
    return DeviceCodeword(domain.tree.zerofier(), domain.field)


def fast_evaluate_device(coefficients, domain):
    """fast_evaluate (ntt.py:82-100): coefficients (DeviceCodeword) at a DeviceDomain -> DeviceCodeword of values"""
    return DeviceCodeword(domain.tree.evaluate(coefficients.vec), domain.field)


def fast_interpolate_device(domain, values):
    """fast_interpolate (ntt.py:102-130): values (DeviceCodeword) on a DeviceDomain -> DeviceCodeword of len(domain) coefficients"""
    assert(len(domain) == len(values)), "cannot interpolate over domain of different length than values list"
    return DeviceCodeword(domain.tree.interpolate(values.vec), domain.field)


def _rows_of(matrix, count, n, field):
    """the rows of a [count][n] device matrix as DeviceCodewords that are views of it (the matrix lives as long as any of them)"""
    return [DeviceCodeword(DeviceVector.wrap(matrix.ptr + 16 * n * c, n, matrix), field) for c in range(count)]


def fast_evaluate_columns_device(coefficient_list, domain):
    """[fast_evaluate_device(c, domain) for c in coefficient_list] for DeviceCodewords of any lengths on a DeviceDomain of either
    kind: every step of the evaluation is issued once for all columns (sc_geodomain_evaluate_columns_dev on a progression,
    sc_polytree_evaluate_columns_dev through the resident tree otherwise) and the results are views of ONE value matrix [cols][n].
    The coefficients are first copied into one zero-padded matrix unless they already are equally spaced rows of one."""
    coefficient_list = list(coefficient_list)
    if not coefficient_list:
        return []
    n, cols = len(domain), len(coefficient_list)
    m = max(len(c) for c in coefficient_list)
    if m:
        holder, pitch = _as_matrix(coefficient_list, m)
        matrix = _View(holder, (cols - 1) * pitch + m)     # (`holder` keeps the owner alive for the call; frees are parked behind the stream)
    else:
        matrix, pitch = DeviceVector(1), 0
    return _rows_of(domain.tree.evaluate_columns(matrix, m, cols, pitch), cols, n, domain.field)


def fast_evaluate_columns(polynomials, domain, primitive_root, root_order):
    """[fast_evaluate(p, domain, primitive_root, root_order) for p in polynomials]: on a domain that goes to the device, one
    upload, one column evaluation (progression tables or subproduct tree), one download; below that the recursion per polynomial"""
    _check_root(primitive_root, root_order)
    polynomials = list(polynomials)
    n, cols = len(domain), len(polynomials)
    if not polynomials or n < DEVICE_TREE_MIN_POINTS:
        return [fast_evaluate(p, domain, primitive_root, root_order) for p in polynomials]
    tables = _device_tree(domain)
    m = max(len(p.coefficients) for p in polynomials)
    matrix = DeviceVector.from_bytes(b"".join(_pack(p.coefficients) + bytes(16 * (m - len(p.coefficients))) for p in polynomials)) if m else DeviceVector(1)
    flat = _unpack(tables.evaluate_columns(matrix, m, cols).to_bytes(), cols * n, primitive_root.field)
    return [flat[c * n:(c + 1) * n] for c in range(cols)]


def fast_interpolate_columns_device(domain, values):
    """[fast_interpolate_device(domain, v) for v in values] for DeviceCodewords of len(domain) values each.  Every step of the
    interpolation is issued once for all columns -- sc_geodomain_interpolate_columns_dev on a progression domain,
    sc_polytree_interpolate_columns_dev through the resident tree on any other -- and the results are views of ONE coefficient
    matrix [cols][n]; the columns are first copied into one matrix unless they already are the consecutive rows of one."""
    values = list(values)
    n = len(domain)
    for v in values:
        assert(n == len(v)), "cannot interpolate over domain of different length than values list"
    if not values:
        return []
    cols = len(values)
    first = values[0].vec.ptr
    if all(v.vec.ptr == first + 16 * n * c for c, v in enumerate(values)):
        matrix = _View(values[0].vec, cols * n)            # (`values` keeps the owner alive for the call; frees are parked behind the stream)
    else:
        matrix = DeviceVector(cols * n)
        for c, v in enumerate(values):
            _sc._check(_sc.lib().sc_memcpy_dev(matrix.ptr + 16 * n * c, v.vec.ptr, n, None))
    return _rows_of(domain.tree.interpolate_columns(matrix, cols), cols, n, domain.field)


def fast_interpolate_columns(domain, values_list, primitive_root, root_order):
    """[fast_interpolate(domain, v, primitive_root, root_order) for v in values_list]: on a domain that goes to the device
    (a progression or any other points), one upload, one column interpolation, one download; below that the recursion per column"""
    _check_root(primitive_root, root_order)
    values_list = list(values_list)
    for values in values_list:
        assert(len(domain) == len(values)), "cannot interpolate over domain of different length than values list"
    if not values_list:
        return []
    n, cols = len(domain), len(values_list)
    if n < DEVICE_TREE_MIN_POINTS:
        return [fast_interpolate(domain, values, primitive_root, root_order) for values in values_list]
    tables = _device_tree(domain)                          # (a repeated point raises AssertionError("divide by zero") as fast_interpolate does)
    matrix = DeviceVector.from_bytes(b"".join(_pack(values) for values in values_list))
    flat = _unpack(tables.interpolate_columns(matrix, cols).to_bytes(), cols * n, primitive_root.field)
    return [Polynomial(flat[c * n:(c + 1) * n]) for c in range(cols)]


def evaluate_points_device(polynomials, points):
    """[p.evaluate_points(points) for p in polynomials] for DevicePolynomials as ONE library call (sc_poly_eval_points_dev with
    one column per polynomial) -> DeviceVectors of len(points) values that are rows of one matrix.  Shorter polynomials count as
    zero-padded to the longest; equally spaced rows of one matrix are read where they lie (_as_matrix), anything else is copied
    into one.  points: a list of FieldElements or a DeviceDomain."""
    polynomials = list(polynomials)
    if not polynomials:
        return []
    _require_main_field(polynomials[0].field)
    xs = points.points_vector() if isinstance(points, DeviceDomain) else DeviceVector.from_bytes(_pack(points))
    k, cols, m = xs.n, len(polynomials), max(len(p) for p in polynomials)
    holder, ld = _as_matrix(polynomials, m) if m else (None, 0)
    out = DeviceVector(max(cols * k, 1))
    _sc._check(_sc.lib().sc_poly_eval_points_dev(holder.ptr if m else None, m, ld, cols, xs.ptr, k, out.ptr, k, None))
    return [DeviceVector.wrap(out.ptr + 16 * k * c, k, out) for c in range(cols)]


# ---- Polynomial.evaluate_domain, interpolate_domain and zerofier_domain (code/univariate.py:104-128) on host lists: the same values
# and list lengths as the host methods, for any points (repeated ones included), no root and no order to pass.
# fast_evaluate_domain goes DIRECT (sc_poly_eval_points: m * k products) when either bound holds and through the domain's tree or
# progression tables (_device_tree) otherwise.  Measured (tools/evaluate_timing.py, profiles/poly_evaluate/):
# with host lists in and out the direct route beat the tree built in the call (the cold figure, which decides) at EVERY shape
# measured, m = 16 .. 16 384 coefficients by k = 16 .. 4 096 points -- x1.8 at 4 096 x 4 096 and at 16 384 x 4 096, x61 at
# 16 384 x 16 -- and the memoised tree (warm) at every shape too (x1.2 at 4 096 x 4 096).  The bounds are therefore the largest
# values measured; beyond BOTH nothing was measured, and the tree's O(k log^2 k) is taken on trust.
EVAL_DIRECT_MAX_POINTS = 4096
EVAL_DIRECT_MAX_COEFFS = 16384


def _domain_field(domain):
    field = domain[0].field
    _require_main_field(field)
    return field


def fast_evaluate_domain(polynomial, domain):
    """Polynomial.evaluate_domain: [polynomial.evaluate(d) for d in domain], one value per point"""
    if not domain:
        return []
    field = _domain_field(domain)
    m, k = polynomial.degree() + 1, len(domain)
    if m == 0:
        return [field.zero() for _ in domain]
    coeffs = _pack(polynomial.coefficients[:m])
    if k <= EVAL_DIRECT_MAX_POINTS or m <= EVAL_DIRECT_MAX_COEFFS:
        out = ctypes.create_string_buffer(16 * k)
        _sc._check(_sc.lib().sc_poly_eval_points(coeffs, m, _pack(domain), k, out))
        return _unpack(out.raw, k, field)
    return _unpack(_device_tree(domain).evaluate(DeviceVector.from_bytes(coeffs)).to_bytes(), k, field)


def fast_evaluate_domain_columns(polynomials, domain):
    """[p.evaluate_domain(domain) for p in polynomials] as one upload, ONE evaluation of all columns and one download"""
    polynomials = list(polynomials)
    if not polynomials or not domain:
        return [[] for _ in polynomials]
    field = _domain_field(domain)
    degrees = [p.degree() for p in polynomials]
    m, k, cols = max(degrees) + 1, len(domain), len(polynomials)
    if m == 0:
        return [[field.zero() for _ in domain] for _ in polynomials]
    matrix = DeviceVector.from_bytes(b"".join(_pack(p.coefficients[:d + 1]) + bytes(16 * (m - d - 1)) for p, d in zip(polynomials, degrees)))
    if k <= EVAL_DIRECT_MAX_POINTS or m <= EVAL_DIRECT_MAX_COEFFS:
        xs, out = DeviceVector.from_bytes(_pack(domain)), DeviceVector(cols * k)
        _sc._check(_sc.lib().sc_poly_eval_points_dev(matrix.ptr, m, m, cols, xs.ptr, k, out.ptr, k, None))
    else:
        out = _device_tree(domain).evaluate_columns(matrix, m, cols)
    flat = _unpack(out.to_bytes(), cols * k, field)
    return [flat[c * k:(c + 1) * k] for c in range(cols)]


def fast_interpolate_domain(domain, values):
    """Polynomial.interpolate_domain: len(domain) coefficients; a repeated point drops its terms as inverse(0) = 0 makes the host
    method drop them (sc_polytree_interpolate_lagrange_columns_dev), nothing is raised"""
    return fast_interpolate_domain_columns(domain, [values])[0]


def fast_interpolate_domain_columns(domain, values_list):
    """[Polynomial.interpolate_domain(domain, v) for v in values_list] as one upload, ONE interpolation of all columns and one download"""
    values_list = list(values_list)
    n = len(domain)
    for values in values_list:
        assert n == len(values), "number of elements in domain does not match number of values -- cannot interpolate"
    assert n > 0, "cannot interpolate between zero points"
    if not values_list:
        return []
    field = _domain_field(domain)
    cols = len(values_list)
    matrix = DeviceVector.from_bytes(b"".join(_pack(values) for values in values_list))
    flat = _unpack(_device_tree(domain).interpolate_lagrange_columns(matrix, cols).to_bytes(), cols * n, field)
    return [Polynomial(flat[c * n:(c + 1) * n]) for c in range(cols)]


def fast_zerofier_domain(domain):
    """Polynomial.zerofier_domain: the len(domain) + 1 coefficients of prod (X - d), multiplicities included"""
    field = _domain_field(domain)
    return Polynomial(_unpack(_device_tree(domain).zerofier().to_bytes(), len(domain) + 1, field))


def fast_coset_evaluate_device(polynomial, offset, generator, order):
    """fast_coset_evaluate with the result left in HBM as a DeviceCodeword."""
    coeffs = polynomial.coefficients
    m = len(coeffs)
    _require_main_field(offset.field)
    out = DeviceVector(order)
    src = DeviceVector.from_bytes(_pack(coeffs)) if m else DeviceVector(1)
    _sc._check(_sc.lib().sc_coset_evaluate_dev(src.ptr, m, _sc.fe_bytes(offset.value), _sc.fe_bytes(generator.value), order, out.ptr, None))
    return DeviceCodeword(out, offset.field)          # (not waited for: `src` is parked behind an event when it is freed)


def fast_coset_evaluate(polynomial, offset, generator, order):
    coeffs = polynomial.coefficients
    m = len(coeffs)
    if order <= 1 or m > order:
        # degenerate shapes: follow the reference's own formula on the host
        padded = polynomial.scale(offset).coefficients + [offset.field.zero()] * (order - m)
        return ntt(generator, padded)
    assert(order & (order - 1) == 0), "cannot compute ntt of non-power-of-two sequence"
    field = offset.field
    assert(generator ^ order == field.one()), "primitive root must be nth root of unity, where n is len(values)"
    assert(generator ^ (order // 2) != field.one()), "primitive root is not primitive nth root of unity, where n is len(values)"
    _require_main_field(field)
    out = ctypes.create_string_buffer(16 * order)
    _sc._check(_sc.lib().sc_coset_evaluate(_pack(coeffs), m, _sc.fe_bytes(offset.value), _sc.fe_bytes(generator.value), order, out))
    return _unpack(out.raw, order, field)


def fast_coset_evaluate_columns(polynomials, offset, generator, order):
    """[fast_coset_evaluate(p, offset, generator, order) for p in polynomials] as ONE call (sc_coset_evaluate_columns_dev): the
    coefficient lists are zero-padded to the longest (padding evaluates to the same values), one upload, one download"""
    polynomials = list(polynomials)
    if not polynomials:
        return []
    lengths = [len(p.coefficients) for p in polynomials]
    if order <= 1 or max(lengths) > order:
        return [fast_coset_evaluate(p, offset, generator, order) for p in polynomials]
    assert(order & (order - 1) == 0), "cannot compute ntt of non-power-of-two sequence"
    field = offset.field
    assert(generator ^ order == field.one()), "primitive root must be nth root of unity, where n is len(values)"
    assert(generator ^ (order // 2) != field.one()), "primitive root is not primitive nth root of unity, where n is len(values)"
    _require_main_field(field)
    m, cols = max(max(lengths), 1), len(polynomials)
    src = DeviceVector.from_bytes(b"".join(_pack(p.coefficients) + bytes(16 * (m - k)) for p, k in zip(polynomials, lengths)))
    out = DeviceVector(cols * order)
    _sc._check(_sc.lib().sc_coset_evaluate_columns_dev(src.ptr, m, cols, _sc.fe_bytes(offset.value), _sc.fe_bytes(generator.value), order, out.ptr, None))
    flat = _unpack(out.to_bytes(), cols * order, field)
    return [flat[c * order:(c + 1) * order] for c in range(cols)]


def fast_coset_divide(lhs, rhs, offset, primitive_root, root_order):  # clean division only!
    _check_root(primitive_root, root_order)
    assert(not rhs.is_zero()), "cannot divide by zero polynomial"
    if lhs.is_zero():
        return Polynomial([])
    dl, dr = lhs.degree(), rhs.degree()
    assert(dr <= dl), "cannot divide by polynomial of larger degree"
    field = lhs.coefficients[0].field
    degree = max(dl, dr)
    if degree < 8:
        return lhs / rhs
    _require_main_field(field)
    root, order = _shrink_order(primitive_root, root_order, degree)
    n_out = dl - dr + 1
    out = ctypes.create_string_buffer(16 * n_out)
    _sc._check(_sc.lib().sc_coset_divide(_pack(lhs.coefficients[:dl + 1]), dl + 1, _pack(rhs.coefficients[:dr + 1]), dr + 1,
                                         _sc.fe_bytes(offset.value), _sc.fe_bytes(root.value), order, out, n_out))
    return Polynomial(_unpack(out.raw, n_out, field))

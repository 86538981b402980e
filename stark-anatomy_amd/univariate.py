"""Dense univariate polynomials over the field: host boundary type `Polynomial`.

Mirrors the interface and list-length conventions of reference code/univariate.py:3-160 (coefficient
lists are little-endian, may carry trailing zeros; `degree()` ignores them, equality ignores them).
Quadratic paths here (schoolbook multiply / long division / Lagrange) are the reference's own
small-degree fallbacks and test oracles; the fast paths live in ntt.py and run on the GPU (`*`, `^`,
`divide` / `/` / `%`, and evaluate_domain / interpolate_domain / zerofier_domain hand long operands to them).
Arithmetic is done on plain ints and wrapped back into FieldElement at the boundary.
"""
from algebra import *


def _wrap(ints, field):
    return [FieldElement(v, field) for v in ints]


def _last_nonzero(ints):
    k = len(ints) - 1
    while k >= 0 and ints[k] == 0:
        k -= 1
    return k


class Polynomial:
    def __init__(self, coefficients):
        self.coefficients = list(coefficients)

    def _values(self):
        return [c.value for c in self.coefficients]

    # -- structure ---------------------------------------------------------------------------
    def degree(self):
        """Index of the last non-zero coefficient; -1 for the zero polynomial (univariate.py:7-17)."""
        return _last_nonzero(self._values())

    def is_zero(self):
        return _last_nonzero(self._values()) < 0

    def leading_coefficient(self):
        # (the zero polynomial indexes with -1 like the reference: last list entry, IndexError on an empty list)
        return self.coefficients[self.degree()]

    def __eq__(self, rhs):
        """univariate.py:66-71: equal degrees, then the reference walks the WHOLE of the left list against the right one, so a
        left operand with more trailing zeros than the right list is long raises IndexError once the real coefficients agree."""
        mine, theirs = self._values(), rhs._values()
        top = _last_nonzero(mine)
        if top != _last_nonzero(theirs):
            return False
        if mine[:top + 1] != theirs[:top + 1]:
            return False
        if top >= 0 and len(mine) > len(theirs):
            raise IndexError("list index out of range")
        return True

    def __neq__(self, rhs):
        return not self == rhs

    __hash__ = None

    def __str__(self):
        return "[%s]" % ",".join(str(c) for c in self.coefficients)

    # -- ring operations ---------------------------------------------------------------------
    def __neg__(self):
        if not self.coefficients:
            return Polynomial([])
        field = self.coefficients[0].field
        return Polynomial(_wrap([(field.p - v) % field.p for v in self._values()], field))

    def __add__(self, rhs):
        # a zero operand hands back the other operand itself (univariate.py:22-26)
        if self.is_zero():
            return rhs
        if rhs.is_zero():
            return self
        field = self.coefficients[0].field
        p = field.p
        a, b = self._values(), rhs._values()
        if len(a) < len(b):
            a, b = b, a
        return Polynomial(_wrap([(v + b[i]) % p if i < len(b) else v for i, v in enumerate(a)], field))

    def __sub__(self, rhs):
        return self + (-rhs)

    # operands at least this long go through the GPU transform instead of the schoolbook loop (same coefficients,
    # same list length; the threshold stays above fast_multiply's own "degree < 8 -> lhs * rhs" fallback)
    FAST_MUL_MIN_LEN = 32

    def __mul__(self, rhs):
        if not self.coefficients or not rhs.coefficients:
            return Polynomial([])
        field = self.coefficients[0].field
        if min(len(self.coefficients), len(rhs.coefficients)) >= Polynomial.FAST_MUL_MIN_LEN and field.p == Field.P_MAIN:
            # Decide on DEGREES, not list lengths: lists may carry trailing zeros, and fast_multiply hands products of
            # degree < 8 straight back to `lhs * rhs` (ntt.py:44-45) -- taking the fast path for those would recurse forever.
            dl, dr = self.degree(), rhs.degree()
            if dl + dr >= 8:
                # Polynomial.__mul__ dominates MPolynomial.evaluate_symbolic (fast_stark.py:109-110) at scale; the product is
                # the same polynomial, so only the time changes
                from ntt import fast_multiply
                full_len = len(self.coefficients) + len(rhs.coefficients) - 1
                order = 1 << max(1, (dl + dr).bit_length())
                product = fast_multiply(self, rhs, field.primitive_nth_root(order), order).coefficients
                return Polynomial(product + [field.zero()] * (full_len - len(product)))
        return self._schoolbook_mul(rhs)

    def _schoolbook_mul(self, rhs):
        """univariate.py:48-57: len(a) + len(b) - 1 coefficients, trailing zeros included"""
        field = self.coefficients[0].field
        p = field.p
        b = rhs._values()
        out = [0] * (len(self.coefficients) + len(b) - 1)
        for i, x in enumerate(self._values()):
            if x:
                for j, y in enumerate(b):
                    out[i + j] = (out[i + j] + x * y) % p
        return Polynomial(_wrap(out, field))

    # divisor and quotient of at least this many coefficients each go through the GPU's division with remainder (ntt.fast_divide:
    # Newton inversion of the reversed divisor, csrc/polydiv.cuh) instead of the long division below: same quotient, same remainder,
    # same list lengths.  Never below 32: short polynomials are divided on machines without a GPU, as FAST_MUL_MIN_LEN assumes.
    # Measured (tools/divide_timing.py, profiles/poly_divide/): at 32 + 32 coefficients the long division
    # still wins (0.17 ms against 0.30), at 64 + 64 the device is 1.9x faster and from there on at every shape measured.
    FAST_DIV_MIN_LEN = 64

    def divide(numerator, denominator):
        """(quotient, remainder); None for a zero denominator (univariate.py:80-97).  Long operands in the main field are divided on
        the GPU, everything else by the reference's long division."""
        if len(denominator.coefficients) >= Polynomial.FAST_DIV_MIN_LEN and len(numerator.coefficients) >= 2 * Polynomial.FAST_DIV_MIN_LEN - 1:
            # decide on DEGREES, not list lengths (lists may carry trailing zeros)
            dd, dn = denominator.degree(), numerator.degree()
            if min(dd + 1, dn - dd + 1) >= Polynomial.FAST_DIV_MIN_LEN and denominator.coefficients[0].field.p == Field.P_MAIN:
                from ntt import fast_divide
                return fast_divide(numerator, denominator)
        return numerator._schoolbook_divide(denominator)

    def _schoolbook_divide(numerator, denominator):
        """Schoolbook long division -> (quotient, remainder); None for a zero denominator (univariate.py:80-97)."""
        dd = denominator.degree()
        if dd == -1:
            return None
        dn = numerator.degree()
        if dn < dd:
            return (Polynomial([]), numerator)
        field = denominator.coefficients[0].field
        p = field.p
        den = denominator._values()
        # the reference's running remainder grows to the subtractee's length when the denominator list
        # carries trailing zeros; keep the same list length
        rem = numerator._values()
        rem += [0] * max(0, (dn - dd) + len(den) - len(rem))
        quo = [0] * (dn - dd + 1)
        lead_inv = pow(den[dd], -1, p)
        top = dn
        while top >= dd:
            c = rem[top] * lead_inv % p
            shift = top - dd
            quo[shift] = c
            for j in range(dd + 1):
                rem[shift + j] = (rem[shift + j] - c * den[j]) % p
            top -= 1
            while top >= 0 and rem[top] == 0:
                top -= 1
        return Polynomial(_wrap(quo, field)), Polynomial(_wrap(rem, field))

    def __truediv__(self, rhs):
        quotient, remainder = self.divide(rhs)            # (a zero divisor: divide gives None and the unpacking raises TypeError)
        assert remainder.is_zero(), "cannot perform polynomial division because remainder is not zero"
        return quotient

    def __mod__(self, rhs):
        _, remainder = self.divide(rhs)
        return remainder

    # a base of at least this many coefficients (up to its degree) raised to an exponent of at least 2 goes through the GPU's power
    # (ntt.fast_power: one forward transform, one pointwise power, one inverse transform, csrc/polymul.cuh) instead of the binary
    # method's ~2 log2(e) products: same coefficients, same list length.  Never below 32: short polynomials are raised on machines
    # without a GPU, as FAST_MUL_MIN_LEN assumes.  10**9: switched off.
    # Measured (tools/multiply_timing.py, profiles/poly_multiply/): from 128 coefficients on fast_power is at
    # least 1.5x faster than the binary method at every exponent measured (at 128: x1.7 for a square, x2.5 for a cube, x3.8 at
    # e = 7, x4.1 at e = 255); at 32 and 64 coefficients a square gains x1.3 and x1.4 only.
    FAST_POW_MIN_LEN = 128

    def __xor__(self, exponent):
        """self^exponent (univariate.py:140-150).  Long bases in the main field are raised on the GPU, everything else by the
        binary method."""
        if exponent >= 2 and len(self.coefficients) >= Polynomial.FAST_POW_MIN_LEN and self.coefficients[0].field.p == Field.P_MAIN:
            # decide on the DEGREE, not the list length (lists may carry trailing zeros)
            if self.degree() + 1 >= Polynomial.FAST_POW_MIN_LEN:
                from ntt import fast_power
                return fast_power(self, exponent)
        return self._binary_power(exponent)

    def _binary_power(self, exponent):
        """self^exponent; the list is exponent * (len - 1) + 1 long whatever the order of the products, so the binary method
        runs from the low bit here (univariate.py:140-150 runs from the high bit)."""
        if self.is_zero():
            return Polynomial([])
        power = Polynomial([self.coefficients[0].field.one()])
        square, e = self, exponent
        while e > 0:
            if e & 1:
                power = power * square
            e >>= 1
            if e:
                square = square * square
        return power

    # -- evaluation / interpolation ----------------------------------------------------------
    def evaluate(self, point):
        """The value at ONE point stays on the host on purpose: packing a coefficient for an upload costs as much Python as its
        Horner step below (0.35 us against 0.3 us), so a device route has nothing to gain from host lists.  A polynomial that
        already lies in HBM is evaluated there: ntt.DevicePolynomial.evaluate."""
        field = point.field
        p = field.p
        x = point.value
        acc = 0
        for v in reversed(self._values()):                # Horner
            acc = (acc * x + v) % p
        return FieldElement(acc, field)

    # The three quadratic methods below hand over to the GPU (ntt.fast_evaluate_domain, fast_interpolate_domain, fast_zerofier_domain:
    # the same values and list lengths for any points, repeated ones included) from these thresholds on, in the main field only.
    # FAST_EVAL_DOMAIN_MIN applies to the number of points AND to degree + 1.  Never below 32: the suite without a GPU and RescuePrime
    # (27 points) run on machines without one, as FAST_DIV_MIN_LEN states.  10**9: switched off.
    # Measured (tools/evaluate_timing.py, profiles/poly_evaluate/), host lists in and out, the rule being the
    # smallest power of two from which the device route is at least 1.5x faster at every larger shape measured (32 .. 4 096 points).
    # The COLD figure decides: the device side with ntt's memo cleared, so that the domain's tree, its inverse series and the weights
    # are built in the call, as a first call on a new domain builds them (the memo holds 8 domains).  zerofier_domain: x0.5 at 32
    # points (0.10 ms on the host against 0.19), x1.6 at 64 (0.36 against 0.22), x680 at 4 096; interpolate_domain: x1.0 at 32 (0.58
    # against 0.61), x2.9 at 64 (2.1 against 0.71), x2 100 at 4 096 (8.0 s against 3.8 ms).  On a memoised domain (warm) both would
    # pass at 32 (x1.9 and x3.8); that is not what decides.  evaluate_domain takes the direct kernel at these shapes and builds no
    # tree: x2.0 at 32 points by 32 coefficients, x1 200 at 4 096 by 4 096, x42 and x16 at the lopsided 32 by 4 096 and 4 096 by 32.
    # Nothing below 32 was measured, and nothing below 32 is allowed.
    FAST_EVAL_DOMAIN_MIN = 32
    FAST_INTERPOLATE_MIN_POINTS = 64
    FAST_ZEROFIER_MIN_POINTS = 64

    def evaluate_domain(self, domain):
        """[self.evaluate(d) for d in domain] (univariate.py:104-105); many points against a long polynomial in the main field are
        evaluated on the GPU"""
        least = Polynomial.FAST_EVAL_DOMAIN_MIN
        if len(domain) >= least and len(self.coefficients) >= least and domain[0].field.p == Field.P_MAIN and self.coefficients[0].field.p == Field.P_MAIN:
            # decide on the DEGREE, not the list length (lists may carry trailing zeros)
            if self.degree() + 1 >= least:
                from ntt import fast_evaluate_domain
                return fast_evaluate_domain(self, domain)
        return self._evaluate_domain_host(domain)

    def _evaluate_domain_host(self, domain):
        return [self.evaluate(d) for d in domain]

    @staticmethod
    def _zerofier_ints(xs, p):
        """coefficients of prod (X - x) over xs, low order first"""
        out = [1]
        for x in xs:
            out = [((out[k - 1] if k else 0) - (x * out[k] if k < len(out) else 0)) % p for k in range(len(out) + 1)]
        return out

    def interpolate_domain(domain, values):
        """the interpolant of univariate.py:107-121, len(domain) coefficients; many points in the main field are interpolated on the
        GPU, repeated abscissas included"""
        if len(domain) >= Polynomial.FAST_INTERPOLATE_MIN_POINTS and len(domain) == len(values) and domain[0].field.p == Field.P_MAIN:
            from ntt import fast_interpolate_domain
            return fast_interpolate_domain(domain, values)
        return Polynomial._interpolate_domain_host(domain, values)

    def _interpolate_domain_host(domain, values):
        """Lagrange interpolation with the results (values AND list length len(domain)) of univariate.py:107-121, in
        O(n^2) instead of its O(n^3): the master polynomial Z = prod (X - x_j) once, then for every point the synthetic
        division Z / (X - x_i) weighted by y_i / prod_{j != i} (x_i - x_j).  The reference inverts each difference through
        Field.inverse, which maps 0 to 0 (algebra.py:87-89): a repeated abscissa silently drops its terms, and so it does here."""
        n = len(domain)
        assert n == len(values), "number of elements in domain does not match number of values -- cannot interpolate"
        assert n > 0, "cannot interpolate between zero points"
        field = domain[0].field
        p = field.p
        xs = [d.value for d in domain]
        master = Polynomial._zerofier_ints(xs, p)
        out = [0] * n
        for i, xi in enumerate(xs):
            denom = 1
            for j, xj in enumerate(xs):
                if j != i:
                    denom = denom * (xi - xj) % p
            weight = values[i].value * pow(denom, -1, p) % p if denom else 0
            if weight == 0:
                continue
            carry = 0
            for k in range(n, 0, -1):                      # quotient of master by (X - xi), high order first
                carry = (master[k] + xi * carry) % p
                out[k - 1] = (out[k - 1] + weight * carry) % p
        return Polynomial(_wrap(out, field))

    def zerofier_domain(domain):
        """prod (X - d) over the domain, len(domain) + 1 coefficients (univariate.py:123-128); many points in the main field are
        multiplied up on the GPU"""
        if len(domain) >= Polynomial.FAST_ZEROFIER_MIN_POINTS and domain[0].field.p == Field.P_MAIN:
            from ntt import fast_zerofier_domain
            return fast_zerofier_domain(domain)
        return Polynomial._zerofier_domain_host(domain)

    def _zerofier_domain_host(domain):
        """prod (X - d) over the domain, len(domain) + 1 coefficients (univariate.py:123-128)"""
        field = domain[0].field
        return Polynomial(_wrap(Polynomial._zerofier_ints([d.value for d in domain], field.p), field))

    def scale(self, factor):
        """coefficient i times factor^i (univariate.py:153-154)."""
        if not self.coefficients:
            return Polynomial([])
        field = self.coefficients[0].field
        p = field.p
        out, f, acc = [], factor.value, 1
        for c in self.coefficients:
            out.append(acc * c.value % p)
            acc = acc * f % p
        return Polynomial(_wrap(out, field))


def test_colinearity(points):
    if len(points) == 3:
        (x0, y0), (x1, y1), (x2, y2) = points
        if x0 != x1 and x0 != x2 and x1 != x2:
            # univariate.py:159-163 interpolates and asks for degree == 1: three points with distinct abscissas lie on a line
            # of non-zero slope (a constant interpolant has degree 0, a parabola 2).  The verifier runs this 3 s (rounds - 1)
            # times (fri.py:207); the cross product is ~40x cheaper than the Lagrange interpolation.
            return (y1 - y0) * (x2 - x0) == (y2 - y0) * (x1 - x0) and y1 != y0
    polynomial = Polynomial.interpolate_domain([x for x, _ in points], [y for _, y in points])
    return polynomial.degree() == 1


test_colinearity.__test__ = False   # a helper (code/fri.py:207 calls it by this name), not a pytest case

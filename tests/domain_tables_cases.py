"""Shapes, operands and exact expectations of the domain-table edge tests: the progression tables of csrc/geoseq.cuh (sc_geodomain_*)
and the subproduct tree of csrc/polytree.cuh (sc_polytree_*), as tests/test_domain_tables_cases_cpu.py runs them through the Python
models and tests/test_gpu_domain_tables_edges.py through the device.

Everything here is Python integers and the definitions (code/ntt.py:66-130 says WHAT a zerofier, a list of values and an interpolant
are); nothing is computed by the code under test, and every comparison is exact.  Test-only.

How much of an output a check looks at:
  * zerofier      X^n - first^n on a full subgroup; the oracle while n <= 513; above that: n + 1 coefficients, monic, and
                  Z(y) = prod (y - x_i) at two seeded y off the domain.  A polynomial of degree <= n that is not Z agrees with Z at no more
                  than n of the p residues, so a wrong zerofier passes the check at one random y with probability at most n / p
                  (< 2^-105 for the longest domain here), and the two y are independent.
  * dense operands   every position by Horner while n * m <= 5 * 10^6 modular products; beyond that the positions `sampled_positions`
                  names: both ends and, on progressions, 2047, 2048, 2049 and n - 2 (the seams of the 2048-element scan workgroups).
  * sparse operands  g = a X^(m-1) + b X^(m // 2) + c has values that cost three powers per point: x_i^e = first^e * (ratio^e)^i by
                  running products on a progression, pow() over arbitrary points.  For the polynomial of n coefficients (`G`) every
                  value is checked at every size, and the interpolant of those values must be g coefficient by coefficient: a COMPLETE
                  check of both directions that shares nothing with the evaluation kernels.
  * constant columns  the interpolant of n values p - 1 is the constant p - 1, of n zeros it is zero (uniqueness): complete as well."""
import collections
import functools
import operator
import random

from oracle import py_oracle as po
import synth

P = po.P
SENTINEL_INT = 0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5         # tests/test_gpu_poly_evaluate.py's: a canonical residue no expected value equals
SENTINEL = SENTINEL_INT.to_bytes(16, "little")
GUARD = 3                                                # sentinel elements in front of and behind every output window
COLS = 3
FULL_HORNER_LIMIT = 5 * 10 ** 6                          # modular products one complete dense check may cost
ORACLE_LIMIT = 513                                       # the reference recursion is quadratic per level
ORACLE_ORDER = 2048
SPARSE_COMPLETE_LIMIT = 5000                             # sparse operands other than G: every point up to this n, sampled above

# ---- elements of a given order ----------------------------------------------------------------------------------------------

def prime_factors(d):
    out, f = [], 2
    while f * f <= d:
        if d % f == 0:
            out.append(f)
            while d % f == 0:
                d //= f
        f += 1
    return out + ([d] if d > 1 else [])


@functools.lru_cache(maxsize=None)
def group_generator():
    """po.GENERATOR where it generates the whole multiplicative group, else the smallest base that does"""
    primes = prime_factors(P - 1)
    for g in [po.GENERATOR] + list(range(2, 1000)):
        if all(pow(g, (P - 1) // r, P) != 1 for r in primes):
            return g
    raise AssertionError("no generator among the small bases")


@functools.lru_cache(maxsize=None)
def element_of_order(d):
    assert (P - 1) % d == 0, d
    h = pow(group_generator(), (P - 1) // d, P)
    assert pow(h, d, P) == 1 and all(pow(h, d // r, P) != 1 for r in prime_factors(d)), d
    return h


ODD_ORDERS = (11, 37, 88, 407, 2368)

# ---- cases ---------------------------------------------------------------------------------------------------------------------

# kind: "scan" (a prefix of a long orbit), "full" (n = ord(ratio)), "prewrap" (n = ord(ratio) - 1), "deep" (three scan levels)
GeoCase = collections.namedtuple("GeoCase", "id first ratio n kind seed")
TreeCase = collections.namedtuple("TreeCase", "id n kind seed")           # n: the number of points (k)
Refusal = collections.namedtuple("Refusal", "id first ratio n")

DEEP_N = (1 << 21) + 1
# The smallest n whose t_j scan has three launch levels is 2^21 + 1, but its outputs read t_j only up to j = 2n - 2 = 2^22, and of the
# middle level's second workgroup (totals 2048 .. 4095) that needs nothing: workgroup b of the top level multiplies by the scanned
# total b - 1, so the second workgroup's scanned totals first reach t_j at j = 2049 * 2048.  A progression reads those from
# n = 2^21 + 1025 on; this one reads two whole workgroups of them (a planted defect in the middle level passes the first deep case and
# fails this one).
DEEP_N_SEEN = (1 << 21) + 2049
BIG_TREE_K = (1 << 18) + 1


def _first_name(first):
    return {1: "1", po.GENERATOR: "g", P - 1: "p-1"}[first]


def _geo_cases():
    out = []

    def add(name, first, ratio, n, kind):
        out.append(GeoCase("%s:n=%d:first=%s" % (name, n, _first_name(first)), first, ratio, n, kind, 910000 + 1000 * len(out)))
    q22 = po.primitive_nth_root(1 << 22)
    for n in (1024, 1025, 2047, 2048, 2049, 2050, 4096, 4097):
        for first in (1, po.GENERATOR):
            add("scan", first, q22, n, "scan")
    for d in ODD_ORDERS:
        for first in (1, po.GENERATOR, P - 1):
            add("full", first, element_of_order(d), d, "full")
    for d in (11, 37, 407, 2368):
        for first in (1, po.GENERATOR):
            add("prewrap", first, element_of_order(d), d - 1, "prewrap")
    add("full", po.GENERATOR, P - 1, 2, "full")          # ratio p - 1 with two points: the full subgroup of order 2
    add("deep", po.GENERATOR, po.primitive_nth_root(1 << 23), DEEP_N, "deep")
    add("deep", po.GENERATOR, po.primitive_nth_root(1 << 23), DEEP_N_SEEN, "deep")
    return tuple(out)


GEO_CASES = _geo_cases()
DEEP_CASES = GEO_CASES[-2:]
DEEP_CASE = DEEP_CASES[0]
SMALL_GEO_CASES = GEO_CASES[:-2]
TREE_CASES = tuple(TreeCase("tree:k=%d" % k, k, "small", 960000 + 1000 * i) for i, k in enumerate((130, 257, 513)))
BIG_TREE_CASE = TreeCase("tree:k=2^18+1", BIG_TREE_K, "big", 970000)

REFUSALS = (
    Refusal("ratio 1, n=2", po.GENERATOR, 1, 2),
    Refusal("ratio p-1, n=3", po.GENERATOR, P - 1, 3),
    Refusal("n=ord+1, ord 11", 1, element_of_order(11), 12),
    Refusal("n=ord+1, ord 2368", 1, element_of_order(2368), 2369),
    Refusal("first 0", 0, po.primitive_nth_root(64), 5),
    Refusal("ratio 0", po.GENERATOR, 0, 5),
    Refusal("first p", P, po.primitive_nth_root(64), 5),
    Refusal("first 2^128-1", (1 << 128) - 1, po.primitive_nth_root(64), 5),
    Refusal("ratio p", po.GENERATOR, P, 5),
    Refusal("ratio p+1", po.GENERATOR, P + 1, 5),
    Refusal("n=0", po.GENERATOR, po.primitive_nth_root(64), 0),
    Refusal("n=1", po.GENERATOR, po.primitive_nth_root(64), 1),
)


def is_geo(case):
    return isinstance(case, GeoCase)


def is_big(case):
    return case.kind in ("deep", "big")


def lengths(case):
    """the numbers of coefficients m a case is evaluated with"""
    n = case.n
    return (3, n, n + 1) if is_big(case) else (0, 1, n, n + 1, 2 * n + 3)


@functools.lru_cache(maxsize=4)
def points(case):
    """every point of the case as a tuple of ints"""
    if is_geo(case):
        out, x = [], case.first % P
        for _ in range(case.n):
            out.append(x)
            x = x * case.ratio % P
        return tuple(out)
    pts = ints_of_stream(case.seed, case.n)
    pts[5], pts[7], pts[11] = 0, 1, P - 1                # 0 is also what the tree pads with
    return tuple(pts)


def point(case, i):
    return case.first * pow(case.ratio, i, P) % P if is_geo(case) else points(case)[i]


def ints_of_stream(seed, n):
    """synth.synth_ints through numpy: the same stream, quick at 2^21 elements"""
    if n == 0:
        return []
    arr = synth.synth_packed(seed, n)
    return [(h << 64) | l for l, h in zip(arr[:, 0].tolist(), arr[:, 1].tolist())]


@functools.lru_cache(maxsize=None)
def sampled_positions(case):
    n = case.n
    if is_geo(case):
        want = {0, n - 1, n - 2, 2047, 2048, 2049}
        if not is_big(case):
            want.add(random.Random(case.seed).randrange(n))
    else:
        want = {0, 1, 5, 7, 11, n // 2, n - 2, n - 1}
    return tuple(sorted(i for i in want if 0 <= i < n))


# ---- operands ------------------------------------------------------------------------------------------------------------------
# evaluation: for every m three polynomials, which are also the three columns of the column call:
#   D<m>  dense: the first m elements of one seeded stream per case (of a second stream for m = 2n + 3)
#   S<m>  sparse: a X^(m-1) + b X^(m // 2) + c (coinciding exponents add up); S<n> is the G of the module's docstring
#   T<m>  D<m> with its top quarter set to zero
# interpolation: "dense" (seeded, one value 0), "G" (the values of S<n>), "pm1" (all p - 1), "zero"

def _base_of(case, m):
    return "B2" if m > case.n + 1 else "B1"


@functools.lru_cache(maxsize=2)
def _base(case, which):
    return ints_of_stream(case.seed + (1 if which == "B1" else 2), case.n + 1 if which == "B1" else 2 * case.n + 3)


def _cut(kind, m):
    return m - m // 4 if kind == "T" else m


def sparse_terms(case, m):
    """{exponent: coefficient} of S<m>"""
    a, b, c = ((v % (P - 1)) + 1 for v in synth.synth_ints(case.seed + 3 + 7 * (m % 1000), 3))
    terms = {}
    for e, v in ((m - 1, a), (m // 2, b), (0, c)):
        terms[e] = (terms.get(e, 0) + v) % P
    return terms


def evaluation_operands(m):
    return () if m == 0 else ("D%d" % m, "S%d" % m, "T%d" % m)


def coefficients(case, name):
    """the m coefficients of an evaluation operand as a list of ints"""
    kind, m = name[0], int(name[1:])
    if kind == "S":
        out = [0] * m
        for e, v in sparse_terms(case, m).items():
            out[e] = v
        return out
    cut = _cut(kind, m)
    return _base(case, _base_of(case, m))[:cut] + [0] * (m - cut)


def interpolation_values(case, name):
    n = case.n
    if name == "dense":
        vals = ints_of_stream(case.seed + 4, n)
        vals[1] = 0
        return vals
    if name == "G":
        return list(g_values(case))
    return [P - 1 if name == "pm1" else 0] * n


def packed_coefficients(case, name):
    """synth.pack_ints(coefficients(case, name)), the dense ones straight from the stream's limbs"""
    kind, m = name[0], int(name[1:])
    if kind == "S":
        return synth.pack_ints(coefficients(case, name))
    cut = _cut(kind, m)
    return synth.synth_packed(case.seed + (1 if _base_of(case, m) == "B1" else 2), cut).tobytes() + bytes(16 * (m - cut))


def packed_interpolation_values(case, name):
    n = case.n
    if name == "dense":
        raw = synth.synth_packed(case.seed + 4, n).tobytes()
        return raw[:16] + bytes(16) + raw[32:]
    if name == "G":
        return synth.pack_ints(g_values(case))
    return ((P - 1).to_bytes(16, "little") if name == "pm1" else bytes(16)) * n


INTERPOLATION_OPERANDS = ("dense", "G", "pm1", "zero")
INTERPOLATION_COLUMNS = ("dense", "G", "pm1")


# ---- expectations --------------------------------------------------------------------------------------------------------------

class Packed:
    """an output as it comes off the device (16 bytes per element) that answers the checks below like a list of ints: a check that
    looks at a few positions of 2^21 does not unpack the rest, one that compares everything compares bytes"""

    def __init__(self, raw):
        self.raw = bytes(raw)

    def __len__(self):
        return len(self.raw) // 16

    def __getitem__(self, i):
        return int.from_bytes(self.raw[16 * i:16 * i + 16], "little")

    def __eq__(self, other):
        return self.raw == (other.raw if isinstance(other, Packed) else synth.pack_ints(other))

    def __ne__(self, other):
        return not self == other


def as_list(got):
    return synth.unpack_ints(got.raw) if isinstance(got, Packed) else got


HORNER_BLOCK = 4096


def horner(coeffs, x):
    """sum c_i x^i.  Long polynomials go block by block, sum_j (x^B)^j * (sum_{i<B} c_(jB+i) x^i) with the inner sums as one
    sum(map(mul, ...)) over a table of x^0 .. x^(B-1): the same integers as the plain loop, a third of its time at 2^21 coefficients"""
    coeffs = as_list(coeffs)
    acc = 0
    if len(coeffs) <= 2 * HORNER_BLOCK:
        for v in reversed(coeffs):
            acc = (acc * x + v) % P
        return acc
    pows = [1]
    for _ in range(HORNER_BLOCK - 1):
        pows.append(pows[-1] * x % P)
    xb = pows[-1] * x % P
    for lo in range((len(coeffs) - 1) // HORNER_BLOCK * HORNER_BLOCK, -1, -HORNER_BLOCK):
        acc = (acc * xb + sum(map(operator.mul, coeffs[lo:lo + HORNER_BLOCK], pows))) % P
    return acc


def prefix_values(coeffs, x, cuts):
    """{cut: value at x of coeffs[:cut]} for every cut, in one pass: Horner over each segment between two cuts"""
    out, total, lo = {}, 0, 0
    for cut in sorted(set(cuts)):
        total = (total + horner(coeffs[lo:cut], x) * pow(x, lo, P)) % P
        out[cut] = total
        lo = cut
    return out


@functools.lru_cache(maxsize=None)
def _dense_at(case, which, i):
    """the values at point i of the dense operands cut out of one base stream: of all of them at a sampled position, elsewhere of those
    that are checked at every position"""
    everywhere = i not in sampled_positions(case)
    ms = [m for m in lengths(case) if m and _base_of(case, m) == which and not (everywhere and case.n * m > FULL_HORNER_LIMIT)]
    return prefix_values(_base(case, which), point(case, i), [_cut(kind, m) for m in ms for kind in "DT"])


def sparse_values(case, terms):
    """the values of a sparse polynomial at EVERY point: running products on a progression, pow() over arbitrary points"""
    n = case.n
    out = [terms.get(0, 0)] * n
    for e, v in terms.items():
        if e == 0:
            continue
        if is_geo(case):
            x, r = v * pow(case.first, e, P) % P, pow(case.ratio, e, P)
            for i in range(n):
                out[i] += x
                x = x * r % P
        else:
            for i, d in enumerate(points(case)):
                out[i] += v * pow(d, e, P)
    return [w % P for w in out]


@functools.lru_cache(maxsize=2)
def g_values(case):
    """the values of G = S<n> at every point"""
    return tuple(sparse_values(case, sparse_terms(case, case.n)))


def check_values(case, name, got):
    """`got`: the n values the code under test gives for evaluation operand `name`.  Returns how many positions were compared."""
    n = case.n
    kind, m = name[0], int(name[1:])
    assert len(got) == n, (case.id, name, len(got))
    if kind == "S":
        terms = sparse_terms(case, m)
        if m == n or n <= SPARSE_COMPLETE_LIMIT:
            assert got == (list(g_values(case)) if m == n else sparse_values(case, terms)), (case.id, name)
            return n
        for i in sampled_positions(case):
            x = point(case, i)
            assert got[i] == sum(v * pow(x, e, P) for e, v in terms.items()) % P, (case.id, name, i)
        return len(sampled_positions(case))
    positions = range(n) if n * m <= FULL_HORNER_LIMIT else sampled_positions(case)
    which, cut = _base_of(case, m), _cut(kind, m)
    for i in positions:
        assert got[i] == _dense_at(case, which, i)[cut], (case.id, name, i)
    return len(positions)


def zero_polynomial_values(case):
    return [0] * case.n


@functools.lru_cache(maxsize=None)
def _oracle_interpolant(case):
    got = po.fast_interpolate(list(points(case)), interpolation_values(case, "dense"), po.primitive_nth_root(ORACLE_ORDER), ORACLE_ORDER)
    return got + [0] * (case.n - len(got))


def check_interpolant(case, name, got):
    """`got`: the n coefficients the code under test gives for the values `name`"""
    n = case.n
    assert len(got) == n, (case.id, name, len(got))
    if name == "G":
        assert got == coefficients(case, "S%d" % n), (case.id, name)
    elif name == "pm1":
        assert got == [P - 1] + [0] * (n - 1), (case.id, name)
    elif name == "zero":
        assert got == [0] * n, (case.id, name)
    elif n <= ORACLE_LIMIT:
        assert got == _oracle_interpolant(case), (case.id, name)
    else:
        vals = interpolation_values(case, name)                  # fewer than n + 1 coefficients that take the n values: the interpolant
        ints = as_list(got)
        for i in (range(n) if n * n <= FULL_HORNER_LIMIT else sampled_positions(case)):
            assert horner(ints, point(case, i)) == vals[i], (case.id, name, i)


def full_subgroup(case):
    return is_geo(case) and case.kind == "full"


def check_zerofier(case, got):
    n = case.n
    assert len(got) == n + 1 and got[n] == 1, (case.id, len(got))
    if full_subgroup(case):
        assert got == [(-pow(case.first, n, P)) % P] + [0] * (n - 1) + [1], case.id
    elif n <= ORACLE_LIMIT:
        assert got == po.fast_zerofier(list(points(case)), po.primitive_nth_root(ORACLE_ORDER), ORACLE_ORDER), case.id
    else:
        ys = synth.synth_ints(case.seed + 5, 2)
        prods = [1, 1]
        if is_geo(case):
            x, q, (y0, y1), p0, p1 = case.first % P, case.ratio, ys, 1, 1
            for _ in range(n):
                p0, p1, x = p0 * (y0 - x) % P, p1 * (y1 - x) % P, x * q % P
            prods = [p0, p1]
        else:
            for x in points(case):
                prods = [prods[0] * (ys[0] - x) % P, prods[1] * (ys[1] - x) % P]
        ints = as_list(got)
        for y, prod in zip(ys, prods):
            assert prod != 0, "a seeded y lies on the domain"
            assert horner(ints, y) == prod, (case.id, y)

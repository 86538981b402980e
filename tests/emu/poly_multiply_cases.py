"""The shapes, operands and exact expectations the multiplication tests share (tests/test_poly_multiply_model.py on the host,
tests/test_gpu_poly_multiply.py and tests/test_gpu_poly_multiply_streams.py on the device).  Expectations are products of Python
integers, never the code under test: the schoolbook product up to 512 x 512 coefficients, Kronecker substitution above.  Test-only."""
import functools

from oracle import py_oracle as po
import synth

P = po.P
EDGES = (0, 1, P - 1, 1 << 64, (1 << 119) + 1)

# (na, nb): constants and the smallest transforms; results of 8 and 64 (the transform exactly full) and 9 and 65 (the size
# doubles); 2^11 (the last one-pass plan, exactly full) and 2^11 + 1 (the first two-pass plan); 2^12 exactly full and 2^12 + 1;
# lopsided
MUL_SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (5, 4), (5, 5), (33, 32), (33, 33), (1025, 1024), (1025, 1025), (2049, 2048), (2049, 2049),
              (4097, 8), (8, 4097))
# (na, exponent): trivial exponents and constants; results of 256 (exactly full) and 257; a real base with a high-bit exponent; 4097
POW_SHAPES = ((1, 0), (1, 5), (4, 0), (4, 1), (4, 2), (4, 3), (2, 255), (2, 256), (33, 5), (33, 255), (1025, 4))
# (count, n): odd carries on several levels, powers of two and others, a level that crosses into a two-pass transform
PRODUCT_SHAPES = ((1, 4), (2, 4), (3, 4), (5, 2), (7, 3), (8, 2), (64, 2), (33, 33), (17, 129))
COLUMN_COUNTS = (1, 3, 5, 16)
COLUMN_SHAPES = ((5, 4), (33, 33), (7, 1))
SCHOOLBOOK_MAX = 512


def schoolbook(a, b):
    """Polynomial._schoolbook_mul on integers: len(a) + len(b) - 1 coefficients, trailing zeros included"""
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return [v % P for v in out]


def kronecker(a, b):
    """the same list by Kronecker substitution: each operand packed into one integer, a slot of 2 * 128 + bit_length(min(na, nb))
    bits per coefficient (rounded up to whole bytes) holds every coefficient of the integer product without carry into the next"""
    slot = (2 * 128 + min(len(a), len(b)).bit_length() + 7) // 8
    pack = lambda v: int.from_bytes(b"".join(x.to_bytes(slot, "little") for x in v), "little")
    n = len(a) + len(b) - 1
    raw = (pack(a) * pack(b)).to_bytes(slot * (n + 1), "little")
    return [int.from_bytes(raw[slot * i:slot * (i + 1)], "little") % P for i in range(n)]


def exact_product(a, b):
    return schoolbook(a, b) if max(len(a), len(b)) <= SCHOOLBOOK_MAX else kronecker(a, b)


def exact_power(a, exponent):
    """Polynomial.__xor__'s list for a non-zero a: exponent * (len(a) - 1) + 1 coefficients, by repeated exact products"""
    out, square = [1], [v % P for v in a]
    while exponent:
        if exponent & 1:
            out = kronecker(out, square)
        exponent >>= 1
        if exponent:
            square = kronecker(square, square)
    return out


def exact_product_of(rows):
    """the left-to-right product"""
    out = rows[0]
    for r in rows[1:]:
        out = kronecker(out, r)
    return [v % P for v in out]


def _edges(values, shift):
    return [EDGES[(i + shift) % 5] if i % 3 == 0 else v for i, v in enumerate(values)]


@functools.lru_cache(maxsize=None)
def mul_operands(na, nb):
    """((label, a, b), ...) of one shape"""
    seed = 9000 + 131 * na + nb
    a, b = synth.synth_ints(seed, na), synth.synth_ints(seed + 1, nb)
    out = [("general", a, b)]
    out.append(("zero top coefficients", a[:max(na - 2, 0)] + [0] * min(2, na), b[:max(nb - 1, 0)] + [0]))
    out.append(("all-zero multiplicand", a, [0] * nb))
    out.append(("all-zero both", [0] * na, [0] * nb))
    out.append(("edge residues", _edges(a, na), _edges(b, nb)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mul_expected(na, nb):
    return tuple(exact_product(a, b) for _, a, b in mul_operands(na, nb))


@functools.lru_cache(maxsize=None)
def square_operand(n):
    return synth.synth_ints(9500 + n, n)


@functools.lru_cache(maxsize=None)
def pow_operands(na, exponent):
    """((label, a), ...): the all-zero base is part of the device tests only (the ABI gives zeros -- or the 1 of exponent 0 -- where
    Polynomial.__xor__ gives the empty polynomial)"""
    seed = 9300 + 131 * na + exponent
    a = synth.synth_ints(seed, na)
    out = [("general", a), ("edge residues", _edges(a, exponent))]
    if na > 1:
        out.append(("zero top coefficient", a[:-1] + [0]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pow_expected(na, exponent):
    return tuple(exact_power(a, exponent) for _, a in pow_operands(na, exponent))


@functools.lru_cache(maxsize=None)
def product_rows(count, n):
    """`count` rows of n coefficients: general rows, one with a zero top coefficient, one of edge residues"""
    rows = [synth.synth_ints(9700 + 17 * count + 3 * n + j, n) for j in range(count)]
    if count > 1 and n > 1:
        rows[1] = rows[1][:-1] + [0]
    rows[-1] = _edges(rows[-1], count)
    return tuple(tuple(r) for r in rows)


@functools.lru_cache(maxsize=None)
def product_expected(count, n):
    return exact_product_of([list(r) for r in product_rows(count, n)])


@functools.lru_cache(maxsize=None)
def column_operands(na, nb, cols):
    """(columns, multiplicands): `cols` multiplicands-to-be of na coefficients and as many of nb; column 1 has zero top coefficients,
    column 2 is all zero"""
    columns = [synth.synth_ints(9800 + 31 * c + na, na) for c in range(cols)]
    others = [synth.synth_ints(9900 + 37 * c + nb, nb) for c in range(cols)]
    if cols > 1:
        columns[1] = columns[1][:max(na - 2, 0)] + [0] * min(2, na)
    if cols > 2:
        columns[2] = [0] * na
    return columns, others

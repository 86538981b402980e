"""Executable model of the device algorithms behind sc_poly_mul_dev, sc_poly_mul_columns_dev, sc_poly_pow_dev and
sc_poly_product_dev (csrc/polymul.cuh; polymul_columns, polypow and polyproduct in csrc/polytree_geo.hip): Polynomial.__mul__
(code/univariate.py:48-57) and Polynomial.__xor__ (code/univariate.py:140-150) through cyclic products.

A result of `length` coefficients is computed at n = 2^ceil(log2 length), at least 2: the operands are zero-extended to n by the
forward transforms (`in_limit`), multiplied or raised pointwise together with the inverse transform's n^-1, transformed back
without scaling, and the first `length` values are stored.  n >= length, so the cyclic product is the product; one step smaller
and it wraps (wrapped_product below shows what that would give).

Every array operation below corresponds to one kernel launch or transform of the device code, with the same truncation lengths,
transform sizes, sets of columns and tree levels.  Test-only.
"""
from oracle import py_oracle as po
import synth

P = po.P
MAX_SET_COLUMNS = 65535          # grid.y


def transform_log(length):
    """pm_log: log2 of the transform size of a result of `length` coefficients"""
    return max(1, (length - 1).bit_length())


def transform(values, limit, n, inverse=False):
    """ntt_device at size n with in_limit = limit: the input behind `limit` reads as zero; the inverse does not scale"""
    padded = [v % P for v in values[:limit]] + [0] * (n - min(limit, len(values)))
    root = po.primitive_nth_root(n)
    if inverse:
        return [v * n % P for v in synth.unpack_ints(po.C.intt(root, synth.pack_ints(padded), n))]
    return synth.unpack_ints(po.C.ntt(root, synth.pack_ints(padded), n))


def per_set(n, launch_log=26, least=1):
    """pm_per_set: the columns one set of launches takes at transform size n"""
    return max(least, min((1 << launch_log) // n, MAX_SET_COLUMNS))


def cyclic_product(x, y, n):
    """pm_mul_kernel between transforms of size n, on operands already zero-extended by their transforms"""
    fx, fy = transform(x, len(x), n), transform(y, len(y), n)
    k = po.inv(n)
    return transform([k * u * v % P for u, v in zip(fx, fy)], n, n, inverse=True)


def wrapped_product(a, b):
    """what a transform one step too small would give: the product folded onto n / 2 entries"""
    n = 1 << transform_log(len(a) + len(b) - 1)
    half = max(n // 2, 1)
    fold = lambda v: [sum(v[i::half]) % P for i in range(min(half, len(v)))]
    return cyclic_product(fold(a), fold(b), max(half, 2))[:half]


def multiply_columns_model(columns, multiplicands, launch_log=26, trace=None):
    """sc_poly_mul_columns_dev: columns of na, multiplicands of nb coefficients (ONE multiplicand list: ld_b == 0, else one per
    column) -> one list of na + nb - 1 coefficients per column.  trace (a list) receives (n, [columns per set])."""
    shared = not isinstance(multiplicands[0], list)
    na, nb = len(columns[0]), len(multiplicands if shared else multiplicands[0])
    length = na + nb - 1
    n = 1 << transform_log(length)
    per = min(per_set(n, launch_log), len(columns))
    k = po.inv(n)
    Bf = transform(multiplicands, nb, n) if shared else None             # once per call
    out, sets = [], []
    for done in range(0, len(columns), per):
        chunk = columns[done:done + per]
        sets.append(len(chunk))
        X = [transform(a, na, n) for a in chunk]                         # one columns transform, read at ld_a
        Y = [Bf] * len(chunk) if shared else [transform(b, nb, n) for b in multiplicands[done:done + per]]
        X = [[k * u * v % P for u, v in zip(x, y)] for x, y in zip(X, Y)]   # pm_mul_kernel
        Y = [transform(x, n, n, inverse=True) for x in X]                # one inverse columns transform
        out += [y[:length] for y in Y]                                   # pm_store_kernel
    if trace is not None:
        trace.append((n, sets))
    return out


def multiply_model(a, b):
    """sc_poly_mul_dev: the columns entry with one column (a square transforms its operand once: the same values)"""
    return multiply_columns_model([a], [b])[0]


def power_model(a, exponent):
    """sc_poly_pow_dev: exponent * (len(a) - 1) + 1 coefficients"""
    if exponent == 0:
        return [1]                                                       # pt_fill_kernel
    if exponent == 1:
        return [v % P for v in a]                                        # a copy
    length = exponent * (len(a) - 1) + 1
    n = 1 << transform_log(length)
    X = transform(a, len(a), n)
    k = po.inv(n)
    X = [k * pow(v, exponent, P) % P for v in X]                         # pm_pow_kernel
    return transform(X, n, n, inverse=True)[:length]


def product_levels(count, n0):
    """[(rows, length, out_length, n)] of the tree of sc_poly_product_dev: `rows` rows of `length` coefficients become
    (rows + 1) // 2 rows of out_length = min(2 length - 1, total) at transform size n"""
    total = count * (n0 - 1) + 1
    levels, rows, length = [], count, n0
    while rows > 1:
        out_length = min(2 * length - 1, total)
        levels.append((rows, length, out_length, 1 << transform_log(out_length)))
        rows, length = (rows + 1) // 2, out_length
    return levels


def product_model(rows, launch_log=26, trace=None):
    """sc_poly_product_dev: the product of the rows (lists of one length n0), count * (n0 - 1) + 1 coefficients.  trace (a list)
    receives per level (n, [rows per set], carried: bool)."""
    count, n0 = len(rows), len(rows[0])
    total = count * (n0 - 1) + 1
    level = [[v % P for v in r] for r in rows]
    for nrows, length, out_length, n in product_levels(count, n0):
        assert nrows == len(level)
        paired = nrows & ~1
        per = min(per_set(n, launch_log, least=2) & ~1, paired)
        k = po.inv(n)
        above, sets = [], []
        for done in range(0, paired, per):
            chunk = level[done:done + per]
            sets.append(len(chunk))
            F = [transform(r, length, n) for r in chunk]                 # one columns transform of the set's rows
            G = [[k * u * v % P for u, v in zip(F[2 * j], F[2 * j + 1])] for j in range(len(chunk) // 2)]   # pm_mul_kernel, pairwise
            above += [transform(g, n, n, inverse=True) for g in G]       # one inverse columns transform: rows at pitch n
        if nrows & 1:
            above.append(level[paired][:length] + [0] * (out_length - length))   # the odd last row, carried up and zero-extended
        if trace is not None:
            trace.append((n, sets, bool(nrows & 1)))
        level = above
    return level[0][:total]

"""Executable model of the device algorithm behind sc_poly_eval_points_dev (csrc/polyeval.cuh; polyeval_enqueue in
csrc/polyeval.hip): Polynomial.evaluate / evaluate_domain (code/univariate.py:99-105) as m * k * cols modular products.

Every function below is one kernel: the same chunking of the coefficients, the same Horner stride x^T per thread with its top
step guarded (the per-thread tail), the same tree through the workgroup's accumulators whose level h folds a_(t+h) x^h into a_t,
the same split of the points between the two forms, the same second launch over the partials.  The arithmetic is exact on both
sides, so the model works on plain residues (the device keeps the powers of x as Montgomery forms; the values are the same).
Also the formula sc_polytree_interpolate_lagrange_columns_dev computes (lagrange_inv0).  Test-only.
"""
from oracle import py_oracle as po

P = po.P
T = 256                      # PE_T
W = 64                       # PE_W
WAYS = 4                     # PE_WAYS
UNITS_WANTED = 16384         # PE_UNITS_WANTED: quarter waves
UNITS_PER_WG = 16            # PE_UNITS_PER_WG
CHUNK_LOG = 8                # sc_set_tuning("eval_chunk_log") by default
ACROSS_MIN = 32              # sc_set_tuning("eval_points_across_min") by default
ACROSS_MIN_PRODUCTS_LOG = 26 # sc_set_tuning("eval_across_min_products_log") by default


def horner(coeffs, x):
    """Polynomial.evaluate on integers"""
    acc = 0
    for v in reversed(coeffs):
        acc = (acc * x + v) % P
    return acc


def ilog2(n):
    """the smallest l with 2^l >= n"""
    return max(n - 1, 0).bit_length()


def fold(acc, x):
    """the tree of pe_coeffs_across_kernel / pe_combine_kernel over len(acc) = 2^b accumulators: sum_t acc[t] x^t"""
    acc = list(acc)
    powers = [pow(x, 1 << b, P) for b in range(ilog2(len(acc)))]       # the squarings on the way to x^T
    for b in reversed(range(len(powers))):
        h = 1 << b
        for t in range(h):
            acc[t] = (acc[t] + acc[t + h] * powers[b]) % P
    return acc[0]


def strided(values, x, lanes, steps_out=None):
    """lane t walks values t, t + lanes, ... by Horner in x^lanes (top step guarded), then the fold"""
    n = len(values)
    steps = (n + lanes - 1) // lanes
    if steps_out is not None:
        steps_out.append([sum(1 for s in range(steps) if t + s * lanes < n) for t in range(lanes)])
    xl = pow(x, lanes, P)
    acc = []
    for t in range(lanes):
        top = t + (steps - 1) * lanes
        a = values[top] if top < n else 0
        for s in reversed(range(steps - 1)):
            a = (a * xl + values[t + s * lanes]) % P
        acc.append(a)
    return fold(acc, x)


def coeffs_across(chunk, xs, steps_out=None):
    """pe_coeffs_across_kernel for one chunk and one group of points: one partial per point"""
    return [strided(chunk, x, T, steps_out) for x in xs]


def points_across(chunk, xs):
    """pe_points_across_kernel for one chunk: per lane WAYS Horner chains in x^WAYS over the coefficients WAYS i + r (top group
    guarded), folded as a_0 + x (a_1 + x (a_2 + x a_3))"""
    n = len(chunk)
    groups = (n + WAYS - 1) // WAYS
    out = []
    for x in xs:
        y = pow(x, WAYS, P)
        top = (groups - 1) * WAYS
        acc = [chunk[top + r] if top + r < n else 0 for r in range(WAYS)]
        for i in reversed(range(groups - 1)):
            acc = [(a * y + chunk[i * WAYS + r]) % P for r, a in enumerate(acc)]
        out.append(horner(acc, x))
    return out


def combine(partials, x, chunk_log):
    """pe_combine_kernel for one output: the partials are the coefficients of a polynomial in y = x^(2^chunk_log)"""
    return strided(partials, pow(x, 1 << chunk_log, P), W)


def across(k, products, across_min=ACROSS_MIN, products_log=ACROSS_MIN_PRODUCTS_LOG):
    """polyeval_across: points [0, kb) go points-across-lanes, the rest coefficients-across-lanes; only in calls of at least
    2^products_log products"""
    if k < across_min or products >> products_log == 0:
        return 0
    rest = k % W
    return k if rest >= across_min or rest == 0 else k - rest


def plan(m, k, cols, chunk_log=CHUNK_LOG, across_min=ACROSS_MIN, products_log=ACROSS_MIN_PRODUCTS_LOG):
    """(kb, G, chunk_log, chunks) as polyeval_enqueue chooses them"""
    kb = across(k, m * k * cols, across_min, products_log)
    ka = k - kb
    G = 1 if ka == 1 else (2 if ka == 2 else 4)
    units = ((kb + W - 1) // W + (ka + G - 1) // G * UNITS_PER_WG) * cols
    wanted = (UNITS_WANTED + units - 1) // units
    log = max(chunk_log, ilog2((m + wanted - 1) // wanted))
    return kb, G, log, (m + (1 << log) - 1) >> log


def eval_points_model(columns, points, chunk_log=CHUNK_LOG, across_min=ACROSS_MIN, products_log=ACROSS_MIN_PRODUCTS_LOG, trace=None):
    """sc_poly_eval_points_dev: columns of m coefficients each at the k points -> one list of k values per column.  trace (a dict)
    receives the plan and the per-thread step counts of the last coefficients-across-lanes workgroup."""
    k = len(points)
    if k == 0 or not columns:
        return [[] for _ in columns]
    m = len(columns[0])
    if m == 0:
        return [[0] * k for _ in columns]                                  # pe_zero_kernel
    kb, G, log, chunks = plan(m, k, len(columns), chunk_log, across_min, products_log)
    steps = []
    out = []
    for column in columns:
        partial = [[0] * chunks for _ in range(k)]
        for ch in range(chunks):
            chunk = column[ch << log:(ch + 1) << log]
            for j, v in enumerate(points_across(chunk, points[:kb])):
                partial[j][ch] = v
            for j0 in range(kb, k, G):
                group = [points[min(j, k - 1)] for j in range(j0, j0 + G)]  # indices past k repeat the last point ...
                for g, v in enumerate(coeffs_across(chunk, group, steps)):
                    if j0 + g < k:                                          # ... and are not stored
                        partial[j0 + g][ch] = v
        out.append([row[0] if chunks == 1 else combine(row, x, log) for row, x in zip(partial, points)])
    if trace is not None:
        trace.update(kb=kb, G=G, chunk_log=log, chunks=chunks, steps=steps[-1] if steps else None)
    return out


def inv0(v):
    """Field.inverse (code/algebra.py:87-89): 0 for 0"""
    return pow(v, P - 2, P)


def zerofier(xs):
    out = [1]
    for x in xs:
        out = [((out[i - 1] if i else 0) - (x * out[i] if i < len(out) else 0)) % P for i in range(len(out) + 1)]
    return out


def lagrange_inv0(xs, ys):
    """sum_i y_i * inv0(Z'(x_i)) * Z(X) / (X - x_i), Z the zerofier of all points with their multiplicities: len(xs) coefficients"""
    n = len(xs)
    Z = zerofier(xs)
    dZ = [(i * Z[i]) % P for i in range(1, n + 1)]
    out = [0] * n
    for x, y in zip(xs, ys):
        w = y * inv0(horner(dZ, x)) % P
        carry = 0
        for i in range(n, 0, -1):                                           # Z / (X - x), high order first
            carry = (Z[i] + x * carry) % P
            out[i - 1] = (out[i - 1] + w * carry) % P
    return out

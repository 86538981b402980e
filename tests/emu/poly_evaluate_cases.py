"""The shapes, operands and exact expectations the evaluation tests share (tests/test_poly_evaluate_model.py on the host,
tests/test_gpu_poly_evaluate.py on the device).  Expectations are Python integers, never the code under test: plain Horner for
the values, the Lagrange formula with inverse(0) = 0 for the interpolants.  Test-only."""
import functools

from oracle import py_oracle as po
import synth

P = po.P


def horner(coeffs, x):
    acc = 0
    for v in reversed(coeffs):
        acc = (acc * x + v) % P
    return acc


def lengths(chunk_log):
    """m: nothing, below / at / above one wave, one workgroup's chunk - 1 / exact / + 1, three chunks + 1"""
    chunk = 1 << chunk_log
    return (0, 1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 1)


GPU_CHUNK_LOG = 10                       # three chunks + 1 = 3 073 coefficients
GPU_POINT_COUNTS = (1, 2, 3, 63, 64, 65, 257)
MODEL_CHUNK_LOG = 9                      # two Horner steps per thread in a full chunk
MODEL_POINT_COUNTS = (1, 2, 3, 5, 31, 32, 65)
COLUMN_PATTERNS = ("random", "all p - 1", "all zero")


@functools.lru_cache(maxsize=None)
def points(chunk_log, count=257):
    """a random residue first (k = 1 must not be the point 0), then 0, 1, p - 1, a root of unity whose order (256) divides the
    Horner stride and the chunk length (x^T = x^chunk = 1), one of order 2^(chunk_log + 1) (x^chunk = -1), a repeat of the first
    point, random residues"""
    rnd = synth.synth_ints(7100 + chunk_log, count)
    special = [rnd[0], 0, 1, P - 1, po.primitive_nth_root(256), po.primitive_nth_root(2 << chunk_log), rnd[0]]
    return tuple(special + rnd[len(special):])


@functools.lru_cache(maxsize=None)
def column(pattern, m, which=0):
    if pattern == "random":
        return tuple(synth.synth_ints(7200 + 7 * m + which, m))
    return tuple([P - 1 if pattern == "all p - 1" else 0] * m)


@functools.lru_cache(maxsize=None)
def _values_at_all_points(pattern, m, which, chunk_log):
    coeffs = column(pattern, m, which)
    return tuple(horner(coeffs, x) for x in points(chunk_log))


def values(pattern, m, which, chunk_log, k):
    """Horner, once per column: the values at the first k points"""
    if pattern == "all zero":
        return tuple([0] * k)
    return _values_at_all_points(pattern, m, which, chunk_log)[:k]


def matrix(m, cols, lead):
    """[(pattern, which)] of the columns of a matrix: one column of pattern `lead`; three: `lead`, all p - 1, another random one"""
    return [(lead, 0)] if cols == 1 else [(lead, 0), ("all p - 1", 0), ("random", 1)]


# ---- interpolation with inverse(0) = 0
LAGRANGE_COUNTS = (1, 2, 3, 16, 17, 33, 100)


def lagrange_patterns(k):
    """(label, points) for k points: distinct; a repeated pair in adjacent leaves; one at positions 0 and k - 1; a triple; all equal;
    a real point 0 beside the padding (k not a power of two); 0 repeated -- those that k points can hold"""
    base = synth.synth_ints(7300 + k, k)
    assert len(set(base)) == k and 0 not in base
    out = [("distinct", list(base))]
    if k >= 2:
        pair = list(base); pair[1] = pair[0]
        out.append(("adjacent pair", pair))
        ends = list(base); ends[k - 1] = ends[0]
        out.append(("pair at 0 and k - 1", ends))
        out.append(("all equal", [base[0]] * k))
        zeros = list(base); zeros[0] = zeros[k // 2] = 0
        out.append(("0 repeated", zeros))
    if k >= 3:
        triple = list(base); triple[k // 2] = triple[k - 1] = triple[0]
        out.append(("triple", triple))
    if k & (k - 1):
        zero = list(base); zero[k - 1] = 0
        out.append(("a real 0 beside the padding", zero))
    return out


def lagrange_values(k, cols):
    """value columns: all zeros, random ones"""
    return [[0] * k] + [synth.synth_ints(7400 + 3 * k + c, k) for c in range(max(cols - 1, 1))]


def lagrange_expected(xs, ys):
    """sum_i y_i * inv0(Z'(x_i)) * Z(X) / (X - x_i) on integers, by the definition: Z'(x_i) = prod_(j != i) (x_i - x_j), the
    quotient by synthetic division"""
    n = len(xs)
    Z = [1]
    for x in xs:
        Z = [((Z[i - 1] if i else 0) - (x * Z[i] if i < len(Z) else 0)) % P for i in range(len(Z) + 1)]
    out = [0] * n
    for i, (x, y) in enumerate(zip(xs, ys)):
        d = 1
        for j, xj in enumerate(xs):
            if j != i:
                d = d * (x - xj) % P
        w = y * pow(d, P - 2, P) % P                    # inverse(0) = 0
        carry = 0
        for e in range(n, 0, -1):
            carry = (Z[e] + x * carry) % P
            out[e - 1] = (out[e - 1] + w * carry) % P
    return out

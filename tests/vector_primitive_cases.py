"""Shapes, operands and expectations for the elementwise vector entries (tests/test_gpu_vector_primitives.py runs them on the GPU,
tests/test_vector_primitive_cases_cpu.py proves on the host that each shape is where it claims to be).

Every expectation here is Python integer arithmetic mod p = 1 + 407 * 2^119, or oracle/py_oracle.py's `fold` (fri.py:85 literally) for
the folds; never an entry of the library.  Operands are synth.synth_ints with the edge residues 0, 1, p - 1, 2^64, 2^119 + 1 at every
third place (the `_edges` pattern of tests/emu/poly_multiply_cases.py).  Nothing here touches a GPU.

The shapes are the smallest that reach the branch they are named for; the constants they are derived from are read out of
stark-anatomy_amd/csrc/core.hip, so a changed constant moves the shape with it."""
import functools
import os
import re

from oracle import py_oracle as po
import synth

P = po.P
G = po.GENERATOR
EDGES = (0, 1, P - 1, 1 << 64, (1 << 119) + 1)
NONZERO_EDGES = (2, 1, P - 1, 1 << 64, (1 << 119) + 1)          # for divisors: the same places, 2 where EDGES has 0
SENTINEL = b"\xff" * 16                                         # 2^128 - 1: not a residue, so no result can equal it
RANDOM = synth.synth_ints(77001, 3)                             # "a random residue", three of them
FACTORS = (("zero", 0), ("one", 1), ("minus one", P - 1), ("random", RANDOM[0]))      # weights, alphas, scales
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "stark-anatomy_amd", "csrc")


def constant(name, unit="core.hip"):
    with open(os.path.join(CSRC, unit)) as f:
        m = re.search(r"constexpr \w+ %s = (\d+);" % name, f.read())
    assert m, name
    return int(m.group(1))


def edges(values, shift=0, table=EDGES):
    return [table[(i + shift) % 5] if i % 3 == 0 else v for i, v in enumerate(values)]


def operands(seed, n, shift=0):
    """n residues of stream `seed`, an edge residue at every third place"""
    return edges(synth.synth_ints(seed, n), shift)


def divisors(seed, n, shift=0):
    vals = edges(synth.synth_ints(seed, n), shift, NONZERO_EDGES)
    return [v if v else 3 for v in vals]


pack = synth.pack_ints
unpack = synth.unpack_ints


def pow2ceil(x):
    c = 1
    while c < x:
        c <<= 1
    return c


def hi_entries(count):
    """what get_pow (core.hip) sizes and keys the high table of `count` powers by"""
    return pow2ceil((count >> 12) + 1)


# ---- 1. the two-level power table -----------------------------------------------------------------------------------------------

SCALE_SIZES = (1, 2, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
SCALE_FACTORS = FACTORS + (("root of order 8192", po.primitive_nth_root(8192)),)       # w^4096 = -1: the high table alternates 1, -1
SCALE_ORDER_RUN = (4097, 4095, 8193, 4096)                      # one factor, these sizes in this order and in the reverse order
SCALE_ORDER_FACTORS = (RANDOM[1], RANDOM[2])                    # factors no other case uses: the first call builds their tables


def powers(f, exponents):
    """{e: f^e} with 0^0 = 1"""
    return {e: pow(f, e, P) for e in set(exponents)}


@functools.lru_cache(maxsize=None)
def scale_input(n):
    return tuple(operands(4000 + n, n, n))


@functools.lru_cache(maxsize=None)
def scale_expected(n, f):
    out, fi = [], 1
    for v in scale_input(n):
        out.append(v * fi % P)
        fi = fi * f % P
    return out


# (rows, cols, row_len, col_base)
SLAB_SHAPES = ((1, 1, 1, 0), (12, 8, 32, 16), (300, 2, 64, 62), (3, 4, 2048, 2044), (5, 1, 4097, 4096), (2, 4096, 4096, 0))
SLAB_REFUSED = ((12, 3, 32, 16), (12, 8, 32, 25))               # cols = 3; col_base + cols = row_len + 1
SLAB_NOTHING = ((0, 8, 32, 16), (12, 0, 32, 16))
SLAB_FACTORS = FACTORS[1:] + (("root of order 8192", po.primitive_nth_root(8192)),)


def slab_exponents(shape):
    rows, cols, row_len, col_base = shape
    return [r * row_len + col_base + c for r in range(rows) for c in range(cols)]


@functools.lru_cache(maxsize=None)
def slab_input(shape):
    n = shape[0] * shape[1]
    return tuple(operands(4100 + 7 * shape[0] + shape[2], n, shape[3]))


def slab_expected(shape, f):
    ex = slab_exponents(shape)
    pw = powers(f, ex)
    return [v * pw[e] % P for v, e in zip(slab_input(shape), ex)]


# (rows, cols, row_base, col_base, order)
TWIDDLE_SHAPES = ((64, 32, 0, 32, 1 << 12), (1, 1, 0, 0, 2), (3, 2, 5, 6, 64), (8, 4, 1020, 1020, 1 << 21), (10, 8, 0, 0, 64))
TWIDDLE_REFUSED = (9, 8, 0, 1, 64)                              # largest exponent 8 * 8 = 64 = order
TWIDDLE_NOTHING = ((0, 8, 0, 0, 64), (0, 8, 0, 60, 64), (9, 0, 0, 1, 64), (0, 0, 0, 0, 64))
TWIDDLE_SCALES = (("no scale", None), ("scale one", 1), ("random scale", RANDOM[0]), ("scale minus one", P - 1))


def twiddle_exponents(shape):
    rows, cols, row_base, col_base, _ = shape
    return [(row_base + r) * (col_base + c) for r in range(rows) for c in range(cols)]


@functools.lru_cache(maxsize=None)
def twiddle_input(shape):
    return tuple(operands(4200 + shape[0] + shape[4], shape[0] * shape[1], shape[2]))


def twiddle_expected(shape, scale):
    root = po.primitive_nth_root(shape[4])
    ex = twiddle_exponents(shape)
    pw = powers(root, ex)
    s = 1 if scale is None else scale
    return [v * pw[e] % P * s % P for v, e in zip(twiddle_input(shape), ex)]


# (rows, cols, R, col_base); the codeword has N = rows * R entries, the slab the columns [col_base, col_base + cols) of its rows.
# The last shape is the one with an exponent from 8192 up: half of N = 2^15 is 2^14 powers of omega^-1
FOLD_SLAB_SHAPES = ((2, 1, 1, 0), (2, 4, 4, 0), (64, 16, 64, 32), (4, 8, 4096, 4088), (16, 1, 1024, 1023), (8, 2, 4096, 4094))
FOLD_SIZES = (2, 4)                                             # sc_fri_fold_dev below the suite's smallest (16)
ALPHAS = FACTORS


def fold_slab_exponents(shape):
    rows, cols, R, col_base = shape
    return [r * R + col_base + c for r in range(rows // 2) for c in range(cols)]


@functools.lru_cache(maxsize=None)
def codeword(N):
    return tuple(operands(4300 + N, N, N))


@functools.lru_cache(maxsize=None)
def fold_expected(N, alpha):
    """oracle/py_oracle.py's fold of the whole codeword, offset the field's generator, omega the primitive N-th root"""
    return tuple(po.fold(list(codeword(N)), alpha, G, po.primitive_nth_root(N)))


def slab_of(values, rows, cols, R, col_base):
    return [values[r * R + col_base + c] for r in range(rows) for c in range(cols)]


def fold_slab_input(shape):
    rows, cols, R, col_base = shape
    return slab_of(codeword(rows * R), rows, cols, R, col_base)


def fold_slab_expected(shape, alpha):
    rows, cols, R, col_base = shape
    return slab_of(fold_expected(rows * R, alpha), rows // 2, cols, R, col_base)


# ---- 2. pointwise product and quotient -----------------------------------------------------------------------------------------

MUL_SIZES = (1, 255, 256, 257)
# the edge operands of test_device_field_ops (tests/test_gpu_cabi.py), every pair of them
FIELD_EDGES = (0, 1, 2, P - 1, P - 2, (1 << 119), (1 << 119) - 1, (1 << 127), 407, (1 << 64) - 1, 1 << 64, (1 << 96) + 1, 0xCB800000 << 96, 511, 512)
EDGE_PAIRS = tuple((x, y) for x in FIELD_EDGES for y in FIELD_EDGES)


@functools.lru_cache(maxsize=None)
def mul_operands(n):
    """(a, b): all 225 pairs of edge residues, then random pairs, the first n of them (n = 1: see mul_single_pairs)"""
    a = [x for x, _ in EDGE_PAIRS] + synth.synth_ints(4400, 64)
    b = [y for _, y in EDGE_PAIRS] + synth.synth_ints(4401, 64)
    assert n <= len(a)
    return a[:n], b[:n]


def mul_single_pairs():
    """n = 1: every pair of EDGES and a random pair, one call each"""
    return [(x, y) for x in EDGES for y in EDGES] + [(RANDOM[0], RANDOM[1])]


DIV_KS = (16, 8)                                                # pointwise_div_kernel<K>: the default and STARKCORE_DIV_K=8
DIV_SIZES = {16: (1, 15, 16, 17, 4095, 4096, 4097, 8193), 8: (1, 7, 8, 9, 2047, 2048, 2049)}
DIV_ZERO_SIZES = {16: (17, 4095, 4096, 4097, 8193), 8: (2049,)}


def div_layout(n, K):
    """how pointwise_div_kernel<K> lays n quotients out: thread t of `nthreads` takes the elements t + k * nthreads, k < K, and a
    divisor of one where that is past the end.  Returns (workgroups, threads with K real slots, threads with some but not K,
    padding slots, workgroups with no real slot)"""
    threads = (n + K - 1) // K
    blocks = (threads + 255) // 256
    nthreads = 256 * blocks
    real = [len(range(t, n, nthreads)[:K]) for t in range(nthreads)]
    assert sum(real) == n
    idle = sum(1 for b in range(blocks) if not any(real[256 * b:256 * b + 256]))
    return blocks, sum(1 for r in real if r == K), sum(1 for r in real if 0 < r < K), K * nthreads - n, idle


def div_companions(n, K, i):
    """the elements that share a thread, and so one inversion, with element i"""
    threads = (n + K - 1) // K
    nthreads = 256 * ((threads + 255) // 256)
    return set(range(i % nthreads, n, nthreads))


@functools.lru_cache(maxsize=None)
def div_operands(n):
    return tuple(operands(4500 + n, n, n)), tuple(divisors(4501 + n, n, n + 1))


@functools.lru_cache(maxsize=None)
def div_expected(n):
    a, b = div_operands(n)
    return [x * pow(y, -1, P) % P for x, y in zip(a, b)]


def div_zero_places(n):
    return (0, n // 2, n - 1)


# ---- 3. axpy with a shift ---------------------------------------------------------------------------------------------------------

# (n_acc, n_src, shift)
AXPY_SHAPES = ((1, 1, 0), (300, 100, 0), (300, 100, 57), (300, 100, 200), (257, 256, 1), (1024, 255, 769))
AXPY_REFUSED = ((300, 100, 201, 1), (300, 2, (1 << 64) - 1, 1), (300, 100, 57, P))          # (n_acc, n_src, shift, weight)
WEIGHTS = FACTORS


@functools.lru_cache(maxsize=None)
def axpy_operands(shape):
    """(accumulator, source): the accumulator is p - 1 at every third place and edge residues at the others, so that sums wrap"""
    n_acc, n_src, shift = shape
    acc = [P - 1 if i % 3 == 0 else EDGES[i % 5] if i % 3 == 1 else v for i, v in enumerate(synth.synth_ints(4600 + n_acc, n_acc))]
    return tuple(acc), tuple(operands(4601 + n_src, n_src, shift))


def axpy_expected(shape, w):
    n_acc, n_src, shift = shape
    acc, src = axpy_operands(shape)
    out = list(acc)
    for j, x in enumerate(src):
        out[shift + j] = (out[shift + j] + w * x) % P
    return out


# ---- 4. degrees --------------------------------------------------------------------------------------------------------------------

DEGREE_PER_THREAD = constant("DEGREE_PER_THREAD")
DEGREE_MAX_BLOCKS = constant("DEGREE_MAX_BLOCKS")
DEGREE_SLOTS = constant("DEGREE_SLOTS")
DEGREE_COLS_PER_LAUNCH = constant("DEGREE_COLS_PER_LAUNCH")
DEGREE_WG = 256 * DEGREE_PER_THREAD                             # entries a workgroup looks at per step
DEGREE_STEP = DEGREE_MAX_BLOCKS * DEGREE_WG                     # entries the capped grid looks at per step
DEGREE_TOP = 1 << 16                                            # sc_vec_degree_dev looks at the top 2^16 entries first
DEGREE_COL_PARTS = 64                                           # sc_vec_degree_columns_dev: at most 64 workgroups per column
NONZERO = (1, P - 1, 1 << 64, (1 << 119) + 1)                   # (2^64 has a zero low limb, 1 a zero high limb)

DEGREE_SMALL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def degree_small_cases():
    """(n, leading index or -1, decoy index or None): the leading entry at each place of the list that is below n, a decoy below it"""
    out = []
    for n in DEGREE_SMALL_SIZES:
        out.append((n, -1, None))
        for lead in sorted({i for i in (0, 63, 64, 255, 256, 1023, n - 1) if i < n}):
            out.append((n, lead, lead // 2 if lead else None))
    return out


DEGREE_STRIDED_SCANNED = DEGREE_STEP + DEGREE_WG + 5            # what the second launch scans: one step, one workgroup and five entries
DEGREE_STRIDED_N = DEGREE_TOP + DEGREE_STRIDED_SCANNED          # ... under a top window that is all zero


def degree_workgroup(i):
    """(workgroup, step) of the capped grid that looks at entry i"""
    return (i % DEGREE_STEP) // DEGREE_WG, i // DEGREE_STEP


def degree_strided_cases():
    """(leading index, decoys in a workgroup that shares the leader's result word, other decoys), every decoy below the leader"""
    out = []
    for lead in (3, DEGREE_STEP - 1, DEGREE_STEP, DEGREE_STEP + 3, DEGREE_STRIDED_SCANNED - 1):
        b, _ = degree_workgroup(lead)
        same = []
        for wg in (b + DEGREE_SLOTS, b - DEGREE_SLOTS, b):          # a first-step entry of workgroup b + 8, b - 8, or b itself
            i = wg * DEGREE_WG + 1
            if 0 <= wg < DEGREE_MAX_BLOCKS and i < lead:
                same.append(i)
        other = [DEGREE_STEP - 1] if DEGREE_STEP - 1 < lead else []
        out.append((lead, same[:2], other))
    return out


DEGREE_COLS_STRIDED = dict(n=DEGREE_COL_PARTS * DEGREE_WG + DEGREE_WG + 5, gap=3, cols=3)
# column -> (leading index, decoy): part 0 in its second step; part 63 in its first; a column of zeros
DEGREE_COLS_STRIDED_LEADS = ((DEGREE_COL_PARTS * DEGREE_WG + 3, 5), (DEGREE_COL_PARTS * DEGREE_WG - 1, 7), (-1, None))
DEGREE_COLS_MANY = dict(n=3, gap=1, cols=DEGREE_COLS_PER_LAUNCH + 3)


def degree_cols_many_expected():
    return [c % 4 - 1 for c in range(DEGREE_COLS_MANY["cols"])]


def degree_cols_many_values():
    """[cols][ld = 4]: column c is non-zero up to its leading index c % 4 - 1 and zero above; the fourth entry is junk between the columns"""
    out = []
    for c in range(DEGREE_COLS_MANY["cols"]):
        lead = c % 4 - 1
        out += [NONZERO[(c + i) % 4] if i <= lead else 0 for i in range(3)] + [NONZERO[c % 4]]
    return out


# ---- 5. multivariate evaluation ---------------------------------------------------------------------------------------------------

SMALL_PAYLOAD = 4 * 2048                                        # upload_small (core.hip): at most four kernel-argument payloads of 2048 bytes
MPOLY_ABSENT = 0xFFFFFFFF


def mpoly_values(seed, nvars, n):
    return [operands(seed + j, n, j) for j in range(nvars)]


def mpoly_expected(vals, n, terms, src=None, rot=None):
    """sum_t coef_t prod_j value(j, i)^e_tj; with src / rot variable j at point i is variable src[j] at point (i + rot[j]) mod n"""
    out = []
    for i in range(n):
        acc = 0
        for exps, coef in terms:
            t = coef
            for j, e in enumerate(exps):
                if e:
                    v = vals[j][i] if src is None else vals[src[j]][(i + rot[j]) % n]
                    t = t * pow(v, e, P) % P
            acc = (acc + t) % P
        out.append(acc)
    return out


def mpoly_terms_basic(nvars):
    """exponent 255 on one variable, exponent 0 everywhere, exponent 1 on every variable"""
    return [((255,) + (0,) * (nvars - 1), RANDOM[0]), ((0,) * nvars, P - 1), ((1,) * nvars, RANDOM[1])]


def mpoly_terms_sparse(nterms, nvars, seed):
    """exponents 0..2, at most two variables per term (the payload's size is what matters, not the work)"""
    coefs = operands(seed, nterms, 1)
    out = []
    for t in range(nterms):
        e = [0] * nvars
        e[t % nvars] = 1 + t % 2
        e[(7 * t + 3) % nvars] = t % 3
        out.append((tuple(e), coefs[t]))
    return out


# name -> (nvars, n, terms): without turned variables
@functools.lru_cache(maxsize=None)
def mpoly_cases():
    cases = {}
    for n in (1, 255, 256, 257):
        cases["three variables, %d points" % n] = (3, n, mpoly_terms_basic(3))
    cases["one variable"] = (1, 257, mpoly_terms_basic(1) + [((2,), 5)])
    cases["255 variables of 2 points"] = (255, 2, mpoly_terms_basic(255) + [((0,) * 254 + (255,), 7), ((3,) + (0,) * 253 + (2,), P - 2)])
    cases["no term"] = (3, 257, [])
    cases["512 terms: coefficients at the limit"] = (1, 257, mpoly_terms_sparse(512, 1, 4700))
    cases["513 terms: coefficients over the limit"] = (1, 257, mpoly_terms_sparse(513, 1, 4701))
    cases["482 terms of 17 variables: exponents over the limit"] = (17, 257, mpoly_terms_sparse(482, 17, 4702))
    return cases


def mpoly_payload(nvars, terms):
    """(coefficient bytes, exponent bytes) of a call"""
    return 16 * max(len(terms), 1), len(terms) * nvars


# name -> (n, turns of the two turned variables): five variables -- 0 and 1 stored, 2 = variable 0 turned, 3 = variable 1 turned, 4 absent
MPOLY_ROT_CASES = {"n = 1": (1, (0, 5)), "n = 2": (2, (1, 5)), "n = 256, turns 3 and n - 1": (256, (3, 255)), "n = 256, turns n + 3 and 2 n - 1": (256, (259, 511))}          # the last two must agree: a turn counts mod n
MPOLY_ROT_SRC = (0, 1, 0, 1, MPOLY_ABSENT)
MPOLY_ROT_TERMS = (((1, 0, 2, 0, 0), 7), ((0, 3, 0, 1, 0), P - 2), ((2, 1, 1, 1, 0), RANDOM[2]), ((0, 0, 0, 0, 0), 11), ((0, 0, 255, 0, 0), P - 1))


def mpoly_rot_expected(n, turns):
    stored = mpoly_values(4800 + n, 2, n)
    src = (0, 1, 0, 1, 0)
    rot = (0, 0, turns[0], turns[1], 0)
    return stored, mpoly_expected(stored, n, MPOLY_ROT_TERMS, src, rot)


# ---- 6. gather ---------------------------------------------------------------------------------------------------------------------

GATHER_N = 300
GATHER_COUNTS = (0, 1, 256, 257, 1000)


def gather_indices(k):
    """k indices below GATHER_N with repeats, the last index of the vector among them"""
    idx = [(GATHER_N - 1 - 37 * i * i) % GATHER_N for i in range(k)]
    assert not k or idx[0] == GATHER_N - 1
    return idx

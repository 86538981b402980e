"""The columns-form entries (include/starkcore.h: sc_pointwise_div_columns_later_dev, sc_coset_divide_columns_later_dev,
sc_combine_columns_dev) called directly: quotients against the C oracle's restatement of the reference (oracle/py_oracle.py) and
byte for byte against the single-column entries on the same inputs, the verdict words against plain Python integers; one pinned slot
per call whatever the number of columns; nothing enqueued when no slot is free; and the Python functions of ntt.py over them."""
import ctypes
import random

import pytest

from oracle import py_oracle as po
import synth

pytestmark = pytest.mark.gpu
C = po.C
P = po.P
G = po.GENERATOR
SC_ERR_BAD_ARG = -6                  # include/starkcore.h
SENTINEL = b"\xff" * 16              # not a residue: a kernel that read it, or wrote over it, shows


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    starkcore.set_tuning("small_divisor_direct", 1)
    starkcore.set_tuning("div_cols_chunk", 0)
    starkcore.set_tuning("div_cols_launch_log", 26)


def _ints(buf):
    return synth.unpack_ints(buf)


def _words(later):
    import starkcore
    w = (ctypes.c_int64 * 8)()
    starkcore._check(starkcore.lib().sc_later_wait(later, w))
    return list(w)


def _nonzero(n, seed):
    return synth.pack_ints([v or 1 for v in synth.synth_ints(seed, n)])


def _matrix(rows, ld):
    """packed rows (bytes, any lengths up to ld elements) as a [len(rows)][ld] matrix with sentinels in the gaps"""
    return b"".join(row + SENTINEL * (ld - len(row) // 16) for row in rows)


def _row(raw, c, ld, n):
    return raw[16 * ld * c:16 * (ld * c + n)]


class Drained:
    """Every pinned slot taken, by 1-element out-of-place deferred divisions, until sc_pointwise_div_later_dev says
    SC_ERR_UNSUPPORTED.  Does not assume the pool's size: other live objects may hold slots.  `release()` waits for all."""

    def __init__(self, sc):
        self.sc = sc
        self.a, self.b, self.out = sc.DeviceVector.from_ints([6]), sc.DeviceVector.from_ints([3]), sc.DeviceVector(1)
        self.handles = []
        lib = sc.lib()
        while True:
            h = ctypes.c_void_p()
            rc = lib.sc_pointwise_div_later_dev(self.a.ptr, self.b.ptr, self.out.ptr, 1, ctypes.byref(h), None)
            if rc == sc.SC_ERR_UNSUPPORTED:
                break
            sc._check(rc)
            self.handles.append(sc.Later(h))
            assert len(self.handles) <= 1 << 16, "the slot pool never ran out"

    def __len__(self):
        return len(self.handles)

    def release(self):
        for h in self.handles:
            assert h.wait() == (False, False)
        self.handles = []
        assert _ints(self.out.to_bytes()) == [2]


def free_slots(sc):
    d = Drained(sc)
    n = len(d)
    d.release()
    return n


# ---------------------------------------------------------------- pointwise division

def _div_columns_later(sc, a, ld_a, b, ld_b, out, ld_out, n, cols, stream=None):
    """the call only enqueued on `stream` (a ctypes.c_void_p, None: the library's): the handle, to be waited for with _words"""
    h = ctypes.c_void_p()
    sc._check(sc.lib().sc_pointwise_div_columns_later_dev(a.ptr, ld_a, b.ptr, ld_b, out.ptr, ld_out, n, cols, ctypes.byref(h), stream))
    return h


def _div_columns(sc, a, ld_a, b, ld_b, out, ld_out, n, cols):
    return _words(_div_columns_later(sc, a, ld_a, b, ld_b, out, ld_out, n, cols))


@pytest.mark.parametrize("n,cols", [(1, 1), (17, 3), (4097, 5), (255, 300), ((1 << 16) + 1, 2)])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_column"])
def test_pointwise_div_columns_matches_the_oracle(sc, n, cols, shared):
    """every column against the oracle's pointwise division and against sc_pointwise_div_later_dev, out of place with strides wider
    than a column (the gaps stay as they were) and in place, at forced chunk sizes that the columns straddle and at the default"""
    a_rows = [synth.synth_packed(100 + 7 * c + n % 89, n).tobytes() for c in range(cols)]
    b_rows = [_nonzero(n, 300 + 5 * c + n % 83) for c in range(1 if shared else cols)]
    want = [C.pointwise_div(a_rows[c], b_rows[0 if shared else c], n) for c in range(cols)]
    single = sc.DeviceVector(n)
    h = ctypes.c_void_p()
    da, db = sc.DeviceVector.from_bytes(a_rows[-1]), sc.DeviceVector.from_bytes(b_rows[-1])
    sc._check(sc.lib().sc_pointwise_div_later_dev(da.ptr, db.ptr, single.ptr, n, ctypes.byref(h), None))
    assert _words(h)[:2] == [0, -1] and single.to_bytes() == want[-1]
    ld_a, ld_b, ld_out = n + 3, n + 1, n + 2
    for chunk in (0, 1, 2, 3):
        sc.set_tuning("div_cols_chunk", chunk)
        a = sc.DeviceVector.from_bytes(_matrix(a_rows, ld_a))
        b = sc.DeviceVector.from_bytes(_matrix(b_rows, ld_b))
        out = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out))
        assert _div_columns(sc, a, ld_a, b, 0 if shared else ld_b, out, ld_out, n, cols)[:4] == [0, -1, -1, 0]
        assert out.to_bytes() == _matrix(want, ld_out), chunk
        assert a.to_bytes() == _matrix(a_rows, ld_a)
        assert _div_columns(sc, a, ld_a, b, 0 if shared else ld_b, a, ld_a, n, cols)[:4] == [0, -1, -1, 0]      # in place
        assert a.to_bytes() == _matrix(want, ld_a), chunk
    sc.set_tuning("div_cols_chunk", 0)


def test_pointwise_div_columns_names_the_lowest_column_with_a_zero_divisor(sc):
    n, cols = 4097, 7
    a_rows = [synth.synth_packed(500 + c, n).tobytes() for c in range(cols)]
    clean = [_nonzero(n, 600 + c) for c in range(cols)]
    a = sc.DeviceVector.from_bytes(b"".join(a_rows))
    for bad, where in (((0,), 0), ((3,), n - 1), ((cols - 1,), 4096), ((5, 2), 77)):
        b_rows = [bytearray(r) for r in clean]
        for c in bad:
            b_rows[c][16 * where:16 * where + 16] = bytes(16)
        b = sc.DeviceVector.from_bytes(b"".join(map(bytes, b_rows)))
        out = sc.DeviceVector(cols * n)
        assert _div_columns(sc, a, n, b, n, out, n, n, cols)[:4] == [1, -1, min(bad), len(bad)]
        got = out.to_bytes()
        for c in range(cols):
            if c not in bad:
                assert _row(got, c, n, n) == C.pointwise_div(a_rows[c], clean[c], n)
    shared = bytearray(clean[0])
    shared[16 * 9:16 * 10] = bytes(16)
    b = sc.DeviceVector.from_bytes(bytes(shared))
    assert _div_columns(sc, a, n, b, 0, sc.DeviceVector(cols * n), n, n, cols)[:4] == [1, -1, 0, cols]      # a shared zero marks every column


# ---------------------------------------------------------------- coset division

def _interpolant(num, d, root, order):
    """ntt.py:159-176 with the oracle's primitives: all `order` coefficients of the unscaled interpolant of the value quotient"""
    ca = C.coset_evaluate(synth.pack_ints(num), len(num), G, root, order)
    cb = C.coset_evaluate(synth.pack_ints(d), len(d), G, root, order)
    return C.scale(C.intt(root, C.pointwise_div(ca, cb, order), order), order, pow(G, -1, P))


def _coset_columns_later(sc, a, na, ld_a, b, nb, ld_b, cols, root, order, out, n_out, ld_out, stream=None):
    """the call only enqueued on `stream` (a ctypes.c_void_p, None: the library's): the handle, to be waited for with _words"""
    h = ctypes.c_void_p()
    sc._check(sc.lib().sc_coset_divide_columns_later_dev(a.ptr, na, ld_a, b.ptr, nb, ld_b, cols, sc.fe_bytes(G), sc.fe_bytes(root), order, out.ptr,
                                                         (ctypes.c_uint64 * cols)(*n_out), ld_out, ctypes.byref(h), stream))
    return h


def _coset_columns(sc, a, na, ld_a, b, nb, ld_b, cols, root, order, out, n_out, ld_out):
    return _words(_coset_columns_later(sc, a, na, ld_a, b, nb, ld_b, cols, root, order, out, n_out, ld_out))


def _coset_single(sc, num, d, root, order, n_out):
    """sc_coset_divide_later_dev on one column: (quotient bytes, words)"""
    da, db, out = sc.DeviceVector.from_ints(num), sc.DeviceVector.from_ints(d), sc.DeviceVector(max(n_out, 1))
    h = ctypes.c_void_p()
    sc._check(sc.lib().sc_coset_divide_later_dev(da.ptr, len(num), db.ptr, len(d), sc.fe_bytes(G), sc.fe_bytes(root), order, out.ptr, n_out, ctypes.byref(h), None))
    words = _words(h)
    return out.to_bytes(0, n_out), words


def _verdict_of(per_column):
    """the four words the columns form must report, from each column's own (zero flag, remainder index)"""
    failing = [c for c, (zero, rem) in enumerate(per_column) if zero or rem >= 0]
    if not failing:
        return [0, -1, -1, 0]
    zero, rem = per_column[failing[0]]
    return [zero, rem, failing[0], len(failing)]


def _degree_of(packed):
    """po.degree of packed coefficients (the zeros above the last non-zero one are not unpacked: there are two million of them)"""
    top = packed.rstrip(b"\0")
    return po.degree(_ints(top + bytes(-len(top) % 16)))


def _coset_operands(sc, columns, nb, shared, n_out):
    """(a, na, ld_a, b, ld_out): the numerators as rows of one device matrix (zero-padded to the longest, sentinels behind each), the
    divisors zero-padded to nb (the first one alone where shared), and the pitch of an output that takes the longest quotient"""
    na = max(len(num) for num, _, _ in columns)
    ld_a, ld_out = na + 2, max(max(n_out), 1) + 1
    a = sc.DeviceVector.from_bytes(_matrix([synth.pack_ints(num + [0] * (na - len(num))) for num, _, _ in columns], ld_a))
    d_rows = [synth.pack_ints(d + [0] * (nb - len(d))) for _, d, _ in columns]
    b = sc.DeviceVector.from_bytes(d_rows[0] if shared else b"".join(d_rows))
    return a, na, ld_a, b, ld_out


def _check_coset_columns(sc, columns, nb, shared, root, order, n_out):
    """columns: [(numerator ints, divisor ints, expected interpolant bytes or None to take it from the oracle)].  The columns form on
    the numerators as rows of one matrix (sentinels behind each) and the divisors zero-padded to nb, under both settings of
    small_divisor_direct: quotients against the expectation and against the single-column entry, words against both."""
    cols = len(columns)
    a, na, ld_a, b, ld_out = _coset_operands(sc, columns, nb, shared, n_out)
    fulls = [full if full is not None else _interpolant(num, d, root, order) for num, d, full in columns]
    want_words = [(0, _degree_of(full[16 * k:])) for full, k in zip(fulls, n_out)]
    for direct in (1, 0):
        sc.set_tuning("small_divisor_direct", direct)
        out = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out))
        words = _coset_columns(sc, a, na, ld_a, b, nb, 0 if shared else nb, cols, root, order, out, n_out, ld_out)
        got = out.to_bytes()
        assert got == _matrix([full[:16 * k] for full, k in zip(fulls, n_out)], ld_out), (order, nb, direct)
        assert words[:4] == _verdict_of(want_words), (order, nb, direct, words[:4])
        singles = [_coset_single(sc, num, d, root, order, k) for (num, d, _), k in zip(columns, n_out)]
        assert [_row(got, c, ld_out, n_out[c]) for c in range(cols)] == [q for q, _ in singles]
        assert words[:4] == _verdict_of([(w[0], w[1]) for _, w in singles])
    sc.set_tuning("small_divisor_direct", 1)
    assert a.to_bytes() == _matrix([synth.pack_ints(num + [0] * (na - len(num))) for num, _, _ in columns], ld_a)


@pytest.mark.parametrize("nb", [1, 2, 8, 9])
@pytest.mark.parametrize("order", [64, 1 << 12, 1 << 21])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_column"])
def test_coset_divide_columns_matches_the_oracle(sc, order, nb, shared):
    """three exact columns at the smallest order of one, two and three passes: column 0 keeps all `order` coefficients, column 1 its
    quotient, column 2 is cut short (the remainder index is then the known top of the quotient); divisors of nb coefficients (the
    last column's one shorter and zero-padded where each has its own).  At 64 and 2^12 the expectation is the oracle's interpolant
    (ntt.py:159-176 with the oracle's primitives).  At 2^21 the oracle's transforms would take minutes, so there the expectation is
    the quotient the numerators were built from -- which is what an exact division's interpolant is -- and the single-column entry
    on the same inputs; the quotients stay short there, the transforms are of `order` points whatever the operands' lengths."""
    assert [sc.lib().sc_ntt_num_passes(o) for o in (32, 64, 1 << 11, 1 << 12, 1 << 20, 1 << 21)] == [1, 1, 1, 2, 2, 3]
    lq = min(order // 2 - 3, 3000)
    root = po.primitive_nth_root(order)
    columns = []
    for c in range(3):
        ld = nb - 1 if (c == 2 and not shared and nb > 1) else nb
        q = synth.synth_ints(1000 + order % 97 + c, lq)
        d = synth.synth_ints(1100 + nb + (0 if shared else c), ld)
        q[-1], d[-1] = q[-1] or 1, d[-1] or 1
        built = synth.pack_ints(q) + bytes(16 * (order - lq))
        if order <= 1 << 12:
            assert _interpolant(po.schoolbook_mul(q, d), d, root, order) == built
        columns.append((po.schoolbook_mul(q, d), d, None if order <= 1 << 12 else built))
    _check_coset_columns(sc, columns, nb, shared, root, order, [order, lq, lq - 5])


@pytest.mark.parametrize("order,nb", [(64, 3), (64, 9), (1 << 12, 9)])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_column"])
def test_coset_divide_columns_in_chunks(sc, order, nb, shared):
    """five columns with the launch limit lowered to two columns' worth of values ("div_cols_launch_log"): the entry works through
    chunks of 2, 2 and 1 columns that reuse its value matrices and report into the same per-column words.  Every column has its own
    quotient length; column 3, in the second chunk, leaves a remainder (its expectation is the oracle's interpolant), so the verdict
    must name it: a chunk that wrote another chunk's words, lengths or output rows shows in the bytes or in the words."""
    cols, lq = 5, order // 2 - nb
    root = po.primitive_nth_root(order)
    columns = []
    for c in range(cols):
        q = synth.synth_ints(1700 + order % 97 + c, lq - c)
        d = synth.synth_ints(1800 + nb + (0 if shared else c), nb)
        q[-1], d[-1] = q[-1] or 1, d[-1] or 1
        lhs = po.schoolbook_mul(q, d)
        if c == 3:
            lhs = [(v + 1) % P for v in lhs]
        columns.append((lhs, d, None))
    assert sc.lib().sc_set_tuning(b"div_cols_launch_log", order.bit_length()) == 0            # 2 * order values per set of launches
    try:
        _check_coset_columns(sc, columns, nb, shared, root, order, [lq - c for c in range(cols)])
    finally:
        sc.set_tuning("div_cols_launch_log", 26)


@pytest.mark.parametrize("order", [64, 1 << 12])
@pytest.mark.parametrize("bad", [0, 1, 2])
def test_coset_divide_columns_one_inexact_column(sc, order, bad):
    """one numerator that its divisor does not divide among exact ones, at column 0, the middle and the last: its quotient bytes and
    its remainder index are the oracle's, and the verdict names it"""
    lq, nb = order // 2, 3
    root = po.primitive_nth_root(order)
    columns = []
    for c in range(3):
        q, d = synth.synth_ints(1300 + c, lq), synth.synth_ints(1400 + c, nb)
        q[-1], d[-1] = q[-1] or 1, d[-1] or 1
        lhs = po.schoolbook_mul(q, d)
        if c == bad:
            columns.append(([(v + 1) % P for v in lhs], d, None))
        else:
            columns.append((lhs, d, synth.pack_ints(q) + bytes(16 * (order - lq))))
    _check_coset_columns(sc, columns, nb, False, root, order, [lq] * 3)


@pytest.mark.parametrize("order,k", [(64, 3), (1 << 12, 4095)])
def test_coset_divide_columns_flags_a_divisor_that_vanishes_on_the_coset(sc, order, k):
    """X - g * w^k in the middle column only (the outer columns divide exactly by X + 5), then as the shared divisor"""
    root = po.primitive_nth_root(order)
    z = G * pow(root, k, P) % P
    vanishing, harmless = [(P - z) % P, 1], [5, 1]
    na = order // 2
    nums = [po.schoolbook_mul(synth.synth_ints(1500 + c, na - 2) + [1], harmless) for c in range(3)]
    a = sc.DeviceVector.from_ints([v for num in nums for v in num])
    for direct in (1, 0):
        sc.set_tuning("small_divisor_direct", direct)
        b = sc.DeviceVector.from_ints(harmless + vanishing + harmless)
        out = sc.DeviceVector(3 * na)
        words = _coset_columns(sc, a, na, na, b, 2, 2, 3, root, order, out, [na - 1] * 3, na)
        assert words[0] == 1 and words[2:4] == [1, 1], (order, direct, words[:4])
        b = sc.DeviceVector.from_ints(vanishing)
        words = _coset_columns(sc, a, na, na, b, 2, 0, 3, root, order, out, [na - 1] * 3, na)
        assert words[0] == 1 and words[2] == 0 and words[3] == 3, (order, direct, words[:4])
    sc.set_tuning("small_divisor_direct", 1)


# ---------------------------------------------------------------- slots

def test_a_division_of_300_columns_holds_one_slot(sc):
    order, cols, lq = 64, 300, 20
    root = po.primitive_nth_root(order)
    d = [3, 0, 1]
    qs = [synth.synth_ints(1600 + c, lq) for c in range(cols)]
    for q in qs:
        q[-1] = q[-1] or 1
    lhs = [po.schoolbook_mul(q, d) for q in qs]
    na = lq + 2
    a, b, out = sc.DeviceVector.from_ints([v for row in lhs for v in row]), sc.DeviceVector.from_ints(d), sc.DeviceVector(cols * lq)
    before = free_slots(sc)
    assert before >= 2
    h = ctypes.c_void_p()
    sc._check(sc.lib().sc_coset_divide_columns_later_dev(a.ptr, na, na, b.ptr, 3, 0, cols, sc.fe_bytes(G), sc.fe_bytes(root), order, out.ptr,
                                                         (ctypes.c_uint64 * cols)(*([lq] * cols)), lq, ctypes.byref(h), None))
    drained = Drained(sc)
    held = before - len(drained)
    drained.release()
    assert held == 1
    assert _words(h)[:4] == [0, -1, -1, 0]
    assert out.to_bytes() == b"".join(synth.pack_ints(q) for q in qs)
    h = ctypes.c_void_p()
    sc._check(sc.lib().sc_pointwise_div_columns_later_dev(out.ptr, lq, b.ptr + 32, 0, out.ptr, lq, 1, cols, ctypes.byref(h), None))
    drained = Drained(sc)
    held = before - len(drained)
    drained.release()
    assert held == 1
    assert _words(h)[:4] == [0, -1, -1, 0]
    assert free_slots(sc) == before


def test_no_slot_free_enqueues_nothing(sc):
    """with every slot taken both deferred forms say SC_ERR_UNSUPPORTED and leave an in-place numerator and the output as they were"""
    order, cols, na = 64, 3, 30
    root = po.primitive_nth_root(order)
    a_raw = synth.synth_packed(1700, cols * na).tobytes()
    b_raw = _nonzero(cols * na, 1701)
    a, b = sc.DeviceVector.from_bytes(a_raw), sc.DeviceVector.from_bytes(b_raw)
    out = sc.DeviceVector.from_bytes(SENTINEL * (cols * na))
    sc.synchronize()
    drained = Drained(sc)
    try:
        h = ctypes.c_void_p()
        lib = sc.lib()
        assert lib.sc_pointwise_div_columns_later_dev(a.ptr, na, b.ptr, na, a.ptr, na, na, cols, ctypes.byref(h), None) == sc.SC_ERR_UNSUPPORTED
        assert lib.sc_pointwise_div_columns_later_dev(a.ptr, na, b.ptr, 0, out.ptr, na, na, cols, ctypes.byref(h), None) == sc.SC_ERR_UNSUPPORTED
        assert lib.sc_coset_divide_columns_later_dev(a.ptr, na, na, b.ptr, 2, 2, cols, sc.fe_bytes(G), sc.fe_bytes(root), order, a.ptr,
                                                     (ctypes.c_uint64 * cols)(*([na - 1] * cols)), na, ctypes.byref(h), None) == sc.SC_ERR_UNSUPPORTED
        assert lib.sc_coset_divide_columns_later_dev(a.ptr, na, na, b.ptr, 2, 0, cols, sc.fe_bytes(G), sc.fe_bytes(root), order, out.ptr,
                                                     (ctypes.c_uint64 * cols)(*([na - 1] * cols)), na, ctypes.byref(h), None) == sc.SC_ERR_UNSUPPORTED
        sc.synchronize()
        assert a.to_bytes() == a_raw and b.to_bytes() == b_raw and out.to_bytes() == SENTINEL * (cols * na)
    finally:
        drained.release()


# ---------------------------------------------------------------- the combination

def _combine(sc, terms, weights, cols, n_out, ld_out, out):
    table = (sc.CombineTerm * len(terms))(*[sc.CombineTerm(src.ptr if src is not None else None, ld, n, shift) for src, ld, n, shift in terms])
    return sc.lib().sc_combine_columns_dev(table, len(terms), synth.pack_ints([w for row in weights for w in row]), cols, out.ptr, n_out, ld_out, None)


@pytest.mark.parametrize("cols", [1, 3])
@pytest.mark.parametrize("nterms", [1, 5, 300])
def test_combine_columns_matches_python_sums(sc, cols, nterms):
    """against plain integers and against the chain of sc_axpy_shift_dev calls over a zeroed accumulator; few terms travel as kernel
    arguments, 300 by copy; [300, 400) is covered by no term and must come out zero"""
    rng = random.Random(nterms + cols)
    n_out, ld_out = 700, 703
    shapes = [(300, 0), (1, 699), (0, 5), (300, 400), (120, 450)]
    while len(shapes) < nterms:
        n = rng.randrange(0, 100)
        shapes.append((n, rng.randrange(0, 300 - n)) if len(shapes) % 2 else (n, rng.randrange(400, 700 - n)))
    shapes = shapes[:nterms]
    sources, terms = [], []
    for k, (n, shift) in enumerate(shapes):
        ld = n + k % 3
        rows = [synth.synth_ints(1800 + 3 * k + c, n) for c in range(cols)]
        vec = sc.DeviceVector.from_bytes(_matrix([synth.pack_ints(r) for r in rows], ld)) if n else None
        sources.append(rows)
        terms.append((vec, ld, n, shift))
    weights = [[rng.choice([0, 1, P - 1, rng.randrange(P)]) for _ in shapes] for _ in range(cols)]
    weights[0][:3] = [0, 1, P - 1][:nterms]
    out = sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out))
    sc._check(_combine(sc, terms, weights, cols, n_out, ld_out, out))
    got = out.to_bytes()
    for c in range(cols):
        want = [0] * n_out
        acc = sc.DeviceVector.zeros(n_out)
        for t, ((n, shift), rows) in enumerate(zip(shapes, sources)):
            for j in range(n):
                want[shift + j] = (want[shift + j] + weights[c][t] * rows[c][j]) % P
            if n and nterms <= 5:
                acc.axpy_shift(sc.DeviceVector.from_ints(rows[c]), shift, weights[c][t])
        assert _row(got, c, ld_out, n_out) == synth.pack_ints(want), (cols, nterms, c)
        assert got[16 * (ld_out * c + n_out):16 * ld_out * (c + 1)] == SENTINEL * (ld_out - n_out)
        if nterms <= 5:
            assert acc.to_bytes() == synth.pack_ints(want)
        if nterms > 1:
            assert want[300:400] == [0] * 100


def test_combine_columns_refuses_bad_arguments(sc):
    src, out = sc.DeviceVector.from_ints([1, 2, 3, 4]), sc.DeviceVector.from_bytes(SENTINEL * 8)
    ok = [(src, 4, 4, 0)]
    assert _combine(sc, ok, [[1]], 1, 8, 8, out) == 0
    assert _ints(out.to_bytes()) == [1, 2, 3, 4, 0, 0, 0, 0]
    before = out.to_bytes()
    assert _combine(sc, [(src, 4, 4, 5)], [[1]], 1, 8, 8, out) == SC_ERR_BAD_ARG           # shift + n > n_out
    assert _combine(sc, ok, [[P]], 1, 8, 8, out) == SC_ERR_BAD_ARG                          # weight not canonical
    assert _combine(sc, [(out, 8, 4, 0)], [[1]], 1, 8, 8, out) == SC_ERR_BAD_ARG           # the output is a source
    two = sc.DeviceVector.from_ints([1, 2, 3, 4, 5, 6, 7, 8])
    h = ctypes.c_void_p()                                                                   # in place with another stride: refused
    assert sc.lib().sc_pointwise_div_columns_later_dev(two.ptr, 4, src.ptr, 0, two.ptr, 3, 3, 2, ctypes.byref(h), None) == SC_ERR_BAD_ARG
    assert _ints(two.to_bytes()) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert _combine(sc, ok, [[1]], 0, 8, 8, out) == 0 and _combine(sc, ok, [[1]], 1, 0, 8, out) == 0
    assert out.to_bytes() == before


# ---------------------------------------------------------------- the Python functions

@pytest.fixture(scope="module")
def field():
    from algebra import Field
    return Field.main()


def _poly(field, ints):
    from algebra import FieldElement
    from univariate import Polynomial
    return Polynomial([FieldElement(v, field) for v in ints])


def test_fast_coset_divide_columns_equals_the_loop(sc, field):
    import ntt
    order = 1 << 10
    root, g = field.primitive_nth_root(order), field.generator()
    divisors = [_poly(field, [3, 1]), _poly(field, [7, 0, 1]), _poly(field, [2, 5, 0, 1])]
    quotients = [_poly(field, synth.synth_ints(1900 + c, 400 - c)) for c in range(3)]
    lhs = [q * d for q, d in zip(quotients, divisors)]                       # one degree (402), three divisor degrees
    assert len({p.degree() for p in lhs}) == 1
    got = ntt.fast_coset_divide_columns(lhs, divisors, g, root, order)
    assert got == [ntt.fast_coset_divide(l, d, g, root, order) for l, d in zip(lhs, divisors)] == quotients
    shared = [q * divisors[1] for q in quotients[:1] * 3]
    assert ntt.fast_coset_divide_columns(shared, divisors[1], g, root, order) == [quotients[0]] * 3
    # degenerate shapes go column by column: mixed degrees, a zero numerator, degree < 8
    mixed = [lhs[0], quotients[1] * divisors[0]]
    assert ntt.fast_coset_divide_columns(mixed, divisors[0], g, root, order) == [ntt.fast_coset_divide(l, divisors[0], g, root, order) for l in mixed]
    assert ntt.fast_coset_divide_columns([_poly(field, []), lhs[0]], divisors[0], g, root, order) == [_poly(field, []), quotients[0]]
    small = [_poly(field, [6, 5, 1]), _poly(field, [12, 7, 1])]
    assert ntt.fast_coset_divide_columns(small, _poly(field, [3, 1]), g, root, order) == [_poly(field, [2, 1]), _poly(field, [4, 1])]
    assert ntt.fast_coset_divide_columns([], divisors[0], g, root, order) == []


def test_coset_divide_columns_device_raises_what_the_loop_raises(sc, field):
    import ntt
    from ntt import DevicePolynomial
    order = 1 << 10
    root, g = field.primitive_nth_root(order), field.generator()
    d = _poly(field, [3, 0, 1])
    quotients = [_poly(field, synth.synth_ints(2000 + c, 300)) for c in range(4)]
    lhs = [q * d for q in quotients]
    one = _poly(field, [1])
    # the transforms run on the coset g <root^2> (the order shrinks to 512 for degree 301): X - g root^10 vanishes at its fifth point
    vanishing = _poly(field, [(P - G * pow(root.value, 10, P) % P) % P, 1]) * _poly(field, [1, 1])
    before = free_slots(sc)

    def run(numerators, divisors, columns):
        dn = [DevicePolynomial.from_polynomial(p, field) for p in numerators]
        dd = [DevicePolynomial.from_polynomial(p, field) for p in divisors]
        pending = []
        if columns:
            results = ntt.coset_divide_columns_device(dn, dd, g, root, order, later=pending)
            assert len(pending) == 1
        else:
            results = [ntt.coset_divide_device(l, r, g, root, order, exact=True, later=pending) for l, r in zip(dn, dd)]
        try:
            for verdict in pending:
                verdict()
        except AssertionError as raised:
            outcome = str(raised)
        else:
            outcome = [r.to_polynomial() for r in results]
        finally:
            del pending[:]
        return outcome

    assert run(lhs, [d] * 4, True) == run(lhs, [d] * 4, False) == quotients
    inexact = lhs[:2] + [lhs[2] + one] + lhs[3:]
    assert run(inexact, [d] * 4, True) == run(inexact, [d] * 4, False) == "cannot perform polynomial division because remainder is not zero"
    by_zero = [d, d, d, vanishing]
    assert run(lhs, by_zero, True) == run(lhs, by_zero, False) == "divide by zero"
    both = [d, vanishing, d, d]                              # the lower column decides: a zero divisor in column 1, a remainder in column 2
    assert run(inexact, both, True) == run(inexact, both, False) == "divide by zero"
    # waited for on the spot without a list; one shared divisor
    dn = [DevicePolynomial.from_polynomial(p, field) for p in lhs]
    assert [r.to_polynomial() for r in ntt.coset_divide_columns_device(dn, DevicePolynomial.from_polynomial(d, field), g, root, order)] == quotients
    with pytest.raises(AssertionError, match="remainder is not zero"):
        ntt.coset_divide_columns_device([DevicePolynomial.from_polynomial(p, field) for p in inexact], DevicePolynomial.from_polynomial(d, field), g, root, order)
    import gc
    gc.collect()
    assert free_slots(sc) == before                          # every verdict gave its slot back


def test_combine_columns_device_equals_the_axpy_chain(sc, field):
    import ntt
    from ntt import DevicePolynomial
    from fast_stark import FastStark
    from algebra import FieldElement
    cols, max_degree = 3, 255
    stark = FastStark.__new__(FastStark)
    stark.field = field
    lengths = [(256, None), (200, 55), (131, 124), (0, 3)]
    polys = [[DevicePolynomial.from_polynomial(_poly(field, synth.synth_ints(2100 + 10 * t + c, n)), field) for c in range(cols)] for t, (n, _) in enumerate(lengths)]
    weights = [[FieldElement(w, field) for w in synth.synth_ints(2200 + c, 7)] for c in range(cols)]
    weights[0][1], weights[1][2], weights[2][0] = FieldElement(0, field), FieldElement(1, field), FieldElement(P - 1, field)
    got = ntt.combine_columns_device([(polys[t], shift) for t, (_, shift) in enumerate(lengths)], weights, max_degree + 1)
    for c in range(cols):
        want = stark._combination_on_device([(polys[t][c], shift) for t, (_, shift) in enumerate(lengths)], weights[c], max_degree)
        assert len(got[c]) == len(want) == max_degree + 1
        assert got[c].vec.to_bytes(0, max_degree + 1) == want.vec.to_bytes(0, max_degree + 1)
        one_pass = stark._combination_on_device([(polys[t][c], shift) for t, (_, shift) in enumerate(lengths)], weights[c], max_degree, one_pass=True)
        assert one_pass.vec.to_bytes(0, max_degree + 1) == want.vec.to_bytes(0, max_degree + 1)

"""The deferred division checks (include/starkcore.h: sc_pointwise_div_later_dev, sc_coset_divide_later_dev, sc_later_wait) called
directly: the quotients against the C oracle's restatement of the reference (oracle/py_oracle.py) and the verdict words against
plain Python integers -- at the lengths where the batch-inverting kernel's last chunk is partial, transform orders of one, two and
three passes, many checks in flight at once, two streams, and with the pinned slots (shared with the asynchronous Merkle roots) all
taken.  No expected value comes from another GPU path; where a GPU entry is compared with another, the oracle pins one of them."""
import ctypes
import gc
import hashlib
import random

import numpy as np
import pytest

from conftest import load_golden
from oracle import py_oracle as po
import synth

pytestmark = pytest.mark.gpu
C = po.C
P = po.P
G = po.GENERATOR


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    starkcore.set_tuning("small_divisor_direct", 1)


def _ints(buf):
    return synth.unpack_ints(buf)


def _words(later):
    """sc_later_wait on a raw handle: the eight words"""
    import starkcore
    w = (ctypes.c_int64 * 8)()
    starkcore._check(starkcore.lib().sc_later_wait(later, w))
    return list(w)


def _div_later(sc, a_ptr, b_ptr, out_ptr, n, stream=None):
    h = ctypes.c_void_p()
    sc._check(sc.lib().sc_pointwise_div_later_dev(a_ptr, b_ptr, out_ptr, n, ctypes.byref(h), stream))
    return h


def _coset_later(sc, a, na, b, nb, root, order, out, n_out):
    h = ctypes.c_void_p()
    sc._check(sc.lib().sc_coset_divide_later_dev(a.ptr, na, b.ptr, nb, sc.fe_bytes(G), sc.fe_bytes(root), order, out.ptr, n_out, ctypes.byref(h), None))
    return h


def _coset_sync(sc, a, na, b, nb, root, order, n_out):
    out, exact = sc.DeviceVector(n_out), ctypes.c_int(-1)
    sc._check(sc.lib().sc_coset_divide_dev(a.ptr, na, b.ptr, nb, sc.fe_bytes(G), sc.fe_bytes(root), order, out.ptr, n_out, ctypes.byref(exact), None))
    return out.to_bytes(), exact.value


def _with_zero(data, idx):
    b = bytearray(data)
    b[16 * idx:16 * idx + 16] = bytes(16)
    return bytes(b)


def _nonzero(n, seed):
    """n canonical residues, none of them zero"""
    raw = synth.synth_packed(seed, n)
    limbs = np.frombuffer(raw.tobytes(), dtype=np.uint64).reshape(n, 2).copy()
    limbs[(limbs[:, 0] == 0) & (limbs[:, 1] == 0), 0] = 1
    return limbs.tobytes()


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

POINTWISE_LENGTHS = [1, 2, 15, 16, 17, 255, 4095, 4096, 4097, (1 << 16) + 1, (1 << 20) + 3]
_expected = {}


def _pointwise_case(n):
    if n not in _expected:
        a, b = synth.synth_packed(7000 + n % 997, n).tobytes(), _nonzero(n, 7100 + n % 991)
        _expected[n] = (a, b, C.pointwise_div(a, b, n))
    return _expected[n]


@pytest.mark.parametrize("n", POINTWISE_LENGTHS)
def test_pointwise_div_later_matches_the_oracle(sc, n):
    """sc_pointwise_div_later_dev element for element against the oracle, out of place and in place, on the library's stream and
    on a caller's; every thread inverts 16 strided values at once, so the lengths straddle the partial last chunk"""
    import torch
    a, b, want = _pointwise_case(n)
    other = torch.cuda.Stream()
    for stream in (None, ctypes.c_void_p(other.cuda_stream)):
        for in_place in (False, True):
            da, db = sc.DeviceVector.from_bytes(a), sc.DeviceVector.from_bytes(b)
            out = da if in_place else sc.DeviceVector.from_bytes(bytes(16 * n))
            if stream is not None:
                sc.synchronize()                    # (short uploads are only enqueued on the library's stream)
            h = _div_later(sc, da.ptr, db.ptr, out.ptr, n, stream)
            words = _words(h)
            if stream is not None:
                other.synchronize()
            assert words[0] == 0 and words[1] == -1, (n, in_place, stream)
            assert out.to_bytes() == want, (n, in_place, stream)
            if not in_place:
                assert da.to_bytes() == a


@pytest.mark.parametrize("n", [1, 17, 4097, (1 << 16) + 1])
def test_pointwise_div_later_flags_a_zero_divisor(sc, n):
    """a zero divisor value anywhere -- the first, the last, inside the partial last chunk, the middle -- sets words[0], and the
    waiting form says SC_ERR_DIV_ZERO on the same inputs (code/algebra.py:92)"""
    a, b, _ = _pointwise_case(n)
    nthreads = ((n + 15) // 16 + 255) // 256 * 256             # value i is the (i // nthreads)-th of the 16 a thread inverts together
    last_row = (n - 1) // nthreads * nthreads                   # the last, partial row of those
    places = sorted({0, n - 1, n // 2, last_row + (n - last_row) // 2})
    lib = sc.lib()
    for idx in places:
        bz = _with_zero(b, idx)
        da, db, out = sc.DeviceVector.from_bytes(a), sc.DeviceVector.from_bytes(bz), sc.DeviceVector(n)
        words = _words(_div_later(sc, da.ptr, db.ptr, out.ptr, n))
        assert words[0] != 0 and words[1] == -1, (n, idx)
        assert lib.sc_pointwise_div_dev(da.ptr, db.ptr, out.ptr, n, None) == sc.SC_ERR_DIV_ZERO, (n, idx)
        # the next check on the same words is clean again
        db_clean = sc.DeviceVector.from_bytes(b)
        words = _words(_div_later(sc, da.ptr, db_clean.ptr, out.ptr, n))
        assert words[0] == 0, (n, idx)


# ---------------------------------------------------------------- coset division

def _interpolant(num, d, root, order):
    """ntt.py:159-176 with the oracle's primitives: all `order` coefficients of the unscaled interpolant of the value quotient.
    (Above 2^17 values the value quotient is taken with Python integers, batch-inverted: the oracle inverts value by value,
    which takes tens of seconds at 2^21.)"""
    ca = C.coset_evaluate(synth.pack_ints(num), len(num), G, root, order)
    cb = C.coset_evaluate(synth.pack_ints(d), len(d), G, root, order)
    if order <= 1 << 17:
        quo = C.pointwise_div(ca, cb, order)
    else:
        a, b = _ints(ca), _ints(cb)
        pre, acc = [], 1
        for v in b:
            pre.append(acc)
            acc = acc * v % P
        inv, out = pow(acc, -1, P), [0] * order
        for i in range(order - 1, -1, -1):
            out[i] = a[i] * inv % P * pre[i] % P
            inv = inv * b[i] % P
        quo = synth.pack_ints(out)
    return C.scale(C.intt(root, quo, order), order, pow(G, -1, P))


# (quotient length, divisor length, order, n_out or None for the quotient's length)
COSET_CASES = [
    (1, 2, 2, None), (1, 1, 2, 2), (3, 2, 4, None), (9, 1, 16, None), (30, 2, 64, None), (20, 12, 64, 64), (700, 3, 1024, None),
    (3000, 8, 1 << 12, None), (3000, 9, 1 << 12, None), (3000, 9, 1 << 12, 1 << 12), (50000, 3, 1 << 16, None),
    (40000, 20, 1 << 17, None), (200001, 2, 1 << 18, 5), ((1 << 20) + 5, 2, 1 << 21, None),
]


@pytest.mark.parametrize("lq,ld,order,n_out", COSET_CASES)
def test_coset_divide_later_matches_the_oracle(sc, lq, ld, order, n_out):
    """sc_coset_divide_later_dev: exact divisions return q; inexact ones the bytes of the oracle's restatement of ntt.py:159-176;
    both the bytes of sc_coset_divide_dev.  words[1] is the integer degree, counted from n_out, of the interpolant's coefficients
    [n_out, order) -- -1 when order == n_out; a quotient cut short (n_out < its length) puts it at a known index, past several
    blocks of the degree scan at the larger orders.  Divisors of 1-8 coefficients take the direct path unless it is switched off."""
    k = COSET_CASES.index((lq, ld, order, n_out))
    q, d = synth.synth_ints(8000 + k, lq), synth.synth_ints(8100 + k, ld)
    q[-1], d[-1] = q[-1] or 1, d[-1] or 1
    root = po.primitive_nth_root(order)
    lhs = po.schoolbook_mul(q, d)
    n_out = lq if n_out is None else n_out
    for exact in (True, False):
        if exact:
            num = lhs
            full = synth.pack_ints(q) + bytes(16 * (order - lq))
        else:
            num = [(v + 1) % P for v in lhs]
            full = _interpolant(num, d, root, order)
        want_q = full[:16 * n_out]
        want_deg = po.degree(_ints(full[16 * n_out:])) if order > n_out else -1
        da, db = sc.DeviceVector.from_ints(num), sc.DeviceVector.from_ints(d)
        for direct in (1, 0):
            sc.set_tuning("small_divisor_direct", direct)
            out = sc.DeviceVector(n_out)
            words = _words(_coset_later(sc, da, len(num), db, ld, root, order, out, n_out))
            got = out.to_bytes()
            sync, flag = _coset_sync(sc, da, len(num), db, ld, root, order, n_out)
            assert got == want_q, (lq, ld, order, exact, direct)
            assert sync == got, (lq, ld, order, exact, direct)
            assert words[0] == 0 and words[1] == want_deg, (lq, ld, order, exact, direct, words[:2])
            assert flag == (1 if want_deg < 0 else 0)
            if exact and n_out == lq:
                assert want_deg == -1
            if order == n_out:
                assert words[1] == -1
    sc.set_tuning("small_divisor_direct", 1)


@pytest.mark.parametrize("order,k", [(16, 3), (1 << 12, 4095), (1 << 17, 77777)])
def test_coset_divide_later_flags_a_divisor_that_vanishes_on_the_coset(sc, order, k):
    """X - g * w^k is zero at the k-th point of the coset g <w>: words[0] != 0, as sc_coset_divide_dev says SC_ERR_DIV_ZERO"""
    root = po.primitive_nth_root(order)
    z = G * pow(root, k, P) % P
    d = [(P - z) % P, 1]
    num = synth.synth_ints(8500 + k, order // 2)
    da, db = sc.DeviceVector.from_ints(num), sc.DeviceVector.from_ints(d)
    for direct in (1, 0):
        sc.set_tuning("small_divisor_direct", direct)
        out = sc.DeviceVector(len(num) - 1)
        words = _words(_coset_later(sc, da, len(num), db, 2, root, order, out, len(num) - 1))
        assert words[0] != 0, (order, k, direct)
        out2, exact = sc.DeviceVector(len(num) - 1), ctypes.c_int(-1)
        rc = sc.lib().sc_coset_divide_dev(da.ptr, len(num), db.ptr, 2, sc.fe_bytes(G), sc.fe_bytes(root), order, out2.ptr, len(num) - 1, ctypes.byref(exact), None)
        assert rc == sc.SC_ERR_DIV_ZERO
    sc.set_tuning("small_divisor_direct", 1)


# ---------------------------------------------------------------- many checks in flight

def test_many_checks_in_flight_each_report_their_own_words(sc):
    """about 64 handles open at once with mixed verdicts, interleaved with sc_vec_degree_dev, sc_mpoly_eval_dev and synchronous
    coset divisions on the same stream (which use the library's shared scratch words); waited for in reverse and in shuffled
    order, every handle reports its own division's words"""
    lib = sc.lib()
    rng = random.Random(2024)
    order, lq, ld = 1 << 10, 500, 3
    root = po.primitive_nth_root(order)
    q, d = synth.synth_ints(9000, lq), synth.synth_ints(9001, ld)
    q[-1], d[-1] = q[-1] or 1, d[-1] or 1
    lhs = po.schoolbook_mul(q, d)
    dlhs, dd = sc.DeviceVector.from_ints(lhs), sc.DeviceVector.from_ints(d)
    bad_num = [(v + 1) % P for v in lhs]
    bad = sc.DeviceVector.from_ints(bad_num)
    bad_full = _interpolant(bad_num, d, root, order)
    bad_deg = po.degree(_ints(bad_full[16 * lq:]))
    zk = 3
    dz = sc.DeviceVector.from_ints([(P - G * pow(root, zk, P) % P) % P, 1])
    n = 300
    a, b = synth.synth_packed(9100, n).tobytes(), _nonzero(n, 9101)
    da, db, dbz = sc.DeviceVector.from_bytes(a), sc.DeviceVector.from_bytes(b), sc.DeviceVector.from_bytes(_with_zero(b, 123))
    want_div = C.pointwise_div(a, b, n)
    assert bad_deg >= 0
    deg_vec_vals = [0] * 5000
    deg_vec_vals[4321] = 9
    deg_vec = sc.DeviceVector.from_ints(deg_vec_vals)
    mp_vals = [synth.synth_ints(9200 + j, 64) for j in range(2)]
    mp_terms = [((1, 2), 5), ((0, 0), 7), ((3, 1), P - 2)]
    mp_want = [sum(c * pow(mp_vals[0][i], e[0], P) * pow(mp_vals[1][i], e[1], P) for e, c in mp_terms) % P for i in range(64)]
    for rounds in range(2):
        held = []                      # (handle, expected words[0] != 0, expected words[1], output vector, expected output bytes)
        for i in range(64):
            kind = i % 5
            if kind == 0:
                out = sc.DeviceVector(n)
                held.append((_div_later(sc, da.ptr, db.ptr, out.ptr, n), False, -1, out, want_div))
            elif kind == 1:
                out = sc.DeviceVector(n)
                held.append((_div_later(sc, da.ptr, dbz.ptr, out.ptr, n), True, -1, out, None))
            elif kind == 2:
                cut = rng.choice([lq, lq - 1, lq - 37])
                out = sc.DeviceVector(cut)
                held.append((_coset_later(sc, dlhs, len(lhs), dd, ld, root, order, out, cut), False, lq - 1 - cut if cut < lq else -1, out,
                             synth.pack_ints(q[:cut])))
            elif kind == 3:
                out = sc.DeviceVector(lq)
                held.append((_coset_later(sc, bad, len(lhs), dd, ld, root, order, out, lq), False, bad_deg, out, bad_full[:16 * lq]))
            else:
                out = sc.DeviceVector(len(lhs) - 1)
                held.append((_coset_later(sc, dlhs, len(lhs), dz, 2, root, order, out, len(lhs) - 1), True, None, out, None))
            # unrelated work between the checks, on the same stream
            step = i % 3
            if step == 0:
                deg = ctypes.c_int64(-7)
                sc._check(lib.sc_vec_degree_dev(deg_vec.ptr, len(deg_vec_vals), ctypes.byref(deg), None))
                assert deg.value == 4321
            elif step == 1:
                dv, mo = sc.DeviceVector.from_ints(mp_vals[0] + mp_vals[1]), sc.DeviceVector(64)
                exps = bytes(e for k, _ in mp_terms for e in k)
                sc._check(lib.sc_mpoly_eval_dev(dv.ptr, 2, 64, exps, synth.pack_ints([c for _, c in mp_terms]), len(mp_terms), mo.ptr, None))
                assert _ints(mo.to_bytes()) == mp_want
            else:
                got, flag = _coset_sync(sc, bad, len(lhs), dd, ld, root, order, lq)
                assert flag == 0
                got, flag = _coset_sync(sc, dlhs, len(lhs), dd, ld, root, order, lq)
                assert flag == 1 and got == synth.pack_ints(q)
        order_of_waits = list(range(len(held)))[::-1] if rounds == 0 else rng.sample(range(len(held)), len(held))
        for j in order_of_waits:
            h, zero, deg, out, want = held[j]
            w = _words(h)
            assert (w[0] != 0) == zero, (j, w[:2])
            if deg is not None:
                assert w[1] == deg, (j, w[:2])
            if want is not None:
                assert out.to_bytes() == want, j


def test_two_streams_each_get_their_own_verdict(sc):
    """deferred pointwise divisions of 2^22 elements in flight together on the library's stream and on a caller's, one with a zero
    divisor and one without: both verdicts right, and the clean quotient right at sampled indices (Python integers).  Before each
    check had words of its own the flag word was shared process-wide, so this was a race that could pass by luck; the per-check
    words make it right by construction, and the test guards against that coming back."""
    import torch
    n = 1 << 22
    a, b = synth.synth_packed(9300, n).tobytes(), _nonzero(n, 9301)
    bz = _with_zero(b, n - 5)
    other = torch.cuda.Stream()
    s_other = ctypes.c_void_p(other.cuda_stream)
    da, db, dbz = sc.DeviceVector.from_bytes(a), sc.DeviceVector.from_bytes(b), sc.DeviceVector.from_bytes(bz)
    sc.synchronize()
    ai, bi = np.frombuffer(a, dtype=np.uint64), np.frombuffer(b, dtype=np.uint64)
    rng = random.Random(5)
    picks = sorted(rng.sample(range(n), 200) + [0, n - 1])
    for zero_on_library in (True, False):
        out_l, out_o = sc.DeviceVector(n), sc.DeviceVector(n)
        sc.stream_join(other.cuda_stream)
        h_l = _div_later(sc, da.ptr, (dbz if zero_on_library else db).ptr, out_l.ptr, n, None)
        h_o = _div_later(sc, da.ptr, (db if zero_on_library else dbz).ptr, out_o.ptr, n, s_other)
        w_o, w_l = _words(h_o), _words(h_l)
        other.synchronize()
        assert (w_l[0] != 0) == zero_on_library and (w_o[0] != 0) == (not zero_on_library), (zero_on_library, w_l[:2], w_o[:2])
        assert w_l[1] == -1 and w_o[1] == -1
        clean = out_o if zero_on_library else out_l
        for i in picks:
            x = int(ai[2 * i]) | int(ai[2 * i + 1]) << 64
            y = int(bi[2 * i]) | int(bi[2 * i + 1]) << 64
            assert _ints(clean.to_bytes(i, 1)) == [x * pow(y, -1, P) % P], i


# ---------------------------------------------------------------- slots

def test_abandoned_handles_give_their_slots_back(sc):
    """a handle waited for at once and a starkcore.Later dropped without waiting: the number of slots that can be drained
    afterwards is the number before"""
    before = free_slots(sc)
    assert before > 0
    n = 4097
    a, b, want = _pointwise_case(n)
    da, db, out = sc.DeviceVector.from_bytes(a), sc.DeviceVector.from_bytes(b), sc.DeviceVector(n)
    assert _words(_div_later(sc, da.ptr, db.ptr, out.ptr, n))[:2] == [0, -1]
    dropped = sc.Later(_div_later(sc, da.ptr, db.ptr, out.ptr, n))
    assert free_slots(sc) == before - 1
    del dropped
    gc.collect()
    assert free_slots(sc) == before
    assert out.to_bytes() == want


def test_exhausted_slots_enqueue_nothing_and_the_fallbacks_agree(sc):
    """with every pinned slot taken, the deferred entries return SC_ERR_UNSUPPORTED with NOTHING enqueued -- an in-place numerator
    and an output are byte-identical afterwards, so the waiting form may follow in place -- and every entry that falls back to a
    copy without a slot (sc_coset_divide_dev's exactness, sc_vec_degree_dev, sc_pointwise_div_dev's zero check, the asynchronous
    Merkle builds) answers as it does with slots free, i.e. as the oracle does"""
    lib = sc.lib()
    before = free_slots(sc)
    n = 4097
    a, b, want = _pointwise_case(n)
    order, lq, ld = 1 << 12, 3000, 3
    root = po.primitive_nth_root(order)
    q, d = synth.synth_ints(9400, lq), synth.synth_ints(9401, ld)
    q[-1], d[-1] = q[-1] or 1, d[-1] or 1
    lhs = po.schoolbook_mul(q, d)
    dlhs, dd = sc.DeviceVector.from_ints(lhs), sc.DeviceVector.from_ints(d)
    bad = sc.DeviceVector.from_ints([(v + 1) % P for v in lhs])
    N = 1 << 11
    mdata = synth.synth_packed(9402, N).tobytes()
    mvec = sc.DeviceVector.from_bytes(mdata)
    mroot = C.merkle_commit(mdata, N)
    leaves = sc.DeviceVector.from_bytes(C.merkle_tree(mdata, N)[:64 * N])
    deg_vals = [0] * 70000
    deg_vals[12345] = 1
    deg_vec = sc.DeviceVector.from_ints(deg_vals)
    da, db, dbz = sc.DeviceVector.from_bytes(a), sc.DeviceVector.from_bytes(b), sc.DeviceVector.from_bytes(_with_zero(b, n - 1))

    def answers():
        out = {}
        out["exact"] = _coset_sync(sc, dlhs, len(lhs), dd, ld, root, order, lq)
        out["inexact"] = _coset_sync(sc, bad, len(lhs), dd, ld, root, order, lq)[1]
        deg = ctypes.c_int64(-7)
        sc._check(lib.sc_vec_degree_dev(deg_vec.ptr, len(deg_vals), ctypes.byref(deg), None))
        out["degree"] = deg.value
        tmp = sc.DeviceVector(n)
        out["div_zero"] = lib.sc_pointwise_div_dev(da.ptr, dbz.ptr, tmp.ptr, n, None)
        out["div"] = (lib.sc_pointwise_div_dev(da.ptr, db.ptr, tmp.ptr, n, None), tmp.to_bytes())
        out["merkle_async"] = sc.MerkleTree.from_device_async(mvec).root
        out["from_digests"] = sc.MerkleTree.from_digests_ptr(leaves.ptr, N).root
        return out

    free = answers()
    assert free == {"exact": (synth.pack_ints(q), 1), "inexact": 0, "degree": 12345, "div_zero": sc.SC_ERR_DIV_ZERO, "div": (0, want),
                    "merkle_async": mroot, "from_digests": mroot}
    drained = Drained(sc)
    try:
        assert len(drained) == before
        # in place: the numerator must come back untouched
        num = sc.DeviceVector.from_bytes(a)
        h = ctypes.c_void_p()
        assert lib.sc_pointwise_div_later_dev(num.ptr, db.ptr, num.ptr, n, ctypes.byref(h), None) == sc.SC_ERR_UNSUPPORTED
        sentinel = synth.synth_packed(9403, lq).tobytes()
        out = sc.DeviceVector.from_bytes(sentinel)
        assert lib.sc_coset_divide_later_dev(dlhs.ptr, len(lhs), dd.ptr, ld, sc.fe_bytes(G), sc.fe_bytes(root), order, out.ptr, lq,
                                             ctypes.byref(h), None) == sc.SC_ERR_UNSUPPORTED
        sc.synchronize()
        assert num.to_bytes() == a
        assert out.to_bytes() == sentinel
        # ... so the waiting form in place gives the quotient once
        sc._check(lib.sc_pointwise_div_dev(num.ptr, db.ptr, num.ptr, n, None))
        assert num.to_bytes() == want
        assert answers() == free
        assert len(Drained(sc)) == 0
    finally:
        drained.release()
    assert free_slots(sc) == before


# ---------------------------------------------------------------- the prover

def _seed_urandom(fast_stark, seed):
    rng = random.Random(seed)
    fast_stark.os.urandom = lambda k: bytes(rng.getrandbits(8) for _ in range(k))


def test_prover_with_slots_drained_and_a_failing_check(sc, monkeypatch):
    """FastStark.prove (every polynomial in HBM: DEVICE_MIN = 32) with every pinned slot taken reproduces the reference's golden
    proofs, and no transition quotient goes the reference's way (the in-place pointwise division is not done twice); a prove
    with a false boundary raises the reference's remainder assertion, and once that exception is gone every slot is back and
    the next prove is byte-identical again"""
    import fast_stark
    from fast_stark import FastStark
    from algebra import Field, FieldElement
    from workload_rescue_prime import RescuePrime
    monkeypatch.setattr(FastStark, "DEVICE_MIN", 32)
    monkeypatch.setattr(fast_stark.os, "urandom", fast_stark.os.urandom)
    reference_way = []
    inner = fast_stark.coset_divide_device

    def counted(*args, **kwargs):
        if not kwargs.get("exact", False):
            reference_way.append(args[0])
        return inner(*args, **kwargs)
    monkeypatch.setattr(fast_stark, "coset_divide_device", counted)
    g = load_golden("fast_stark.json")
    field = Field.main()
    rp = RescuePrime()
    rec = g["runs"][0]
    input_element = FieldElement(int(rec["input"]), field)
    output_element = rp.hash(input_element)
    stark = FastStark(field, rec["expansion_factor"], rec["num_colinearity_checks"], rec["security_level"], rp.m, rp.N + 1)
    tz, tz_codeword, tz_root = stark.preprocess()
    trace = rp.trace(input_element)
    air = rp.transition_constraints(stark.omicron)

    def prove(boundary):
        _seed_urandom(fast_stark, rec["urandom_seed"])
        return stark.prove(trace, air, boundary, tz, tz_codeword)

    before = free_slots(sc)
    drained = Drained(sc)
    try:
        proof = prove(rp.boundary_constraints(output_element))
        assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]
        assert reference_way == [], "a transition quotient was re-derived the reference's way"
    finally:
        drained.release()
    assert free_slots(sc) == before
    # a false claim: the boundary quotient of register 0 leaves a remainder; the deferred check raises what the reference raises
    with pytest.raises(AssertionError, match="remainder is not zero"):
        prove(rp.boundary_constraints(output_element + field.one()))
    gc.collect()
    assert free_slots(sc) == before
    proof = prove(rp.boundary_constraints(output_element))
    assert hashlib.sha256(proof).hexdigest() == rec["proof_sha256"]
    assert reference_way == []

"""The entries include/starkcore.h documents as free of the one-stream rule, in flight on several HIP streams at once: the division
with remainder (sc_poly_divmod_dev, sc_poly_divmod_columns_dev), the columns divisions with one deferred verdict
(sc_pointwise_div_columns_later_dev, sc_coset_divide_columns_later_dev) and the transforms (sc_ntt_dev, sc_coset_evaluate_dev) -- and,
for the other class, the documented way to take entries with shared scratch buffers across streams: ordered by events.

What is at stake is host machinery that every single-stream test passes over: temporaries that go back to the exact-size free lists
behind one event per stream in use (csrc/core.h: PoolTmpAsync, release_after_streams, Ctx::seen_streams), the per-stream work and
flag buffers of the transforms, the pinned slots and their sequence numbers, the table caches.  Every test computes its expectations
first, on the library's stream, one call at a time, and pins them to the oracle (the defining property a = q b + r by the oracle's
product, the oracle's interpolants and pointwise quotients, its transforms, Python integers); then the same calls are enqueued on
their streams with no host wait of the test's own in between, and every output must equal its expectation byte for byte, the
sentinels behind and between the outputs included.  A correct library is deterministic here; nothing is asserted about timing.

DeviceVector.from_ints / from_bytes upload on the library's stream, short vectors without waiting, so every test calls
sc.synchronize() between building operands and the first call on a caller's stream."""
import ctypes
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
from oracle import py_oracle as po
import poly_divide_cases as cases
import synth
import test_gpu_columns_divide as cdiv        # the helpers of the single-stream tests of the same entries, not copies of them
import test_gpu_poly_divide as pdiv

pytestmark = pytest.mark.gpu
C = po.C
P = po.P
G = po.GENERATOR
GUARD = pdiv.GUARD


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def handle_of(stream):
    """a torch stream as the entries take it; None stays None (the library's own stream)"""
    return None if stream is None else ctypes.c_void_p(stream.cuda_stream)


def caller_streams(torch, count):
    dev = torch.device("cuda", 0)
    return [torch.cuda.Stream(device=dev) for _ in range(count)]


def keep_tensor(torch, rounds, elems):
    """device memory of the test's own for `rounds` outputs of `elems` field elements each"""
    return torch.empty((rounds, max(elems, 1), 2), dtype=torch.int64, device=torch.device("cuda", 0))


def kept_bytes(t, rnd, elems):
    return t[rnd].cpu().numpy().tobytes()[:16 * elems]


def copy_on(sc, dst_ptr, src_ptr, elems, stream):
    sc._check(sc.lib().sc_memcpy_dev(ctypes.c_void_p(int(dst_ptr)), ctypes.c_void_p(int(src_ptr)), elems, handle_of(stream)))


# ---- the division with remainder at multi-pass sizes ----------------------------------------------------------------------------

NA, NB, DIV_COLS = 4200, 2100, 3                      # m = 2101: Newton up to 2^13, the quotient product at 2^13, the remainder product at 2^12
M, NR = NA - NB + 1, NB - 1
LD_A, LD_Q, LD_R = NA + 5, M + 3, NR + 2
Q_ELEMS, R_ELEMS = M + GUARD, NR + GUARD              # what the outputs hold: the values, then the guard
CQ_ELEMS, CR_ELEMS = DIV_COLS * LD_Q + GUARD, DIV_COLS * LD_R + GUARD
FORMS = ((True, True), (True, True), (True, False), (False, True))      # (quotient, remainder) asked for, by round


class DivmodCase:
    """One stream's operands of sc_poly_divmod_dev and sc_poly_divmod_columns_dev, resident, and what the outputs must hold -- guard
    and gaps included -- for each of the three forms."""

    def __init__(self, sc, seed):
        self.a = synth.synth_ints(seed, NA)
        self.b = synth.synth_ints(seed + 1, NB)
        self.b[-1] = self.b[-1] or 1
        self.columns = [synth.synth_ints(seed + 2 + c, NA) for c in range(DIV_COLS)]
        self.b2 = synth.synth_ints(seed + 7, NB)
        self.b2[-1] = P - 2
        # one call at a time on the library's stream; pdiv's helpers check the guards and the gaps
        q, r = pdiv.dev_divmod(sc, self.a, self.b)
        cq, cr = pdiv.dev_divmod_columns(sc, self.columns, self.b2, LD_A, LD_Q, LD_R)
        for a, b, qc, rc in [(self.a, self.b, q, r)] + [(col, self.b2, x, y) for col, x, y in zip(self.columns, cq, cr)]:
            qi, ri = synth.unpack_ints(qc), synth.unpack_ints(rc)
            assert len(qi) == M and len(ri) == NB - 1 and max(qi) < P and max(ri) < P
            assert pdiv.trim(po.poly_add(pdiv.oracle_product(qi, b), ri)) == pdiv.trim(a)
        assert pdiv.dev_divmod(sc, self.a, self.b, want_r=False) == (q, None)
        assert pdiv.dev_divmod(sc, self.a, self.b, want_q=False) == (None, r)
        assert pdiv.dev_divmod_columns(sc, self.columns, self.b2, LD_A, LD_Q, LD_R, want_r=False) == [cq, None]
        assert pdiv.dev_divmod_columns(sc, self.columns, self.b2, LD_A, LD_Q, LD_R, want_q=False) == [None, cr]
        S = pdiv.SENTINEL
        self.want = {
            "q": q + S * GUARD, "r": r + S * GUARD,
            "cq": b"".join(x + S * (LD_Q - M) for x in cq) + S * GUARD, "cr": b"".join(x + S * (LD_R - NR) for x in cr) + S * GUARD,
        }
        self.untouched = {"q": S * Q_ELEMS, "r": S * R_ELEMS, "cq": S * CQ_ELEMS, "cr": S * CR_ELEMS}
        self.da, self.db = sc.DeviceVector.from_ints(self.a), sc.DeviceVector.from_ints(self.b)
        self.dmat, self.db2 = pdiv.matrix_of(sc, self.columns, NA, LD_A), sc.DeviceVector.from_ints(self.b2)

    def expected(self, name, form):
        asked = form[0] if name in ("q", "cq") else form[1]
        return self.want[name] if asked else self.untouched[name]


@functools.lru_cache(maxsize=None)
def divmod_case(sc, seed):
    return DivmodCase(sc, seed)


def enqueue_divmod(sc, case, form, dq, dr, stream):
    want_q, want_r = form
    sc._check(sc.lib().sc_poly_divmod_dev(case.da.ptr, NA, case.db.ptr, NB, dq.ptr if want_q else None, dr.ptr if want_r else None, handle_of(stream)))


def enqueue_divmod_columns(sc, case, form, cq, cr, stream):
    want_q, want_r = form
    sc._check(sc.lib().sc_poly_divmod_columns_dev(case.dmat.ptr, NA, LD_A, DIV_COLS, case.db2.ptr, NB, cq.ptr if want_q else None, LD_Q,
                                                  cr.ptr if want_r else None, LD_R, handle_of(stream)))


def divmod_rounds(sc, torch, streams, rounds, observe=False):
    """`rounds` rounds of both divisions on every stream of `streams`, alternating streams within a round, every stream with operands
    of its own but the same shapes -- so what one stream's call hands back to the exact-size free lists is what the other stream's next
    call asks for.  observe: per-call start and end events; returns how many pairs of calls on different streams overlapped."""
    S = pdiv.SENTINEL
    these = [divmod_case(sc, 9100 + 20 * k) for k in range(len(streams))]
    outs = [[[sc.DeviceVector.from_bytes(S * n) for n in (Q_ELEMS, R_ELEMS, CQ_ELEMS, CR_ELEMS)] for _ in streams] for _ in range(rounds)]
    sc.synchronize()
    sc.set_tuning("pool_trim", 1)                      # the pool starts empty: whatever is recycled from here on was released by these calls
    spans = [[] for _ in streams]
    for rnd in range(rounds):
        form = FORMS[rnd % len(FORMS)]
        for k, (stream, case) in enumerate(zip(streams, these)):
            dq, dr, cq, cr = outs[rnd][k]
            for call, x, y in ((enqueue_divmod, dq, dr), (enqueue_divmod_columns, cq, cr)):
                if observe:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                call(sc, case, form, x, y, stream)
                if observe:
                    t1.record(stream)
                    spans[k].append((t0, t1))
    torch.cuda.synchronize()
    for rnd in range(rounds):
        form = FORMS[rnd % len(FORMS)]
        for k, case in enumerate(these):
            for name, vec in zip(("q", "r", "cq", "cr"), outs[rnd][k]):
                assert vec.to_bytes() == case.expected(name, form), (rnd, k, name, form)
    if not observe:
        return None
    base = spans[0][0][0]
    times = [[(base.elapsed_time(t0), base.elapsed_time(t1)) for t0, t1 in s] for s in spans]
    return sum(1 for s0, e0 in times[0] for s1, e1 in times[1] if s0 < e1 and s1 < e0), len(times[0])


def test_divmod_on_two_streams(sc, torch):
    """sc_poly_divmod_dev and sc_poly_divmod_columns_dev (3 columns, padded pitches) at na = 4200, nb = 2100 -- every transform that
    matters has more than one pass, so the per-stream work buffers are live -- for 12 rounds on two caller streams, different operands
    and equal shapes, the quotient-only and remainder-only forms in every fourth round each.  The header's claim: the temporaries are
    the call's own and go back to the pool behind the streams in use.  A temporary put straight back on the free list would be handed
    to the other stream's next call while the first still reads it; stream-ordered reuse hides that from every single-stream test."""
    assert sc.lib().sc_ntt_num_passes(1 << 12) > 1
    overlapped, calls = divmod_rounds(sc, torch, caller_streams(torch, 2), 12, observe=True)
    print("\ndivmod on two streams: %d of %d x %d pairs of calls on different streams overlapped on the device" % (overlapped, calls, calls))


# ---- the columns divisions with one deferred verdict ----------------------------------------------------------------------------

ORDER = 1 << 12                                        # two passes
ROOT = po.primitive_nth_root(ORDER)
DIVISOR_LEN = 9                                        # above SMALL_DIVISOR: the divisors are transformed
LQ = ORDER // 2 - 3
COSET_N_OUT = [ORDER, LQ, LQ]                          # column 0 keeps every coefficient of its interpolant
PW_N, PW_COLS = 4097, 5
PW_LD_A, PW_LD_B, PW_LD_OUT = PW_N + 3, PW_N + 1, PW_N + 2


class CosetCase:
    """Three columns of sc_coset_divide_columns_later_dev, resident, with the output bytes and the verdict words the oracle's
    interpolants give.  exact: every numerator is a product; else column 1 is a product plus one in every coefficient."""

    def __init__(self, sc, seed, shared, exact):
        self.shared = shared
        columns = []
        for c in range(3):
            q = synth.synth_ints(seed + c, LQ)
            d = synth.synth_ints(seed + 10 + (0 if shared else c), DIVISOR_LEN)
            q[-1], d[-1] = q[-1] or 1, d[-1] or 1
            lhs = po.schoolbook_mul(q, d)
            if c == 1 and not exact:
                lhs = [(v + 1) % P for v in lhs]
            full = cdiv._interpolant(lhs, d, ROOT, ORDER)
            if exact or c != 1:
                assert full == synth.pack_ints(q) + bytes(16 * (ORDER - LQ))
            columns.append((lhs, d, full))
        # one call at a time on the library's stream, against these interpolants and against the single-column entry
        cdiv._check_coset_columns(sc, columns, DIVISOR_LEN, shared, ROOT, ORDER, COSET_N_OUT)
        self.a, self.na, self.ld_a, self.b, self.ld_out = cdiv._coset_operands(sc, columns, DIVISOR_LEN, shared, COSET_N_OUT)
        self.out_elems = 3 * self.ld_out
        self.want = cdiv._matrix([full[:16 * k] for (_, _, full), k in zip(columns, COSET_N_OUT)], self.ld_out)
        self.words = cdiv._verdict_of([(0, cdiv._degree_of(full[16 * k:])) for (_, _, full), k in zip(columns, COSET_N_OUT)])
        assert (self.words == [0, -1, -1, 0]) if exact else (self.words[0] == 0 and self.words[1] >= 0 and self.words[2:] == [1, 1])

    def enqueue(self, sc, out, stream):
        return cdiv._coset_columns_later(sc, self.a, self.na, self.ld_a, self.b, DIVISOR_LEN, 0 if self.shared else DIVISOR_LEN, 3, ROOT, ORDER, out,
                                         COSET_N_OUT, self.ld_out, handle_of(stream))


class PointwiseCase:
    """Five columns of sc_pointwise_div_columns_later_dev, each with a divisor column of its own.  clean: no divisor value is zero;
    else column 3 has one zero.  The expectation is the call on the library's stream, pinned to the oracle's quotients in every
    column without a zero and to the verdict words."""

    def __init__(self, sc, seed, clean):
        a_rows = [synth.synth_packed(seed + c, PW_N).tobytes() for c in range(PW_COLS)]
        b_rows = [cdiv._nonzero(PW_N, seed + 10 + c) for c in range(PW_COLS)]
        bad = () if clean else (3,)
        for c in bad:
            b_rows[c] = b_rows[c][:16 * 4096] + bytes(16) + b_rows[c][16 * 4097:]
        self.a = sc.DeviceVector.from_bytes(cdiv._matrix(a_rows, PW_LD_A))
        self.b = sc.DeviceVector.from_bytes(cdiv._matrix(b_rows, PW_LD_B))
        self.out_elems = PW_COLS * PW_LD_OUT
        out = sc.DeviceVector.from_bytes(cdiv.SENTINEL * self.out_elems)
        self.words = cdiv._div_columns(sc, self.a, PW_LD_A, self.b, PW_LD_B, out, PW_LD_OUT, PW_N, PW_COLS)[:4]
        assert self.words == ([0, -1, -1, 0] if clean else [1, -1, 3, 1])
        self.want = out.to_bytes()
        for c in range(PW_COLS):
            if c not in bad:
                assert cdiv._row(self.want, c, PW_LD_OUT, PW_N) == C.pointwise_div(a_rows[c], b_rows[c], PW_N), c
            assert self.want[16 * (PW_LD_OUT * c + PW_N):16 * PW_LD_OUT * (c + 1)] == cdiv.SENTINEL * (PW_LD_OUT - PW_N)

    def enqueue(self, sc, out, stream):
        return cdiv._div_columns_later(sc, self.a, PW_LD_A, self.b, PW_LD_B, out, PW_LD_OUT, PW_N, PW_COLS, handle_of(stream))


@functools.lru_cache(maxsize=None)
def coset_case(sc, seed, shared, exact):
    return CosetCase(sc, seed, shared, exact)


@functools.lru_cache(maxsize=None)
def pointwise_case(sc, seed, clean):
    return PointwiseCase(sc, seed, clean)


@pytest.mark.parametrize("first_is_library", [True, False], ids=["library_and_caller", "two_callers"])
def test_columns_divisions_on_two_streams(sc, torch, first_is_library):
    """sc_coset_divide_columns_later_dev (order 2^12, 3 columns, divisors of 9 coefficients; a shared divisor in even rounds, one per
    column in odd ones) and sc_pointwise_div_columns_later_dev (n = 4097, 5 columns) for 8 rounds on two streams.  The first stream's
    operands divide exactly by non-zero values; the second's have one inexact column resp. one column with a zero divisor.  Each call
    has value matrices, per-column words, quotient lengths and a pinned slot of its own: every call's four words are its own (the
    lowest failing column, that column's words, the number of failing columns), and both streams' quotients are the oracle's.  The 32
    handles are waited for after the final synchronize (32 of the 256 pinned slots are held until then)."""
    rounds = 8
    streams = [None if first_is_library else caller_streams(torch, 1)[0], caller_streams(torch, 1)[0]]
    per_stream = [
        ([coset_case(sc, 9400, True, True), coset_case(sc, 9420, False, True)], pointwise_case(sc, 9440, True)),
        ([coset_case(sc, 9460, True, False), coset_case(sc, 9480, False, False)], pointwise_case(sc, 9500, False)),
    ]
    outs = [[(sc.DeviceVector.from_bytes(cdiv.SENTINEL * coset[rnd % 2].out_elems), sc.DeviceVector.from_bytes(cdiv.SENTINEL * pw.out_elems))
             for coset, pw in per_stream] for rnd in range(rounds)]
    sc.synchronize()
    handles = []
    for rnd in range(rounds):
        for k, (stream, (coset, pw)) in enumerate(zip(streams, per_stream)):
            handles.append((rnd, k, "coset", coset[rnd % 2].words, coset[rnd % 2].enqueue(sc, outs[rnd][k][0], stream)))
            handles.append((rnd, k, "pointwise", pw.words, pw.enqueue(sc, outs[rnd][k][1], stream)))
    torch.cuda.synchronize()
    assert len(handles) == 32
    for rnd, k, kind, want, handle in handles:
        assert cdiv._words(handle)[:4] == want, (rnd, k, kind)
    for rnd in range(rounds):
        for k, (coset, pw) in enumerate(per_stream):
            assert outs[rnd][k][0].to_bytes() == coset[rnd % 2].want, (rnd, k, "coset")
            assert outs[rnd][k][1].to_bytes() == pw.want, (rnd, k, "pointwise")


# ---- transforms, the division with remainder and the coset division side by side -------------------------------------------------

NTT_N, LDE_M = 1 << 14, 1 << 12


@functools.lru_cache(maxsize=None)
def transform_case(sc, seed, n):
    """(input vector, the oracle's forward transform, its coset evaluation of the first n / 4 coefficients): the entries on the
    library's stream give these"""
    data = synth.synth_packed(seed, n).tobytes()
    root = po.primitive_nth_root(n)
    x = sc.DeviceVector.from_bytes(data)
    fwd, lde = C.ntt(root, data, n), C.coset_evaluate(data[:16 * (n // 4)], n // 4, G, root, n)
    y, z, w = sc.DeviceVector(n), sc.DeviceVector(n), sc.DeviceVector(n)
    enqueue_transforms(sc, x, y, z, w, n, None)
    assert (y.to_bytes(), z.to_bytes(), w.to_bytes()) == (fwd, data, lde)
    return x, data, fwd, lde


def enqueue_transforms(sc, x, y, z, w, n, stream):
    rt = sc.fe_bytes(po.primitive_nth_root(n))
    lib, s = sc.lib(), handle_of(stream)
    sc._check(lib.sc_ntt_dev(x.ptr, y.ptr, n, rt, 0, s))
    sc._check(lib.sc_ntt_dev(y.ptr, z.ptr, n, rt, 1, s))
    sc._check(lib.sc_coset_evaluate_dev(x.ptr, n // 4, sc.fe_bytes(G), rt, n, w.ptr, s))


def test_mixed_entries_on_three_streams(sc, torch):
    """8 rounds on three caller streams: sc_ntt_dev forward and inverse at 2^14 and sc_coset_evaluate_dev 2^12 -> 2^14 on the first,
    the columns division with remainder of test_divmod_on_two_streams on the second, the coset columns division (exact operands) on
    the third.  Every round allocates its outputs as DeviceVectors and drops the round before's -- sc_vec_free hands them to
    release_after_streams with three seen streams busy -- after a copy on the same stream into memory of the test's own has kept
    their bytes.  All rounds' bytes are the expectations."""
    assert NTT_N // 4 == LDE_M
    rounds = 8
    s_ntt, s_div, s_coset = caller_streams(torch, 3)
    x, data, fwd, lde = transform_case(sc, 9600, NTT_N)
    div = divmod_case(sc, 9100)
    coset = coset_case(sc, 9400, True, True)
    fill_div = sc.DeviceVector.from_bytes(pdiv.SENTINEL * max(CQ_ELEMS, CR_ELEMS))
    fill_coset = sc.DeviceVector.from_bytes(cdiv.SENTINEL * coset.out_elems)
    kept = {name: keep_tensor(torch, rounds, n) for name, n in (("y", NTT_N), ("z", NTT_N), ("w", NTT_N), ("cq", CQ_ELEMS), ("cr", CR_ELEMS), ("coset", coset.out_elems))}
    sc.synchronize()
    torch.cuda.synchronize()
    live, handles = {}, []
    for rnd in range(rounds):
        y, z, w = sc.DeviceVector(NTT_N), sc.DeviceVector(NTT_N), sc.DeviceVector(NTT_N)
        enqueue_transforms(sc, x, y, z, w, NTT_N, s_ntt)
        for name, vec in (("y", y), ("z", z), ("w", w)):
            copy_on(sc, kept[name][rnd].data_ptr(), vec.ptr, NTT_N, s_ntt)
        live["ntt"] = (y, z, w)                        # the round before's are dropped here, their copies still in flight
        cq, cr = sc.DeviceVector(CQ_ELEMS), sc.DeviceVector(CR_ELEMS)
        copy_on(sc, cq.ptr, fill_div.ptr, CQ_ELEMS, s_div)
        copy_on(sc, cr.ptr, fill_div.ptr, CR_ELEMS, s_div)
        enqueue_divmod_columns(sc, div, (True, True), cq, cr, s_div)
        copy_on(sc, kept["cq"][rnd].data_ptr(), cq.ptr, CQ_ELEMS, s_div)
        copy_on(sc, kept["cr"][rnd].data_ptr(), cr.ptr, CR_ELEMS, s_div)
        live["div"] = (cq, cr)
        out = sc.DeviceVector(coset.out_elems)
        copy_on(sc, out.ptr, fill_coset.ptr, coset.out_elems, s_coset)
        handles.append(coset.enqueue(sc, out, s_coset))
        copy_on(sc, kept["coset"][rnd].data_ptr(), out.ptr, coset.out_elems, s_coset)
        live["coset"] = out
    torch.cuda.synchronize()
    live.clear()
    for rnd, handle in enumerate(handles):
        assert cdiv._words(handle)[:4] == coset.words, rnd
    for rnd in range(rounds):
        assert kept_bytes(kept["y"], rnd, NTT_N) == fwd, rnd
        assert kept_bytes(kept["z"], rnd, NTT_N) == data, rnd
        assert kept_bytes(kept["w"], rnd, NTT_N) == lde, rnd
        assert kept_bytes(kept["cq"], rnd, CQ_ELEMS) == div.want["cq"], rnd
        assert kept_bytes(kept["cr"], rnd, CR_ELEMS) == div.want["cr"], rnd
        assert kept_bytes(kept["coset"], rnd, coset.out_elems) == coset.want, rnd


# ---- more caller streams than the library tracks --------------------------------------------------------------------------------

def test_more_caller_streams_than_the_library_tracks(sc, torch):
    """csrc/core.h: SEEN_STREAMS = 8.  pick_stream records caller streams while the list holds at most that many, so the ninth stream
    is the last one recorded and brings the list above SEEN_STREAMS; from then on no stream is recorded, and the next
    release_after_streams waits for the whole device, forgets every stream and puts its buffer straight back.  Ten caller streams, two
    passes over them; each stream in each pass runs one sc_poly_divmod_dev at (m, nb) = (65, 100) and one sc_ntt_dev at 2^12 on operands
    of its own into outputs allocated for the call and freed right behind it (their bytes kept by a copy on the same stream).  All
    results are the oracle's.  Afterwards a division on the library's stream and a round of test_divmod_on_two_streams on two of the ten
    streams are right as well: the streams have to be picked up again after the list was cleared."""
    count, passes, m, nb, n = 10, 2, 65, 100, 1 << 12
    na, nr = m + nb - 1, nb - 1
    root = po.primitive_nth_root(n)
    streams = caller_streams(torch, count)
    ops = []
    for k in range(count):
        a, b = synth.synth_ints(9700 + 3 * k, na), synth.synth_ints(9701 + 3 * k, nb)
        b[-1] = b[-1] or 1
        q, r = cases.expected(a, b)                    # the oracle's long division
        assert pdiv.dev_divmod(sc, a, b) == (synth.pack_ints(q), synth.pack_ints(r))
        data = synth.synth_packed(9702 + 3 * k, n).tobytes()
        ops.append((sc.DeviceVector.from_ints(a), sc.DeviceVector.from_ints(b), sc.DeviceVector.from_bytes(data), synth.pack_ints(q), synth.pack_ints(r), C.ntt(root, data, n)))
    kept = {name: keep_tensor(torch, passes * count, elems) for name, elems in (("q", m), ("r", nr), ("y", n))}
    sc.synchronize()
    torch.cuda.synchronize()
    lib = sc.lib()
    for rnd in range(passes):
        for k, stream in enumerate(streams):
            da, db, dx = ops[k][:3]
            slot = rnd * count + k
            q, r, y = sc.DeviceVector(m), sc.DeviceVector(nr), sc.DeviceVector(n)
            sc._check(lib.sc_poly_divmod_dev(da.ptr, na, db.ptr, nb, q.ptr, r.ptr, handle_of(stream)))
            sc._check(lib.sc_ntt_dev(dx.ptr, y.ptr, n, sc.fe_bytes(root), 0, handle_of(stream)))
            for name, vec, elems in (("q", q, m), ("r", r, nr), ("y", y, n)):
                copy_on(sc, kept[name][slot].data_ptr(), vec.ptr, elems, stream)
            del q, r, y, vec                           # sc_vec_free, with this stream and the ones before it busy
    torch.cuda.synchronize()
    for rnd in range(passes):
        for k in range(count):
            slot = rnd * count + k
            assert kept_bytes(kept["q"], slot, m) == ops[k][3], (rnd, k)
            assert kept_bytes(kept["r"], slot, nr) == ops[k][4], (rnd, k)
            assert kept_bytes(kept["y"], slot, n) == ops[k][5], (rnd, k)
    a, b = synth.synth_ints(9700, na), synth.synth_ints(9701, nb)
    b[-1] = b[-1] or 1
    assert pdiv.dev_divmod(sc, a, b) == (ops[0][3], ops[0][4])
    divmod_rounds(sc, torch, [streams[9], streams[4]], 1)


# ---- the other class: entries with shared scratch buffers, ordered by events ----------------------------------------------------

class SharedScratchCase:
    """Operands of sc_coset_divide_dev (scratch slots 1 to 3) and of PolyTree.evaluate_columns / interpolate_columns (their batched
    transforms take their work buffer from scratch slot 0), resident.  The expectations need no run of these entries: the quotient
    is the one the numerator was built from (Python integers); the tree's values are those of the SINGLE-column entries on the
    library's stream, one column at a time (tests/test_gpu_tree_columns.py: the columns form equals them byte for byte), which
    interpolate back to the coefficients they came from and, at k = 1000, are the oracle's Horner values at a few points.  So the
    scratch slots are as small when the test proper starts as the single-column entries leave them."""

    def __init__(self, sc, seed, order, lq, k, cols):
        self.order, self.lq, self.k, self.cols = order, lq, k, cols
        q, d = synth.synth_ints(seed, lq), synth.synth_ints(seed + 1, DIVISOR_LEN)
        q[-1], d[-1] = q[-1] or 1, d[-1] or 1
        lhs = po.schoolbook_mul(q, d)
        self.na = len(lhs)
        self.lhs, self.d, self.quotient = sc.DeviceVector.from_ints(lhs), sc.DeviceVector.from_ints(d), synth.pack_ints(q)
        points = synth.synth_ints(seed + 2, k)
        assert len(set(points)) == k
        self.tree = sc.PolyTree(synth.pack_ints(points))
        polys = [synth.synth_ints(seed + 3 + c, k) for c in range(cols)]
        self.coeffs_bytes = b"".join(synth.pack_ints(f) for f in polys)
        self.coeffs = sc.DeviceVector.from_bytes(self.coeffs_bytes)
        values = [self.tree.evaluate(sc.DeviceVector.from_ints(f)) for f in polys]
        assert [self.tree.interpolate(v).to_bytes() for v in values] == [synth.pack_ints(f) for f in polys]
        self.values_bytes = b"".join(v.to_bytes() for v in values)
        if k <= 1000:
            for c in range(cols):
                for i in (0, 1, k // 2, k - 1):
                    assert synth.unpack_ints(self.values_bytes[16 * (c * k + i):16 * (c * k + i + 1)]) == [po.evaluate(polys[c], points[i])], (c, i)

    def enqueue(self, sc, stream):
        """the three calls on `stream`; nothing is read back"""
        lib, s, k, cols = sc.lib(), handle_of(stream), self.k, self.cols
        quo, vals, back = sc.DeviceVector(self.lq), sc.DeviceVector(cols * k), sc.DeviceVector(cols * k)
        exact = ctypes.c_int(-1)
        sc._check(lib.sc_coset_divide_dev(self.lhs.ptr, self.na, self.d.ptr, DIVISOR_LEN, sc.fe_bytes(G), sc.fe_bytes(po.primitive_nth_root(self.order)), self.order,
                                          quo.ptr, self.lq, ctypes.byref(exact), s))
        sc._check(lib.sc_polytree_evaluate_columns_dev(self.tree._h, self.coeffs.ptr, k, k, cols, self.tree.points.ptr, vals.ptr, k, s))
        sc._check(lib.sc_polytree_interpolate_columns_dev(self.tree._h, vals.ptr, k, cols, back.ptr, k, s))
        return exact, quo, vals, back

    @staticmethod
    def read(enqueued):
        exact, quo, vals, back = enqueued
        return exact.value, quo.to_bytes(), vals.to_bytes(), back.to_bytes()

    def expected(self):
        return 1, self.quotient, self.values_bytes, self.coeffs_bytes


def test_one_stream_rule_entries_ordered_by_events(sc, torch):
    """The documented way to use the entries that KEEP the one-stream rule on several streams: sc_coset_divide_dev and the tree's
    column evaluation and interpolation (k = 1000, 3 columns) on stream A; B waits for A on the device (an event) and runs the same
    entries on other, larger data (order 2^17, k = 5000, 5 columns: scratch slots 1 to 3 need 2 MiB where A left them at 1 MiB, and
    eight lanes of transforms of 2^14 need 2 MiB of slot 0 -- grow_buffer replaces a slot behind a device-wide wait); then
    sc.stream_join(B) and the same entries on the library's stream.  The host never waits for a stream in between (the entries'
    own waits stay).  Results: the quotients the numerators were built from, the values of the single-column entries on the library's
    stream, and the coefficients those values came from."""
    small = SharedScratchCase(sc, 9800, 1 << 12, (1 << 11) - 3, 1000, 3)
    large = SharedScratchCase(sc, 9820, 1 << 17, 3000, 5000, 5)
    third = SharedScratchCase(sc, 9840, 1 << 12, (1 << 11) - 3, 1000, 3)
    A, B = caller_streams(torch, 2)
    sc.synchronize()
    torch.cuda.synchronize()
    on_a = small.enqueue(sc, A)
    B.wait_stream(A)
    on_b = large.enqueue(sc, B)
    sc.stream_join(B.cuda_stream)
    on_library = third.enqueue(sc, None)
    torch.cuda.synchronize()
    assert small.read(on_a) == small.expected()
    assert large.read(on_b) == large.expected()
    assert third.read(on_library) == third.expected()

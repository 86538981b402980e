"""The elementwise vector entries at their edge shapes and operands (tests/vector_primitive_cases.py): every result against Python integer
arithmetic mod p, the folds against oracle/py_oracle.py's fold, byte for byte.  Operands carry 0, 1, p - 1, 2^64 and 2^119 + 1 at every
third place; every output has a 16-byte 0xff..ff sentinel (no residue) behind its stated length, and is all sentinel before an
out-of-place call, so an element left unwritten or written past the end shows.  tests/test_vector_primitive_cases_cpu.py proves each
"why" of the table from the constants of stark-anatomy_amd/csrc/core.hip without a GPU.

Which case reaches which branch, and why its shape does (pow2level(lo, hi, e) = lo[e & 4095] * hi[e >> 12]; get_pow gives the high
table pow2ceil((count >> 12) + 1) entries and keys its cache on that number):

  test_scale[n]                            scale_pow_kernel.  n = 1, 2: one thread, two.  255, 256, 257: the last partial wave, a full
                                           workgroup, one element in a second.  4095, 4096, 4097: the last exponent of the low table,
                                           the first of hi[1] (4096 elements already ask for a high table of 2); 8191, 8192, 8193:
                                           the same at hi[2] and a table of 4; 12289: hi[3], its last entry.  Factor 0 (0^0 = 1), 1,
                                           p - 1, a random one, and a root of order 8192, whose high table alternates 1 and -1
  test_scale_in_any_order                  get_pow's cache: one factor at 4097, 4095, 8193, 4096 (tables of 2, 1, 4, 2), then backwards;
                                           a second factor backwards first
  test_scale_slab[shape]                   scale_slab_kernel.  (1,1,1,0) one element; (12,8,32,16) the suite's old shape; (300,2,64,62)
                                           600 elements = two workgroups and 88 threads, the slab at the row's end; (3,4,2048,2044)
                                           exponents to 6143: hi[1]; (5,1,4097,4096) a row length that is no power of two, exponents
                                           4096, 8193, ... 20484: hi[1] to hi[5]; (2,4096,4096,0) whole rows, hi[0] and hi[1]
  test_twiddle_matrix[shape]               twiddle_matrix_kernel on the plan tables of `order`.  (64,32,0,32,2^12) exponents to 3969, with
                                           scale NULL, 1 (byte-equal: neither multiplies), random, p - 1; (1,1,0,0,2) the smallest
                                           order; (3,2,5,6,64) rows no power of two, row_base > 0; (8,4,1020,1020,2^21) exponents to
                                           1027 * 1023: hi[256]; (10,8,0,0,64) largest exponent 63 = order - 1, accepted
  test_twiddle_matrix_refusals             (9,8,0,1,64): largest exponent 64 = order, refused; rows = 0 (row_base = 0: rows - 1 wraps in
                                           the range check) and cols = 0: SC_OK, before any check
  test_fold_slab[shape,alpha]              fri_fold_slab_kernel.  (2,1,1,0) N = 2; (2,4,4,0); (64,16,64,32) the suite's old shape;
                                           (4,8,4096,4088) exponents 4088..4095 and 8184..8191: lo's last entries under hi[0] and hi[1];
                                           (16,1,1024,1023) one column, to 8191; (8,2,4096,4094) N = 2^15, exponents to 16383: hi[2], hi[3]
  test_fold_below_sixteen                  fri_fold_kernel at N = 2 and 4
  test_pointwise_mul[n]                    pointwise_mul_kernel at 1, 255, 256, 257 on all 225 pairs of edge residues; out = a, = b, = both
  test_pointwise_div[n]                    pointwise_div_kernel<16>: thread t of T = 256 * workgroups inverts elements t, t + T, ... (16 of
                                           them, ones past the end).  1: one thread with one divisor; 15, 16, 17: as many threads, 15
                                           ones each; 4095: one one in one thread; 4096: one workgroup, no padding; 4097: two
                                           workgroups, every thread half padding, thread 0 one more; 8193: three.  out = a, = b
  test_pointwise_div_zero_divisor[n]       the flag: a zero at 0, n / 2, n - 1 (the last real slot, next to the padding); only its own
                                           thread's quotients are spoiled; the next call succeeds
  test_pointwise_div_eight_per_thread      pointwise_div_kernel<8> (STARKCORE_DIV_K=8, read once per process): a child process
  test_axpy_shift[shape]                   axpy_shift_kernel: one element; 100 into 300 at the start, inside, at the very end; 256 into
                                           257 (a full workgroup, shifted by one); 255 at the end of 1024.  Sums that wrap past p
  test_degree_small                        vec_degree_kernel, one launch of 1 or 2 workgroups: the leader in each wave's first and last
                                           lane, the first, second and last of the four rows a thread loads, the second workgroup; a decoy below it
  test_degree_strided                      the second launch of sc_vec_degree_dev (top 2^16 zero) over DEGREE_MAX_BLOCKS * 1024 + 1024 + 5
                                           entries: the capped grid's `base += step`.  Leaders in the first step (3, step - 1) and the
                                           second (step, step + 3, the last entry); decoys in workgroups b +- DEGREE_SLOTS, which share
                                           the leader's result word, and at step - 1
  test_degree_columns_strided              vec_degree_cols_kernel: n = 64 * 1024 + 1024 + 5 puts part 0 into a second step; junk between
  test_degree_columns_second_launch        DEGREE_COLS_PER_LAUNCH + 3 columns of 3 entries: a second launch at d_v + done * ld
  test_mpoly[case,stream]                  mpoly_eval_kernel: exponent 255, exponent 0 everywhere, 255 variables, no term; coefficient
                                           bytes 8192 (kernel arguments) and 8208 (copied), exponent bytes 8194 under 7712 coefficient
                                           bytes (copied); the library's stream and a caller's (the path that waits)
  test_mpoly_turned[case,stream]           `where`: n = 1, 2, 256; turns n - 1, and n + 3 = 3 mod n
  test_gather[k]                           gather_kernel: k = 0, 1, 256, 257, 1000 with repeats and the last index"""
import ctypes
import os
import subprocess
import sys

import pytest

from oracle import py_oracle as po
import vector_primitive_cases as vc
import vector_primitive_div_worker as divw
from vector_primitive_div_worker import blank, dev, read

pytestmark = pytest.mark.gpu
P = po.P
SC_OK, SC_ERR_NOT_POW2, SC_ERR_DIV_ZERO, SC_ERR_BAD_ARG = 0, -2, -5, -6
NOT_RESIDUES = (P, P + 1, (1 << 128) - 1)


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


@pytest.fixture(scope="module")
def caller_stream(sc):
    import torch
    return torch.cuda.Stream(device=torch.device("cuda", 0))


def fe(v):
    return None if v is None else int(v).to_bytes(16, "little")


def untouched(vec):
    assert vec.to_bytes() == vc.SENTINEL * vec.n, "a refused or empty call wrote something"


# ---- 1. the two-level power table -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", vc.SCALE_SIZES)
def test_scale(sc, n):
    lib = sc.lib()
    vals = vc.scale_input(n)
    for name, f in vc.SCALE_FACTORS:
        want = vc.scale_expected(n, f)
        src, out = dev(sc, vals), blank(sc, n)
        assert lib.sc_scale_dev(src.ptr, out.ptr, n, fe(f), None) == SC_OK
        assert read(out, n) == want, (n, name)
        assert read(src, n) == list(vals)
        assert lib.sc_scale_dev(src.ptr, src.ptr, n, fe(f), None) == SC_OK         # in place
        assert read(src, n) == want, (n, name, "in place")
    if n > 1:
        assert want[0] == vals[0] and any(want[1:])                                # (the last factor is no zero)


def test_scale_refuses_a_factor_that_is_no_residue(sc):
    lib = sc.lib()
    n = 257
    src, out = dev(sc, vc.scale_input(n)), blank(sc, n)
    for f in NOT_RESIDUES:
        assert lib.sc_scale_dev(src.ptr, out.ptr, n, fe(f), None) == SC_ERR_BAD_ARG, f
        assert lib.sc_scale_slab_dev(src.ptr, out.ptr, 32, 8, 32, 16, fe(f), None) == SC_ERR_BAD_ARG, f
        untouched(out)
    assert lib.sc_scale_dev(src.ptr, out.ptr, 0, fe(P), None) == SC_OK              # nothing to do comes first, as everywhere
    untouched(out)
    assert lib.sc_scale_dev(src.ptr, out.ptr, n, fe(P - 1), None) == SC_OK          # the largest residue is taken
    assert read(out, n) == vc.scale_expected(n, P - 1)


def test_scale_in_any_order(sc):
    """sizes that share and outgrow one factor's cached tables: the results depend on the size alone"""
    lib = sc.lib()
    forward = list(vc.SCALE_ORDER_RUN)
    for f, orders in zip(vc.SCALE_ORDER_FACTORS, ((forward, forward[::-1]), (forward[::-1], forward))):
        for order in orders:
            for n in order:
                src, out = dev(sc, vc.scale_input(n)), blank(sc, n)
                assert lib.sc_scale_dev(src.ptr, out.ptr, n, fe(f), None) == SC_OK
                assert read(out, n) == vc.scale_expected(n, f), (n, order)


@pytest.mark.parametrize("shape", vc.SLAB_SHAPES)
def test_scale_slab(sc, shape):
    lib = sc.lib()
    rows, cols, row_len, col_base = shape
    n = rows * cols
    vals = vc.slab_input(shape)
    for name, f in vc.SLAB_FACTORS:
        want = vc.slab_expected(shape, f)
        src, out = dev(sc, vals), blank(sc, n)
        assert lib.sc_scale_slab_dev(src.ptr, out.ptr, rows, cols, row_len, col_base, fe(f), None) == SC_OK
        assert read(out, n) == want, (shape, name)
        assert lib.sc_scale_slab_dev(src.ptr, src.ptr, rows, cols, row_len, col_base, fe(f), None) == SC_OK
        assert read(src, n) == want, (shape, name, "in place")


def test_scale_slab_refusals_and_empty_slabs(sc):
    lib = sc.lib()
    src, out = dev(sc, vc.operands(4190, 12 * 8)), blank(sc, 12 * 8)
    for rows, cols, row_len, col_base in vc.SLAB_REFUSED:
        assert lib.sc_scale_slab_dev(src.ptr, out.ptr, rows, cols, row_len, col_base, fe(vc.RANDOM[0]), None) == SC_ERR_BAD_ARG
        untouched(out)
    for rows, cols, row_len, col_base in vc.SLAB_NOTHING:
        assert lib.sc_scale_slab_dev(src.ptr, out.ptr, rows, cols, row_len, col_base, fe(vc.RANDOM[0]), None) == SC_OK
        untouched(out)


@pytest.mark.parametrize("shape", vc.TWIDDLE_SHAPES)
def test_twiddle_matrix(sc, shape):
    lib = sc.lib()
    rows, cols, row_base, col_base, order = shape
    n = rows * cols
    root = fe(po.primitive_nth_root(order))
    raw = {}
    for name, scale in vc.TWIDDLE_SCALES:
        data = dev(sc, vc.twiddle_input(shape))
        assert lib.sc_twiddle_matrix_dev(data.ptr, rows, cols, row_base, col_base, root, order, fe(scale), None) == SC_OK, (shape, name)
        assert read(data, n) == vc.twiddle_expected(shape, scale), (shape, name)
        raw[name] = data.to_bytes()
    assert raw["no scale"] == raw["scale one"]


def test_twiddle_matrix_refusals(sc):
    lib = sc.lib()
    rows, cols, row_base, col_base, order = vc.TWIDDLE_REFUSED
    root = fe(po.primitive_nth_root(order))
    data = blank(sc, rows * cols)
    assert lib.sc_twiddle_matrix_dev(data.ptr, rows, cols, row_base, col_base, root, order, None, None) == SC_ERR_BAD_ARG
    untouched(data)
    for rows, cols, row_base, col_base, order in vc.TWIDDLE_NOTHING:
        assert lib.sc_twiddle_matrix_dev(data.ptr, rows, cols, row_base, col_base, root, order, None, None) == SC_OK, (rows, cols, row_base, col_base)
        untouched(data)


FOLD_SLAB_CASES = [(s, a) for s in vc.FOLD_SLAB_SHAPES for a in range(len(vc.ALPHAS))
                   if s != vc.FOLD_SLAB_SHAPES[-1] or a >= 2]                       # the 2^15 codeword: p - 1 and random (a second of oracle each)


@pytest.mark.parametrize("shape,a", FOLD_SLAB_CASES)
def test_fold_slab(sc, shape, a):
    lib = sc.lib()
    rows, cols, R, col_base = shape
    name, alpha = vc.ALPHAS[a]
    N = rows * R
    half = rows // 2 * cols
    src, out = dev(sc, vc.fold_slab_input(shape)), blank(sc, half)
    assert lib.sc_fri_fold_slab_dev(src.ptr, rows, cols, R, col_base, fe(alpha), fe(vc.G), fe(po.primitive_nth_root(N)), out.ptr, None) == SC_OK
    assert read(out, half) == vc.fold_slab_expected(shape, alpha), (shape, name)
    assert read(src, rows * cols) == vc.fold_slab_input(shape)


def test_fold_below_sixteen(sc):
    lib = sc.lib()
    for N in vc.FOLD_SIZES:
        for name, alpha in vc.ALPHAS:
            src, out = dev(sc, vc.codeword(N)), blank(sc, N // 2)
            assert lib.sc_fri_fold_dev(src.ptr, N, fe(alpha), fe(vc.G), fe(po.primitive_nth_root(N)), out.ptr, None) == SC_OK
            assert read(out, N // 2) == list(vc.fold_expected(N, alpha)), (N, name)


# ---- 2. pointwise product and quotient -----------------------------------------------------------------------------------------

def mul_every_way(sc, a, b):
    lib = sc.lib()
    n = len(a)
    want = [x * y % P for x, y in zip(a, b)]
    for alias in ("none", "a", "b"):
        da, db = dev(sc, a), dev(sc, b)
        out = {"none": blank(sc, n), "a": da, "b": db}[alias]
        assert lib.sc_pointwise_mul_dev(da.ptr, db.ptr, out.ptr, n, None) == SC_OK
        assert read(out, n) == want, (n, alias)
    da = dev(sc, a)                                                                 # d_out = d_a = d_b: squares
    assert lib.sc_pointwise_mul_dev(da.ptr, da.ptr, da.ptr, n, None) == SC_OK
    assert read(da, n) == [x * x % P for x in a], n


@pytest.mark.parametrize("n", vc.MUL_SIZES)
def test_pointwise_mul(sc, n):
    if n == 1:
        for x, y in vc.mul_single_pairs():
            mul_every_way(sc, [x], [y])
    else:
        mul_every_way(sc, *vc.mul_operands(n))


@pytest.mark.parametrize("n", vc.DIV_SIZES[16])
def test_pointwise_div(sc, n):
    divw.check_quotients(sc, n)


@pytest.mark.parametrize("n", vc.DIV_ZERO_SIZES[16])
def test_pointwise_div_zero_divisor(sc, n):
    assert os.environ.get("STARKCORE_DIV_K", "16") != "8"
    for place in vc.div_zero_places(n):
        divw.check_zero_divisor(sc, n, 16, place)


def test_pointwise_div_eight_per_thread(sc):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vector_primitive_div_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, STARKCORE_DIV_K="8"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok: pointwise_div_kernel<8>" in r.stdout


# ---- 3. axpy with a shift ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", vc.AXPY_SHAPES)
def test_axpy_shift(sc, shape):
    lib = sc.lib()
    n_acc, n_src, shift = shape
    acc0, src0 = vc.axpy_operands(shape)
    for name, w in vc.WEIGHTS:
        acc, src = dev(sc, acc0), dev(sc, src0)
        assert lib.sc_axpy_shift_dev(acc.ptr, n_acc, src.ptr, n_src, shift, fe(w), None) == SC_OK
        got = read(acc, n_acc)
        assert got == vc.axpy_expected(shape, w), (shape, name)
        assert got[:shift] == list(acc0[:shift]) and got[shift + n_src:] == list(acc0[shift + n_src:])
        assert read(src, n_src) == list(src0)
        if shift == 0 and n_src <= n_acc:                                           # d_acc == d_src: acc[j] * (1 + w)
            both = dev(sc, acc0)
            assert lib.sc_axpy_shift_dev(both.ptr, n_acc, both.ptr, n_src, 0, fe(w), None) == SC_OK
            assert read(both, n_acc) == [v * (1 + w) % P for v in acc0[:n_src]] + list(acc0[n_src:]), (shape, name)


def test_axpy_shift_refusals(sc):
    lib = sc.lib()
    for n_acc, n_src, shift, w in vc.AXPY_REFUSED:
        acc0 = vc.operands(4690, n_acc)
        acc, src = dev(sc, acc0), dev(sc, vc.operands(4691, n_src))
        assert lib.sc_axpy_shift_dev(acc.ptr, n_acc, src.ptr, n_src, shift, fe(w), None) == SC_ERR_BAD_ARG, (n_acc, n_src, shift)
        assert read(acc, n_acc) == acc0
    assert lib.sc_axpy_shift_dev(acc.ptr, n_acc, src.ptr, 0, 5, fe(1), None) == SC_OK
    assert lib.sc_axpy_shift_dev(acc.ptr, n_acc, src.ptr, 0, n_acc + 7, fe(P), None) == SC_OK      # nothing to add: nothing is looked at
    assert read(acc, n_acc) == acc0


# ---- 4. degrees --------------------------------------------------------------------------------------------------------------------

def degree_of(sc, ptr, n):
    out = (ctypes.c_int64 * 2)(77, 77)
    assert sc.lib().sc_vec_degree_dev(ptr, n, out, None) == SC_OK
    assert out[1] == 77
    return out[0]


def test_degree_small(sc):
    for n, lead, decoy in vc.degree_small_cases():
        vals = [0] * n
        if lead >= 0:
            vals[lead] = vc.NONZERO[(n + lead) % 4]
        if decoy is not None:
            vals[decoy] = vc.NONZERO[(n + decoy + 1) % 4]
        v = dev(sc, vals)                                                           # (the sentinel behind the vector is non-zero: it is not to be read)
        assert degree_of(sc, v.ptr, n) == lead == po.degree(vals), (n, lead, decoy)


def test_degree_strided(sc):
    lib = sc.lib()
    n = vc.DEGREE_STRIDED_N
    v = sc.DeviceVector.zeros(n)

    def put(i, value):
        sc._check(lib.sc_vec_upload(v._h, i, fe(value), 1))

    assert degree_of(sc, v.ptr, n) == -1
    for k, (lead, same, other) in enumerate(vc.degree_strided_cases()):
        places = [lead] + same + other
        for j, i in enumerate(places):
            put(i, vc.NONZERO[(k + j) % 4])
        assert degree_of(sc, v.ptr, n) == lead, (lead, same, other)
        assert degree_of(sc, v.ptr, vc.DEGREE_STRIDED_SCANNED) == lead               # the same entries as the top window and the rest of a shorter vector
        for i in places:
            put(i, 0)
    assert degree_of(sc, v.ptr, n) == -1
    put(n - vc.DEGREE_TOP, 1)                                                       # the first entry of the top window: found by the first launch
    put(vc.DEGREE_STEP + 3, 1)
    assert degree_of(sc, v.ptr, n) == n - vc.DEGREE_TOP


def degrees_of_columns(sc, ptr, n, ld, cols):
    out = (ctypes.c_int64 * (cols + 1))(*([77] * (cols + 1)))
    assert sc.lib().sc_vec_degree_columns_dev(ptr, n, ld, cols, out, None) == SC_OK
    assert out[cols] == 77
    return list(out[:cols])


def test_degree_columns_strided(sc):
    n, gap, cols = (vc.DEGREE_COLS_STRIDED[k] for k in ("n", "gap", "cols"))
    ld = n + gap
    raw = bytearray(16 * ld * cols)
    want = []
    for c, (lead, decoy) in enumerate(vc.DEGREE_COLS_STRIDED_LEADS):
        for j, i in enumerate([i for i in (lead, decoy) if i is not None and i >= 0]):
            raw[16 * (c * ld + i):16 * (c * ld + i + 1)] = fe(vc.NONZERO[(c + j) % 4])
        raw[16 * (c * ld + n):16 * (c + 1) * ld] = b"".join(fe(vc.NONZERO[(c + j) % 4]) for j in range(gap))      # junk between the columns
        want.append(lead)
    v = sc.DeviceVector.from_bytes(bytes(raw))
    assert degrees_of_columns(sc, v.ptr, n, ld, cols) == want
    assert degrees_of_columns(sc, v.ptr + 16 * ld, n, ld, 2) == want[1:]


def test_degree_columns_second_launch(sc):
    n, gap, cols = (vc.DEGREE_COLS_MANY[k] for k in ("n", "gap", "cols"))
    v = sc.DeviceVector.from_ints(vc.degree_cols_many_values())
    assert degrees_of_columns(sc, v.ptr, n, n + gap, cols) == vc.degree_cols_many_expected()


# ---- 5. multivariate evaluation ---------------------------------------------------------------------------------------------------

def stream_handle(sc, which, caller_stream):
    if which == "library stream":
        return None
    sc.synchronize()                                                                # the operands were uploaded on the library's stream
    return ctypes.c_void_p(caller_stream.cuda_stream)


def exps_bytes(terms):
    return bytes(e for exps, _ in terms for e in exps) or bytes(1)


def coef_bytes(terms):
    return vc.pack([c for _, c in terms]) or bytes(16)


STREAMS = ("library stream", "caller's stream")
_mpoly_want = {}


@pytest.mark.parametrize("which", STREAMS)
@pytest.mark.parametrize("case", list(vc.mpoly_cases()))
def test_mpoly(sc, caller_stream, case, which):
    lib = sc.lib()
    nvars, n, terms = vc.mpoly_cases()[case]
    vals = vc.mpoly_values(4750 + nvars, nvars, n)
    if case not in _mpoly_want:
        _mpoly_want[case] = vc.mpoly_expected(vals, n, terms)
    want = _mpoly_want[case]
    if not terms:
        assert want == [0] * n
    dv, out, again = dev(sc, [v for col in vals for v in col]), blank(sc, n), blank(sc, n)
    st = stream_handle(sc, which, caller_stream)
    assert lib.sc_mpoly_eval_dev(dv.ptr, nvars, n, exps_bytes(terms), coef_bytes(terms), len(terms), out.ptr, st) == SC_OK
    sc.synchronize()
    assert read(out, n) == want, (case, which)
    read(dv, nvars * n)                                                             # converted in place, not past its end
    st = stream_handle(sc, which, caller_stream)
    assert lib.sc_mpoly_eval_ex_dev(dv.ptr, nvars, n, exps_bytes(terms), coef_bytes(terms), len(terms), again.ptr, 1, st) == SC_OK
    sc.synchronize()
    assert read(again, n) == want, (case, which, "values converted already")


@pytest.mark.parametrize("which", STREAMS)
@pytest.mark.parametrize("case", list(vc.MPOLY_ROT_CASES))
def test_mpoly_turned(sc, caller_stream, case, which):
    lib = sc.lib()
    n, turns = vc.MPOLY_ROT_CASES[case]
    stored, want = vc.mpoly_rot_expected(n, turns)
    nv = len(vc.MPOLY_ROT_SRC)
    dv = sc.DeviceVector.from_bytes(vc.pack(stored[0] + stored[1]) + vc.SENTINEL * ((nv - 2) * n + 1))
    out, again = blank(sc, n), blank(sc, n)
    src = (ctypes.c_uint32 * nv)(*vc.MPOLY_ROT_SRC)
    rot = (ctypes.c_uint64 * nv)(0, 0, turns[0], turns[1], 0)
    for converted, dst in ((0, out), (1, again)):
        st = stream_handle(sc, which, caller_stream)
        assert lib.sc_mpoly_eval_rot_dev(dv.ptr, nv, n, exps_bytes(vc.MPOLY_ROT_TERMS), coef_bytes(vc.MPOLY_ROT_TERMS), len(vc.MPOLY_ROT_TERMS), dst.ptr,
                                         converted, src, rot, st) == SC_OK
        sc.synchronize()
        assert read(dst, n) == want, (case, which, converted)
    assert dv.to_bytes(2 * n) == vc.SENTINEL * ((nv - 2) * n + 1)                   # the places of turned and absent variables hold nothing


def test_mpoly_refusals(sc):
    lib = sc.lib()
    n = 255
    stored = vc.mpoly_values(4790, 2, n)
    nv = len(vc.MPOLY_ROT_SRC)
    before = vc.pack(stored[0] + stored[1]) + vc.SENTINEL * ((nv - 2) * n + 1)
    dv, out = sc.DeviceVector.from_bytes(before), blank(sc, n)
    src = (ctypes.c_uint32 * nv)(*vc.MPOLY_ROT_SRC)
    rot = (ctypes.c_uint64 * nv)(0, 0, 3, 1, 0)
    terms = vc.MPOLY_ROT_TERMS
    # turned variables on 255 points
    assert lib.sc_mpoly_eval_rot_dev(dv.ptr, nv, n, exps_bytes(terms), coef_bytes(terms), len(terms), out.ptr, 0, src, rot, None) == SC_ERR_NOT_POW2
    # 256 variables (of one point each would do; the count is refused before anything is read)
    assert lib.sc_mpoly_eval_dev(dv.ptr, 256, 1, bytes(256), coef_bytes(terms[:1]), 1, out.ptr, None) == SC_ERR_BAD_ARG
    # a coefficient that is no residue
    for bad in NOT_RESIDUES:
        two = [((1, 0), 5), ((0, 1), bad)]
        assert lib.sc_mpoly_eval_dev(dv.ptr, 2, n, exps_bytes(two), b"".join(fe(c) for _, c in two), 2, out.ptr, None) == SC_ERR_BAD_ARG, bad
    sc.synchronize()
    untouched(out)
    assert dv.to_bytes() == before                                                  # not converted either


# ---- 6. gather ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", vc.GATHER_COUNTS)
def test_gather(sc, k):
    lib = sc.lib()
    vals = vc.operands(4900, vc.GATHER_N)
    v = sc.DeviceVector.from_ints(vals)
    idx = vc.gather_indices(k)
    arr = (ctypes.c_uint64 * max(k, 1))(*idx)
    host = ctypes.create_string_buffer(vc.SENTINEL * (k + 1))
    assert lib.sc_vec_gather(v._h, arr, k, host) == SC_OK
    assert host.raw[:16 * (k + 1)] == vc.pack([vals[i] for i in idx]) + vc.SENTINEL, k
    if k:
        arr[k // 2] = vc.GATHER_N                                                   # one index past the end
        host = ctypes.create_string_buffer(vc.SENTINEL * (k + 1))
        assert lib.sc_vec_gather(v._h, arr, k, host) == SC_ERR_BAD_ARG
        assert host.raw[:16 * (k + 1)] == vc.SENTINEL * (k + 1)
    assert v.to_bytes() == vc.pack(vals)

"""sc_randomized_columns_dev: the randomized trace matrix of a batch of proofs in one launch -- every member's trace columns with the
randomizer rows sampled behind them, and (rows = 0, one register) the members' randomizer polynomials.  The cases of the CPU walk
(tests/randomize_cases.py) through the entry against Python integers; equality with FastStark._randomized_columns and
sampled_polynomial on the same bytes; the argument errors; the empty shapes."""
import ctypes

import pytest

import randomize_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import starkcore as sc                                          # noqa: E402
from algebra import Field                                       # noqa: E402
from fast_stark import DeviceTrace, FastStark, sampled_polynomial    # noqa: E402
from starkcore import DeviceVector                              # noqa: E402

field = Field.main()
SC_ERR_BAD_ARG = -6


def call(trace_ptr, rows, ld_trace, members, registers, draws, stride, extra, width, out_ptr, ld_out):
    return sc.lib().sc_randomized_columns_dev(trace_ptr, rows, ld_trace, members, registers, draws, stride, extra, width, out_ptr, ld_out, None)


@pytest.mark.parametrize("case", rc.all_cases(), ids=rc.case_id)
def test_matrix_matches_python(case):
    c = rc.Case(*case)
    out = DeviceVector.from_bytes(c.blank_output())
    trace = DeviceVector.from_bytes(c.trace) if c.rows else None
    sc._check(call(trace.ptr if trace else None, c.rows, c.ld_trace, c.members, c.registers, c.draws, c.draws_stride, c.extra, c.width, out.ptr, c.ld_out))
    assert rc.unpack(out.to_bytes()) == c.want
    if trace:
        assert trace.to_bytes() == c.trace


def test_equals_the_per_register_code_on_the_same_bytes():
    """three members of a two-register trace: the matrix is FastStark._randomized_columns member by member, and the rows = 0 form is
    sampled_polynomial member by member, from one buffer of K equal blocks laid out as prove_batch lays it out"""
    import random
    rng = random.Random(11)
    K, R, rows, count = 3, 2, 28, 40
    stark = FastStark(field, 4, 2, 2, R, rows)
    extra = stark.num_randomizers
    block = 17 * (extra * R + count)
    raw = bytes(rng.getrandbits(8) for _ in range(K * block))
    columns = [[rng.randrange(rc.P) for _ in range(rows)] for _ in range(K * R)]
    source = DeviceVector.from_bytes(b"".join(rc.pack(column) for column in columns))
    n = rows + extra
    out, sampled = DeviceVector(K * R * n), DeviceVector(K * count)
    draws = (ctypes.c_char * len(raw)).from_buffer_copy(raw)
    at = ctypes.addressof(draws)
    sc._check(call(source.ptr, rows, rows, K, R, at, block, extra, 17, out.ptr, n))
    sc._check(call(None, 0, 0, K, 1, at + 17 * extra * R, block, count, 17, sampled.ptr, count))
    for m in range(K):
        mine = raw[m * block:(m + 1) * block]
        trace = DeviceTrace.from_packed([rc.pack(columns[m * R + s]) for s in range(R)], field)
        for together in (False, True):
            want = stark._randomized_columns(trace, mine[:17 * extra * R], together)
            assert b"".join(w.vec.to_bytes() for w in want) == out.to_bytes(m * R * n, R * n), (m, together)
        polynomial = sampled_polynomial(mine[17 * extra * R:], field)
        assert len(polynomial) == count and polynomial.vec.to_bytes(0, count) == sampled.to_bytes(m * count, count), m


def test_bad_arguments_are_refused_and_nothing_is_written():
    rows, extra, members, registers, width = 5, 3, 2, 2, 17
    n, block = rows + extra, extra * registers * width
    trace = DeviceVector.from_bytes(rc.pack([7] * (members * registers * rows)))
    blank = rc.pack([rc.SENTINEL] * (members * registers * n))
    out = DeviceVector.from_bytes(blank)
    draws = bytes(members * block)
    good = dict(trace_ptr=trace.ptr, rows=rows, ld_trace=rows, members=members, registers=registers, draws=draws, stride=block, extra=extra, width=width,
                out_ptr=out.ptr, ld_out=n)
    wrong = [dict(ld_out=n - 1), dict(ld_trace=rows - 1), dict(width=0), dict(width=33), dict(stride=block - 1), dict(out_ptr=None), dict(trace_ptr=None),
             dict(draws=None)]
    for change in wrong:
        assert call(**dict(good, **change)) == SC_ERR_BAD_ARG, change
        assert out.to_bytes() == blank, change
    # a single member's stride is not looked at; neither is a null trace without rows or null draws without randomizers
    assert call(**dict(good, members=1, stride=0)) == 0
    assert call(**dict(good, trace_ptr=None, rows=0, ld_trace=0, ld_out=extra)) == 0
    assert call(**dict(good, draws=None, extra=0, ld_out=rows)) == 0
    sc._check(call(**good))
    assert rc.unpack(out.to_bytes()) == ([7] * rows + [0] * extra) * (members * registers)


def test_empty_shapes_do_nothing():
    out = DeviceVector.from_bytes(rc.pack([rc.SENTINEL] * 8))
    for members, registers, rows, extra in ((0, 2, 1, 1), (2, 0, 1, 1), (2, 2, 0, 0)):
        assert call(None, rows, rows, members, registers, None, 0, extra, 17, None, rows + extra) == 0
        assert call(None, rows, rows, members, registers, None, 0, extra, 99, out.ptr, 0) == 0       # before any argument is looked at
    assert rc.unpack(out.to_bytes()) == [rc.SENTINEL] * 8

"""sc_poly_mul_dev, sc_poly_mul_columns_dev and sc_poly_pow_dev in flight on three HIP streams at once: include/starkcore.h documents
them as free of the one-stream rule (the temporaries are the call's own, csrc/core.h: PoolTmpAsync).  A dozen calls of different
shapes -- one-pass and two-pass transforms, shared and per-column multiplicands, sets of columns -- are computed first one at a time
on the library's stream and pinned to exact integer products (tests/emu/poly_multiply_cases.py); then the same calls are enqueued
round-robin on three caller streams with no host wait in between, each operand copied into place ON the stream that uses it, and
every output must equal the single-stream bytes, the sentinels behind and between the outputs included."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import poly_multiply_cases as cases
import synth
import test_gpu_poly_multiply as pmul          # the helpers of the single-stream tests of the same entries, not copies of them

pytestmark = pytest.mark.gpu
S, GUARD = pmul.SENTINEL, pmul.GUARD


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


def handle_of(stream):
    return ctypes.c_void_p(stream.cuda_stream)


class Call:
    """one call: staged operands (complete before anything is enqueued), operands and output of its own, what the output must hold"""

    def __init__(self, sc, kind, *shape):
        self.kind, self.shape = kind, shape
        if kind == "mul":
            na, nb = shape
            a, b = synth.synth_ints(9990 + na, na), synth.synth_ints(9991 + nb, nb)
            single = pmul.dev_mul(sc, a, b)
            assert single == synth.pack_ints(cases.exact_product(a, b))
            self.staged = [sc.DeviceVector.from_ints(a), sc.DeviceVector.from_ints(b)]
            self.want = single + S * GUARD
        elif kind == "columns":
            na, nb, cols, shared = shape
            columns, others = cases.column_operands(na, nb, cols)
            self.ld_a, self.ld_b, self.ld_out = na + 3, 0 if shared else nb + 1, na + nb + 1
            single = pmul.dev_mul_columns(sc, columns, others[0] if shared else others, self.ld_a, self.ld_b, self.ld_out)
            assert single == [synth.pack_ints(cases.exact_product(a, others[0] if shared else b)) for a, b in zip(columns, others)]
            self.staged = [pmul.matrix_of(sc, columns, na, self.ld_a),
                           sc.DeviceVector.from_ints(others[0]) if shared else pmul.matrix_of(sc, others, nb, self.ld_b)]
            self.want = b"".join(x + S * (self.ld_out - na - nb + 1) for x in single) + S * GUARD
        else:
            na, exponent = shape
            a = synth.synth_ints(9992 + na, na)
            single = pmul.dev_pow(sc, a, exponent)
            assert single == synth.pack_ints(cases.exact_power(a, exponent))
            self.staged = [sc.DeviceVector.from_ints(a)]
            self.want = single + S * GUARD
        self.operands = [sc.DeviceVector(v.n) for v in self.staged]
        self.out = sc.DeviceVector.from_bytes(S * (len(self.want) // 16))

    def enqueue(self, sc, stream):
        h = handle_of(stream)
        lib = sc.lib()
        for dst, src in zip(self.operands, self.staged):        # the operands become complete on the stream that uses them
            sc._check(lib.sc_memcpy_dev(ctypes.c_void_p(int(dst.ptr)), ctypes.c_void_p(int(src.ptr)), src.n, h))
        if self.kind == "mul":
            na, nb = self.shape
            sc._check(lib.sc_poly_mul_dev(self.operands[0].ptr, na, self.operands[1].ptr, nb, self.out.ptr, h))
        elif self.kind == "columns":
            na, nb, cols, _ = self.shape
            sc._check(lib.sc_poly_mul_columns_dev(self.operands[0].ptr, na, self.ld_a, cols, self.operands[1].ptr, nb, self.ld_b, self.out.ptr, self.ld_out, h))
        else:
            na, exponent = self.shape
            sc._check(lib.sc_poly_pow_dev(self.operands[0].ptr, na, exponent, self.out.ptr, h))


def test_three_streams(sc):
    import torch
    calls = [
        Call(sc, "mul", 2049, 2049), Call(sc, "columns", 33, 33, 5, True), Call(sc, "pow", 33, 5),
        Call(sc, "pow", 1025, 4), Call(sc, "mul", 33, 32), Call(sc, "columns", 4097, 100, 3, False),
        Call(sc, "columns", 5, 4, 16, False), Call(sc, "pow", 2, 256), Call(sc, "mul", 4097, 8),
        Call(sc, "mul", 5, 5), Call(sc, "columns", 4097, 100, 3, True), Call(sc, "pow", 4, 3),
    ]
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    sc.synchronize()                                            # the staged operands and the sentinels are in place
    sc.set_tuning("div_cols_launch_log", 14)                    # 4097 x 100 in sets of 2 and 1 columns, everything else whole
    try:
        for rnd in range(2):                                    # the second round finds the first one's temporaries in the pool
            for i, call in enumerate(calls):
                call.enqueue(sc, streams[(i + rnd) % 3])
            torch.cuda.synchronize()
            for i, call in enumerate(calls):
                assert call.out.to_bytes() == call.want, (rnd, i, call.kind, call.shape)
                sc._check(sc.lib().sc_vec_upload(call.out._h, 0, S * call.out.n, call.out.n))
            sc.synchronize()
    finally:
        sc.set_tuning("div_cols_launch_log", 26)

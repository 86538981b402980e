"""The eight-element batch kernels with the top-limb field corrections (ntt_pass_kernel_fixed8, then ntt_pass_redo8_kernel on the tiles
it flagged): sc_set_tuning("fast_fixups", 1) -- the default --, 0 (exact arithmetic on every tile) and 2 (both kernels on every tile)
agree bit for bit, forward and inverse, on random data and on inputs that flag every tile of a pass, and every column equals the C oracle.
A three-pass transform, whose in-place middle pass takes the exact kernel alone, equals sc_ntt_dev column by column."""
import functools

import numpy as np
import pytest

from oracle import py_oracle as po
import synth

pytestmark = pytest.mark.gpu
C = po.C
P = po.P

# (log2 length, columns).  Passes: 2^17 x 8 (9,3) (8,4) | 2^19 (10,2) (9,3) | 2^20 (10,2) (10,2); three columns of 2^17 are too few
# for 2^12-element tiles and take the four-element kernels (the knob must not matter there either).
SHAPES = [(17, 3), (17, 8), (19, 2), (20, 2)]
INPUTS = ["random", "zero", "p-1", "alternating", "halves 0|1", "halves p-1|2^32"]


def _fe(v, count):
    a = np.empty((count, 2), dtype=np.uint64)
    a[:, 0] = v & ((1 << 64) - 1)
    a[:, 1] = v >> 64
    return a


@functools.lru_cache(maxsize=None)
def _column(logn, name):
    """one column of 2^logn elements, packed; every column of a case carries the same pattern (random: column 0, the others differ)"""
    n = 1 << logn
    if name == "random":
        return synth.synth_packed(2600 + logn, n).tobytes()
    if name == "zero":
        return _fe(0, n).tobytes()
    if name == "p-1":
        return _fe(P - 1, n).tobytes()
    if name == "alternating":
        a = _fe(0, n)
        a[1::2, 0] = 1
        return a.tobytes()
    lo, hi = (0, 1) if name == "halves 0|1" else (P - 1, 1 << 32)       # u - v = -1: every wave of pass 0 flags through sub | (p-1) + 2^32: through add
    return _fe(lo, n // 2).tobytes() + _fe(hi, n // 2).tobytes()


@functools.lru_cache(maxsize=None)
def _want(logn, name, inverse):
    n = 1 << logn
    return (C.intt if inverse else C.ntt)(po.primitive_nth_root(n), _column(logn, name), n)


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    starkcore.set_tuning("fast_fixups", 1)


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.int64).copy()).to(torch.device("cuda", 0))


def _columns(sc, x, n, cols, rt, inverse, mode):
    import torch
    y = torch.empty_like(x)
    sc.set_tuning("fast_fixups", mode)
    try:
        sc._check(sc.lib().sc_ntt_columns_dev(x.data_ptr(), y.data_ptr(), n, cols, rt, inverse, None))
        sc.synchronize()
    finally:
        sc.set_tuning("fast_fixups", 1)
    return y


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("logn,cols", SHAPES)
def test_fast_fixups_modes_agree(sc, logn, cols, name):
    import torch
    n = 1 << logn
    rt = sc.fe_bytes(po.primitive_nth_root(n))
    col = _column(logn, name)
    if name == "random":
        data = col + synth.synth_packed(2700 + logn, n * (cols - 1)).tobytes()
    else:
        data = col * cols
    x = _dev(data)
    for inverse in (0, 1):
        y = _columns(sc, x, n, cols, rt, inverse, 1)
        for mode in (0, 2):
            assert torch.equal(_columns(sc, x, n, cols, rt, inverse, mode), y), (logn, cols, name, inverse, mode)
        got = y.cpu().numpy().tobytes()
        for c in range(cols):
            if name == "random" and c:
                want = (C.intt if inverse else C.ntt)(po.primitive_nth_root(n), data[16 * n * c:16 * n * (c + 1)], n)
            else:
                want = _want(logn, name, inverse)
            assert got[16 * n * c:16 * n * (c + 1)] == want, (logn, cols, name, inverse, c)
        # the flags are all clear again: a second default run gives the same
        assert torch.equal(_columns(sc, x, n, cols, rt, inverse, 1), y), (logn, cols, name, inverse, "again")


def test_three_pass_columns_take_the_exact_middle_pass(sc):
    """2^22 x 2 columns: three passes of eight-element tiles, the middle one in place (exact kernel on every tile); equal to each
    column transformed alone, in every mode"""
    import torch
    logn, cols = 22, 2
    n = 1 << logn
    lib = sc.lib()
    assert lib.sc_ntt_num_passes(n) == 3
    rt = sc.fe_bytes(po.primitive_nth_root(n))
    half = _fe(0, n // 2).tobytes() + _fe(1, n // 2).tobytes()
    x = _dev(synth.synth_packed(2922, n).tobytes() + half)
    one = torch.empty(2 * n, dtype=torch.int64, device=x.device)
    for inverse in (0, 1):
        y = _columns(sc, x, n, cols, rt, inverse, 1)
        for c in range(cols):
            sc._check(lib.sc_ntt_dev(x.data_ptr() + 16 * n * c, one.data_ptr(), n, rt, inverse, None))
            sc.synchronize()
            assert torch.equal(one, y[2 * n * c:2 * n * (c + 1)]), (inverse, c)
        for mode in (0, 2):
            assert torch.equal(_columns(sc, x, n, cols, rt, inverse, mode), y), (inverse, mode)

"""sc_scale_columns_dev (include/starkcore.h): Polynomial.scale for the rows of a matrix in one launch -- every row byte for byte what
sc_scale_dev gives on it, strides above the row length with the gaps left alone, in place, and the argument errors with nothing written."""
import random

import pytest

pytestmark = pytest.mark.gpu
P = 1 + 407 * (1 << 119)
SC_ERR_BAD_ARG = -6                  # include/starkcore.h
SENTINEL = b"\xff" * 16              # not a residue: a kernel that wrote over it shows


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


def pack(values):
    return b"".join(v.to_bytes(16, "little") for v in values)


@pytest.mark.parametrize("n,cols", [(1, 1), (257, 3), (4099, 2), (1024, 130)])
def test_rows_equal_the_single_vector_entry(sc, n, cols):
    rng = random.Random(1000 * n + cols)
    lib = sc.lib()
    factor = sc.fe_bytes(rng.randrange(2, P))
    rows = [pack([rng.choice([0, 1, P - 1, rng.randrange(P)]) for _ in range(n)]) for _ in range(cols)]
    want = []
    for row in rows:
        a, b = sc.DeviceVector.from_bytes(row), sc.DeviceVector(n)
        sc._check(lib.sc_scale_dev(a.ptr, b.ptr, n, factor, None))
        want.append(b.to_bytes())
    ld_in, ld_out = n + 2, n + 1
    source = b"".join(row + SENTINEL * 2 for row in rows)
    a, out = sc.DeviceVector.from_bytes(source), sc.DeviceVector.from_bytes(SENTINEL * (cols * ld_out))
    sc._check(lib.sc_scale_columns_dev(a.ptr, ld_in, out.ptr, ld_out, n, cols, factor, None))
    assert out.to_bytes() == b"".join(row + SENTINEL for row in want)
    assert a.to_bytes() == source
    sc._check(lib.sc_scale_columns_dev(a.ptr, ld_in, a.ptr, ld_in, n, cols, factor, None))          # in place
    assert a.to_bytes() == b"".join(row + SENTINEL * 2 for row in want)


def test_argument_errors_write_nothing(sc):
    lib = sc.lib()
    n, cols = 64, 3
    blank = SENTINEL * (n * cols)
    a, out = sc.DeviceVector.from_bytes(pack(range(1, n * cols + 1))), sc.DeviceVector.from_bytes(blank)
    factor = sc.fe_bytes(5)
    assert lib.sc_scale_columns_dev(a.ptr, n, out.ptr, n, 0, cols, factor, None) == 0
    assert lib.sc_scale_columns_dev(a.ptr, n, out.ptr, n, n, 0, factor, None) == 0
    for args in ((None, n, out.ptr, n, n, cols, factor), (a.ptr, n, None, n, n, cols, factor), (a.ptr, n, out.ptr, n, n, cols, None),
                 (a.ptr, n - 1, out.ptr, n, n, cols, factor), (a.ptr, n, out.ptr, n - 1, n, cols, factor),
                 (a.ptr, n, out.ptr, n, n, cols, sc.fe_bytes(P)), (out.ptr, n + 1, out.ptr, n, n - 1, cols, factor)):
        assert lib.sc_scale_columns_dev(*args, None) == SC_ERR_BAD_ARG, args
    sc.synchronize()
    assert out.to_bytes() == blank

"""The eight-element batch kernels (ntt_pass_kernel_fixed8, 2^12-element tiles of 2^10 / 2^9 / 2^8 points) on every shape the planner
gives them -- forward and inverse, with the direct four-step tables, coset scaling, zero padding and the pruned first pass -- equal each
column transformed alone (sc_ntt_dev / sc_coset_evaluate_dev, the four-element kernels), the generic pass kernel (fixed_shapes = 0) and
the C oracle."""
import numpy as np
import pytest

from oracle import py_oracle as po
import synth

pytestmark = pytest.mark.gpu
C = po.C

# log2 length -> fixed8 shapes of its two passes: 17: (9,3) (8,4) | 18: (9,3) (9,3) | 19: (10,2) (9,3) | 20: (10,2) (10,2)
SHAPES = [(17, 3), (18, 2), (19, 2), (20, 2)]


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    starkcore.set_tuning("fixed_shapes", 1)


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.int64).copy()).to(torch.device("cuda", 0))


def _generic(sc, fn):
    sc.set_tuning("fixed_shapes", 0)
    try:
        return fn()
    finally:
        sc.set_tuning("fixed_shapes", 1)


@pytest.mark.parametrize("logn,cols", SHAPES)
def test_fixed8_columns_forward_inverse(sc, logn, cols):
    import torch
    lib = sc.lib()
    n = 1 << logn
    root = po.primitive_nth_root(n)
    rt = sc.fe_bytes(root)
    data = synth.synth_packed(1700 + logn, n * cols).tobytes()
    x = _dev(data)
    for inverse in (0, 1):
        y, one = torch.empty_like(x), torch.empty(2 * n, dtype=torch.int64, device=x.device)
        sc._check(lib.sc_ntt_columns_dev(x.data_ptr(), y.data_ptr(), n, cols, rt, inverse, None))
        sc.synchronize()
        for c in range(cols):
            sc._check(lib.sc_ntt_dev(x.data_ptr() + 16 * n * c, one.data_ptr(), n, rt, inverse, None))
            sc.synchronize()
            assert torch.equal(one, y[2 * n * c:2 * n * (c + 1)]), (logn, inverse, c)
        g = torch.empty_like(x)
        _generic(sc, lambda: (sc._check(lib.sc_ntt_columns_dev(x.data_ptr(), g.data_ptr(), n, cols, rt, inverse, None)), sc.synchronize()))
        assert torch.equal(g, y), (logn, inverse)
        c = cols - 1
        want = (C.intt if inverse else C.ntt)(root, data[16 * n * c:16 * n * (c + 1)], n)
        assert y[2 * n * c:2 * n * (c + 1)].cpu().numpy().tobytes() == want, (logn, inverse)


# (logn, cols, m): m coefficients per column, zero-padded to n and scaled by the coset offset; m << n prunes the first pass's top stages
@pytest.mark.parametrize("logn,cols,m", [(17, 2, 1 << 14), (18, 3, 1 << 15), (19, 2, (1 << 19) - 5), (20, 2, 1000)])
def test_fixed8_coset_evaluate_columns(sc, logn, cols, m):
    import torch
    lib = sc.lib()
    n = 1 << logn
    root = po.primitive_nth_root(n)
    rt, off = sc.fe_bytes(root), sc.fe_bytes(po.GENERATOR)
    data = synth.synth_packed(1800 + logn, m * cols).tobytes()
    x = _dev(data)
    y = torch.empty(2 * n * cols, dtype=torch.int64, device=x.device)
    one = torch.empty(2 * n, dtype=torch.int64, device=x.device)
    sc._check(lib.sc_coset_evaluate_columns_dev(x.data_ptr(), m, cols, off, rt, n, y.data_ptr(), None))
    sc.synchronize()
    for c in range(cols):
        sc._check(lib.sc_coset_evaluate_dev(x.data_ptr() + 16 * m * c, m, off, rt, n, one.data_ptr(), None))
        sc.synchronize()
        assert torch.equal(one, y[2 * n * c:2 * n * (c + 1)]), (logn, m, c)
    g = torch.empty_like(y)
    _generic(sc, lambda: (sc._check(lib.sc_coset_evaluate_columns_dev(x.data_ptr(), m, cols, off, rt, n, g.data_ptr(), None)), sc.synchronize()))
    assert torch.equal(g, y), (logn, m)
    assert y[:2 * n].cpu().numpy().tobytes() == C.coset_evaluate(data[:16 * m], m, po.GENERATOR, root, n), (logn, m)

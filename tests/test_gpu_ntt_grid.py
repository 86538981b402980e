"""Every NTT entry of the library, bit for bit against the C oracle, under every tuning of tests/ntt_grid.py: the planner's knobs
(tests/emu/plan_dump.cpp's grid) and the launch-only ones (fixed shapes, wave-local fences, s_setprio placement, XCD remap, direct
table limits).  include/starkcore.h promises that results never depend on the tuning.  Where the planner refuses a case
(tests/emu/kernel_cover.cpp, built against the tree's planner, says which) the entry must return SC_ERR_UNSUPPORTED, never a result.

Inputs are synth data with edge residues (0, 1, p-1, 2^64-1, 2^64, 2^127) sprinkled in; expected values come from the oracle once per
module.  Inverse transforms take the oracle's forward output as input and must give back the forward input exactly."""
import ctypes
import time

import numpy as np
import pytest
import torch

import ntt_grid
from oracle import py_oracle as po
import synth

pytestmark = pytest.mark.gpu
C = po.C
P = po.P
EDGES = (0, 1, P - 1, (1 << 64) - 1, 1 << 64, 1 << 127)
SENTINEL = -1                      # int64 limbs of 2^128 - 1: not a residue, never written by a transform
ORACLE_SECONDS = [0.0]


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    t0 = time.time()
    yield starkcore
    _reset(starkcore)
    print(f"\ntest_gpu_ntt_grid: oracle {ORACLE_SECONDS[0]:.1f} s of {time.time() - t0:.1f} s")


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    return ntt_grid.plan_grid(ntt_grid.build_helper(str(tmp_path_factory.mktemp("kernel_cover"))))


def _reset(sc):
    for k, v in ntt_grid.DEFAULTS.items():
        sc.set_tuning(k, v)


@pytest.fixture(autouse=True)
def tuned(request, sc):
    """applies the test's tuning; afterwards the header's defaults, checked: the rest of the suite must not inherit a tuning"""
    name = request.node.callspec.params["tuning"]
    try:
        for k, v in ntt_grid.TUNING[name].items():
            sc.set_tuning(k, v)
        yield name
    finally:
        _reset(sc)
        lib = sc.lib()
        assert lib.sc_ntt_num_passes(1 << 20) == 2 and lib.sc_ntt_num_passes(1 << 24) == 3
        x, y = _columns_expect(17)
        out = torch.empty_like(x[:3 << 17])
        torch.cuda.synchronize()                   # (the library's stream is not ordered with torch's)
        sc._check(lib.sc_ntt_columns_dev(x.data_ptr(), out.data_ptr(), 1 << 17, 3, _rt(_root(1 << 17)), 0, None))
        sc.synchronize()
        assert torch.equal(out, y[:3 << 17]), "the default tuning no longer computes a 2^17 x 3 column batch correctly"


# ---- inputs and expected values (module caches; nothing here depends on the tuning)

def _data(seed, n):
    a = synth.synth_packed(seed, n)
    for i, e in zip((0, n - 1, n // 2, 1, n // 2 + 1, 7919), EDGES):
        a[i % n] = (e & ((1 << 64) - 1), e >> 64)
    return a


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 2)).to(torch.device("cuda", 0))


def _oracle(fn, *args):
    t = time.time()
    r = fn(*args)
    ORACLE_SECONDS[0] += time.time() - t
    return r


def _root(n, which=0):
    r = po.primitive_nth_root(n)
    return r if which == 0 else pow(r, (0x9E3779B97F4A7C15 % n) | 1, P)     # another primitive n-th root


def _rt(v):
    return (ctypes.c_uint64 * 2)(v & ((1 << 64) - 1), v >> 64)


_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _ntt_expect(lg, which):
    def make():
        n = 1 << lg
        x = _data(100 + lg, n).tobytes()
        return _dev(np.frombuffer(x, np.uint64)), _dev(np.frombuffer(_oracle(C.ntt, _root(n, which), x, n), np.uint64))
    return _cached(("ntt", lg, which), make)


COL_MAX = 5


def _columns_expect(lg):
    """x: COL_MAX columns of 2^lg (70 for 2^9), y: their transforms; a batch of c columns is the first c of them"""
    def make():
        n, cols = 1 << lg, (70 if lg == 9 else COL_MAX)
        x = _data(200 + lg, n * cols).tobytes()
        y = b"".join(_oracle(C.ntt, _root(n), x[16 * n * c:16 * n * (c + 1)], n) for c in range(cols))
        return _dev(np.frombuffer(x, np.uint64)), _dev(np.frombuffer(y, np.uint64))
    return _cached(("cols", lg), make)


def _coset_expect(lg, cols, m):
    def make():
        n = 1 << lg
        x = _data(300 + lg, m * cols).tobytes()
        y = b"".join(_oracle(C.coset_evaluate, x[16 * m * c:16 * m * (c + 1)], m, po.GENERATOR, _root(n), n) for c in range(cols))
        return _dev(np.frombuffer(x, np.uint64)), _dev(np.frombuffer(y, np.uint64))
    return _cached(("coset", lg, cols, m), make)


def _rows_expect(ll, lb):
    """R [batch][len] (host, (batch, len, 2) uint64) and the transforms of its rows, transposed: [len][batch] (device)"""
    def make():
        ln, b = 1 << ll, 1 << lb
        R = _data(400 + 32 * ll + lb, ln * b).reshape(b, ln, 2)
        root = _root(ln)
        T = np.empty_like(R)
        for i in range(b):
            T[i] = np.frombuffer(_oracle(C.ntt, root, R[i].tobytes(), ln), np.uint64).reshape(ln, 2)
        return R, _dev(T.transpose(1, 0, 2))
    return _cached(("rows", ll, lb), make)


def _outer_expect(ll, lb, base, order, ninv):
    def make():
        ln, b = 1 << ll, 1 << lb
        _, tt = _rows_expect(ll, lb)
        t0 = time.time()
        v = synth.unpack_ints(tt.cpu().numpy().tobytes())
        w = po.primitive_nth_root(order)
        s = po.inv(order) if ninv else 1
        out = []
        for r in range(ln):
            wr = pow(w, r, P)
            f = pow(wr, base, P) * s % P
            for c in range(b):
                out.append(v[r * b + c] * f % P)
                f = f * wr % P
        ORACLE_SECONDS[0] += time.time() - t0
        return _dev(np.frombuffer(synth.pack_ints(out), np.uint64))
    return _cached(("outer", ll, lb, base, order, ninv), make)


def _chunked(R, chunks):
    """[batch][len] -> [chunks][batch][len / chunks] (what all_to_all_single delivers)"""
    b, ln, _ = R.shape
    return R.reshape(b, chunks, ln // chunks, 2).transpose(1, 0, 2, 3)


def _fails(fails, cid, got, want, kernels):
    if not torch.equal(got, want):
        bad = (got != want).any(dim=-1)
        idx = torch.nonzero(bad).flatten()
        unwritten = int((bad & (got == SENTINEL).all(dim=-1)).sum())
        fails.append(f"{cid}: {idx.numel()} of {want.shape[0]} elements differ ({unwritten} of them never written: still the sentinel), "
                     f"first at {idx[0].item()}   [{' '.join(kernels)}]")


def _run(sc, planned, tuning, cid, call, fails):
    """call() -> rc; the passes as planned (kernel@prio_balance) if the case ran and its result is to be checked, else None.
    The entries run on the library's own stream, which nothing orders with torch's: the inputs and the sentinel-filled outputs
    torch prepared must have landed before the call (and sc.synchronize() after it lets torch read the result)."""
    kernels = planned[tuning][cid]
    torch.cuda.synchronize()
    rc = call()
    if kernels is None:
        if rc != sc.SC_ERR_UNSUPPORTED:
            fails.append(f"{cid}: the planner refuses it, the entry returned {rc} instead of SC_ERR_UNSUPPORTED")
        return None
    if rc != 0:
        fails.append(f"{cid}: rc {rc} ({sc.lib().sc_last_error().decode()}), planned as {' '.join(kernels)}")
        return None
    sc.synchronize()
    return kernels


def _report(tuning, fails):
    assert not fails, f"tuning {tuning}: {len(fails)} failing cases\n" + "\n".join(fails[:40])


TUNING_NAMES = [name for name, _ in ntt_grid.TUNINGS]


@pytest.mark.parametrize("tuning", TUNING_NAMES)
def test_ntt_dev(sc, planned, tuning):
    lib, fails = sc.lib(), []
    for cid, lg, which, inv in ntt_grid.ntt_cases(tuning):
        n = 1 << lg
        x, y = _ntt_expect(lg, which)
        src, want = (y, x) if inv else (x, y)
        out = torch.full_like(x, SENTINEL)
        k = _run(sc, planned, tuning, cid, lambda: lib.sc_ntt_dev(src.data_ptr(), out.data_ptr(), n, _rt(_root(n, which)), inv, None), fails)
        if k:
            _fails(fails, cid, out, want, k)
    _report(tuning, fails)


@pytest.mark.parametrize("tuning", TUNING_NAMES)
def test_ntt_columns_dev(sc, planned, tuning):
    lib, fails = sc.lib(), []
    for cid, lg, cols, inv, in_place in ntt_grid.column_cases():
        n = 1 << lg
        x, y = _columns_expect(lg)
        src, want = (y, x) if inv else (x, y)
        src, want = src[:n * cols], want[:n * cols]
        if in_place:
            out = src.clone()
            src = out
        else:
            out = torch.full_like(src, SENTINEL)
        k = _run(sc, planned, tuning, cid, lambda: lib.sc_ntt_columns_dev(src.data_ptr(), out.data_ptr(), n, cols, _rt(_root(n)), inv, None), fails)
        if k:
            _fails(fails, cid, out, want, k)
    _report(tuning, fails)


@pytest.mark.parametrize("tuning", TUNING_NAMES)
def test_coset_evaluate(sc, planned, tuning):
    lib, fails = sc.lib(), []
    off = _rt(po.GENERATOR)
    for cid, lg, cols, m, columns in ntt_grid.coset_cases():
        n = 1 << lg
        x, y = _coset_expect(lg, dict(ntt_grid.COSET_SHAPES)[lg], m)
        out = torch.full((n * cols, 2), SENTINEL, dtype=torch.int64, device=x.device)
        if columns:
            call = lambda: lib.sc_coset_evaluate_columns_dev(x.data_ptr(), m, cols, off, _rt(_root(n)), n, out.data_ptr(), None)
        else:
            call = lambda: lib.sc_coset_evaluate_dev(x.data_ptr(), m, off, _rt(_root(n)), n, out.data_ptr(), None)
        k = _run(sc, planned, tuning, cid, call, fails)
        if k:
            _fails(fails, cid, out, y[:n * cols], k)
    _report(tuning, fails)


@pytest.mark.parametrize("tuning", TUNING_NAMES)
def test_ntt_batch(sc, planned, tuning):
    """kinds 0 and 1 plain (sc_ntt_batch_dev), kind 0 with the outer twiddle and kind 1 from chunks (sc_ntt_batch_ex_dev)"""
    lib, fails = sc.lib(), []
    for cid, kind, ll, lb in ntt_grid.batch_cases():
        ln, b = 1 << ll, 1 << lb
        if planned[tuning][cid] is None and not any(planned[t][cid] for t in planned):
            src = want = torch.zeros((ln * b, 2), dtype=torch.int64, device="cuda")     # refused by every tuning: no oracle needed
        else:
            R, want = _rows_expect(ll, lb)
            src = _dev(R.transpose(1, 0, 2) if kind == 0 else R)
        out = torch.full_like(want, SENTINEL)
        k = _run(sc, planned, tuning, cid, lambda: lib.sc_ntt_batch_dev(src.data_ptr(), out.data_ptr(), ln, b, kind, _rt(_root(ln)), None), fails)
        if k:
            _fails(fails, cid, out, want, k)
    for cid, ll, lb, base, order, ninv in ntt_grid.outer_cases():
        ln, b = 1 << ll, 1 << lb
        R, _ = _rows_expect(ll, lb)
        src, want = _dev(R.transpose(1, 0, 2)), _outer_expect(ll, lb, base, order, ninv)
        out = torch.full_like(want, SENTINEL)
        call = lambda: lib.sc_ntt_batch_ex_dev(src.data_ptr(), out.data_ptr(), ln, b, 0, _rt(_root(ln)), _rt(po.primitive_nth_root(order)), order,
                                               base, ninv, 1, None)
        k = _run(sc, planned, tuning, cid, call, fails)
        if k:
            _fails(fails, cid, out, want, k)
    for cid, ll, lb, chunks in ntt_grid.chunk_cases():
        ln, b = 1 << ll, 1 << lb
        R, want = _rows_expect(ll, lb)
        src = _dev(_chunked(R, chunks))
        out = torch.full_like(want, SENTINEL)
        call = lambda: lib.sc_ntt_batch_ex_dev(src.data_ptr(), out.data_ptr(), ln, b, 1, _rt(_root(ln)), None, 0, 0, 0, chunks, None)
        k = _run(sc, planned, tuning, cid, call, fails)
        if k:
            _fails(fails, cid, out, want, k)
    _report(tuning, fails)


@pytest.mark.parametrize("tuning", TUNING_NAMES)
def test_ntt_rows_t_ld(sc, planned, tuning):
    """a row block written as `batch` adjacent columns of a wider [len][out_ld] output: the other columns stay untouched"""
    lib, fails = sc.lib(), []
    for cid, ll, lb, chunks, ld, col0 in ntt_grid.rows_ld_cases():
        ln, b = 1 << ll, 1 << lb
        R, t = _rows_expect(ll, lb)
        src = _dev(_chunked(R, chunks))
        out = torch.full((ln, ld, 2), SENTINEL, dtype=torch.int64, device=src.device)
        want = out.clone()
        want[:, col0:col0 + b] = t.reshape(ln, b, 2)
        call = lambda: lib.sc_ntt_rows_t_ld_dev(src.data_ptr(), out.data_ptr() + 16 * col0, ln, b, _rt(_root(ln)), chunks, ld, None)
        k = _run(sc, planned, tuning, cid, call, fails)
        if k:
            _fails(fails, cid, out.reshape(-1, 2), want.reshape(-1, 2), k)
    _report(tuning, fails)


@pytest.mark.parametrize("tuning", TUNING_NAMES)
def test_sharded_stages(sc, planned, tuning):
    """the column stage (outer twiddle, the rank's own block into its receive buffer: the ALT kernels) and the row stage (chunked
    input, row blocks, deferred second pass) of the sharded transform, through tests/test_gpu_sharded.py's simulated world"""
    from test_gpu_sharded import _simulate
    fails = []
    for cid, lg, world, blocks, defer, diag, log1 in ntt_grid.sharded_cases():
        refused = any(v is None for k, v in planned[tuning].items() if k.startswith(cid + "/"))
        try:
            full_in, got, back, root = _simulate(sc, lg, world, seed=17, blocks=blocks, defer=defer, diag_in_place=diag, log_n1=log1 or None)
        except sc.StarkCoreError as e:
            if not (refused and f"error {sc.SC_ERR_UNSUPPORTED}" in str(e)):
                fails.append(f"{cid}: {e}")
            continue
        if refused:
            fails.append(f"{cid}: the planner refuses a stage, the transform ran")
            continue
        n = 1 << lg
        want = _cached(("sharded", lg), lambda: _oracle(C.ntt, root, full_in, n))
        if got != want:
            fails.append(f"{cid}: forward transform differs")
        if back != full_in:
            fails.append(f"{cid}: round trip differs")
    _report(tuning, fails)

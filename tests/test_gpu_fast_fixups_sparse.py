"""The flag-to-redo path of the eight-element batch kernels (ntt_pass_kernel_fixed8 marks flags[grid index], ntt_pass_redo8_kernel
transforms the marked tiles again from the pass's input) on inputs that flag a proper subset of a launch's workgroups: one lane of one
interior tile, the last wave of the last workgroup, pass 1 alone, the last round of a tile, a butterfly product, the product at the
store, three workgroups of one launch with one of the other pass (fast_fixups_cases.py builds them and proves on the CPU where they
flag; test_fast_fixups_cases_emu.py).  Every result equals the C oracle in every column and sc_set_tuning("fast_fixups", 0 / 2) bit
for bit; under xcd_remap and wave_local 0 / 1; with two flagged transforms in flight on two streams, whose flag words are separate;
and a random input after a flagged one on the same stream."""
import ctypes

import numpy as np
import pytest

import fast_fixups_cases as fxc
import synth

pytestmark = pytest.mark.gpu
DEFAULTS = dict(fast_fixups=1, xcd_remap=1, wave_local=1)


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    yield starkcore
    for key, value in DEFAULTS.items():
        starkcore.set_tuning(key, value)


def _dev(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.int64).copy()).to(torch.device("cuda", 0))


def _run(sc, case, x, stream=None, **tuning):
    """the case's transform of the device tensor x under the given knobs (restored afterwards); waits unless a stream is given"""
    import torch
    y = torch.empty_like(x)
    plan = case.plan
    try:
        for key, value in tuning.items():
            sc.set_tuning(key, value)
        sc._check(sc.lib().sc_ntt_columns_dev(x.data_ptr(), y.data_ptr(), plan.n, plan.cols, sc.fe_bytes(plan.root), case.inverse, stream))
        if stream is None:
            sc.synchronize()
    finally:
        for key in tuning:
            sc.set_tuning(key, DEFAULTS[key])
    return y


def _bytes(y):
    return y.cpu().numpy().tobytes()


@pytest.mark.parametrize("shape,inverse,name", fxc.case_ids())
def test_sparse_flags_redo_the_right_tiles(sc, shape, inverse, name):
    import torch
    case = fxc.build(shape, inverse, name)
    want = case.plan.oracle(case.data)
    x = _dev(case.data)
    y = _run(sc, case, x, fast_fixups=1)
    got = _bytes(y)
    n16 = 16 * case.plan.n
    bad = [c for c in range(case.cols) if got[n16 * c:n16 * (c + 1)] != want[n16 * c:n16 * (c + 1)]]
    assert not bad, (shape, inverse, name, "columns", bad)
    for mode in (0, 2):
        assert torch.equal(_run(sc, case, x, fast_fixups=mode), y), (shape, inverse, name, mode)
    # the flags are all clear again
    assert torch.equal(_run(sc, case, x, fast_fixups=1), y), (shape, inverse, name, "again")


@pytest.mark.parametrize("name", ["p0-sub", "p1-sub", "three"])
@pytest.mark.parametrize("shape,inverse", [(s, inv) for s in fxc.SHAPES for inv in (0, 1)])
def test_sparse_flags_under_launch_knobs(sc, shape, inverse, name):
    case = fxc.build(shape, inverse, name)
    want = case.plan.oracle(case.data)
    x = _dev(case.data)
    for remap in (0, 1):
        for wave_local in (0, 1):
            assert _bytes(_run(sc, case, x, xcd_remap=remap, wave_local=wave_local)) == want, (shape, inverse, name, remap, wave_local)


def test_two_flagged_transforms_in_flight_on_two_streams(sc):
    """the tile flags are per stream: two flagged transforms of shape A side by side, many times over, never waiting in between"""
    import torch
    dev = torch.device("cuda", 0)
    cases = [fxc.build("A", 0, "three"), fxc.build("A", 0, "p0-add-last")]
    wants = [c.plan.oracle(c.data) for c in cases]
    xs = [_dev(c.data) for c in cases]
    streams = [torch.cuda.Stream(device=dev) for _ in cases]
    torch.cuda.synchronize()
    ys = [[], []]
    for rep in range(6):
        for k, (case, x) in enumerate(zip(cases, xs)):
            ys[k].append(_run(sc, case, x, stream=ctypes.c_void_p(streams[k].cuda_stream)))
    torch.cuda.synchronize()
    for k in range(2):
        for y in ys[k]:
            assert _bytes(y) == wants[k], k


def test_random_input_after_a_flagged_one_on_the_same_stream(sc):
    """the redo leaves every flag word zero: a random input of the same shape right behind a flagged one, same stream, no wait"""
    import torch
    for shape, name in (("A", "three"), ("B", "late")):
        case = fxc.build(shape, 0, name)
        plan = case.plan
        rnd = synth.synth_packed(7300 + plan.logn, plan.count).tobytes()
        want_rnd = plan.oracle(rnd)
        st = torch.cuda.Stream(device=torch.device("cuda", 0))
        x, r = _dev(case.data), _dev(rnd)
        torch.cuda.synchronize()
        p = ctypes.c_void_p(st.cuda_stream)
        y = _run(sc, case, x, stream=p)
        z = _run(sc, case, r, stream=p)
        torch.cuda.synchronize()
        assert _bytes(y) == plan.oracle(case.data), (shape, name)
        assert _bytes(z) == want_rnd, (shape, name)

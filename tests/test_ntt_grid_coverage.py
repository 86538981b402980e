"""The GPU grid of tests/test_gpu_ntt_grid.py reaches every NTT pass kernel the library can launch.  tests/emu/kernel_cover.cpp
plans every case of tests/ntt_grid.py with the tree's planner and reports the kernel of each launch as launch_pass picks it
(csrc/ntt_plan.h: pass_kernel, pass_prio_balance -- the functions core.hip uses).  The fixed-shape lists are read from the
X-macros of csrc/ntt_tile.cuh, so a shape added there without a GPU case fails here."""
import json
import os
import re

import pytest

from conftest import GOLDEN
import ntt_grid

GIB = 1 << 30
DEVICE_BUDGET = 24 * GIB       # what one GPU test may allocate


def _shapes(name):
    with open(os.path.join(ntt_grid.CSRC, "ntt_tile.cuh")) as f:
        m = re.search(r"#define\s+" + name + r"\(X\)\s+(.*)", f.read())
    return [(int(a), int(b)) for a, b in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", m.group(1))]


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    return ntt_grid.build_helper(str(tmp_path_factory.mktemp("kernel_cover")))


@pytest.fixture(scope="module")
def launches(helper):
    """{kernel: {prio_balance}} over every launch of every case of every tuning"""
    out = {}
    for res in ntt_grid.plan_grid(helper).values():
        for kernels in res.values():
            for k in kernels or []:
                kern, prio = k.split("@p")
                out.setdefault(kern, set()).add(int(prio))
    return out


def test_grid_tunings_are_the_plan_dumps():
    """the planner knobs of the grid are exactly tests/emu/plan_dump.cpp's tunings (the digests' case names)"""
    with open(os.path.join(GOLDEN, "ntt_plans.json")) as f:
        dumped = {name.rsplit(" ", 1)[0] for name in json.load(f)}
    launch_only = {"fixed_shapes", "wave_local", "xcd_remap", "prio_balance", "direct_tw_max_log"}
    planner = {name for name, t in ntt_grid.TUNINGS if not set(t) & launch_only}
    assert planner == dumped
    for key in launch_only:
        assert any(key in t for _, t in ntt_grid.TUNINGS), key


def test_every_fixed4_shape_launched_plain_and_alt(launches):
    shapes = _shapes("SC_FIXED4_SHAPES")
    assert len(shapes) >= 6
    missing = [f"fixed4<{lr},{lc},0,{alt}>" for lr, lc in shapes for alt in (0, 1) if f"fixed4<{lr},{lc},0,{alt}>" not in launches]
    assert not missing, f"SC_FIXED4_SHAPES entries no GPU grid case launches: {missing}"


def test_every_fixed8_shape_launched(launches):
    shapes = _shapes("SC_FIXED8_SHAPES")
    assert len(shapes) >= 3
    missing = [f"fixed8<{lr},{lc}>" for lr, lc in shapes if f"fixed8<{lr},{lc}>" not in launches]
    assert not missing, f"SC_FIXED8_SHAPES entries no GPU grid case launches: {missing}"


def test_generic_kernels_launched(launches):
    assert {f"generic<{e}>" for e in (1, 2, 3, 4)} <= set(launches)


def test_prio_balance_schedules_on_fixed_kernels(launches):
    for fam in ("fixed4", "fixed8"):
        seen = set().union(*(p for k, p in launches.items() if k.startswith(fam + "<")))
        assert seen == {0, 1, 2}, (fam, seen)


def test_only_the_traced_kernels_are_left_out(launches):
    """every instantiation launch_pass can select is in the grid except the traced ones (sc_debug_trace: diagnostics, never a
    production launch) -- and nothing outside that set is reported"""
    can = {f"fixed4<{lr},{lc},0,{alt}>" for lr, lc in _shapes("SC_FIXED4_SHAPES") for alt in (0, 1)}
    can |= {f"fixed8<{lr},{lc}>" for lr, lc in _shapes("SC_FIXED8_SHAPES")}
    can |= {f"generic<{e}>" for e in (1, 2, 3, 4)}
    traced = {f"fixed4<{lr},{lc},1,0>" for lr, lc in _shapes("SC_FIXED4_SHAPES")}
    got = {k.split(":")[0] for k in launches}
    assert got == can
    assert not got & traced


def test_fixed8_offset_fallback_is_out_of_device_reach(helper):
    """fixed_offsets_fit keeps an eight-element launch whose lane byte offsets could reach 4 GiB on the generic kernel.  The search
    (kernel_cover 'nofit') runs sc_ntt_columns_dev plans over every tuning of the grid, lengths 2^1..2^32, forward and inverse, full,
    zero-padded and pruned inputs, and power-of-two column counts 1..2^16.  A column count enters a plan only as cols > 1 and
    floor(log2 cols), so these stand for every count; a column input stride enters only PassParams::col_stride_in, which
    fixed_offsets_fit does not read.  The smallest such transform needs more device memory than a test may take (input + work
    buffer, in place), so the GPU grid cannot hold one; if a planner change brings one within reach, this fails and the case belongs
    in tests/test_gpu_ntt_grid.py."""
    lines = [ntt_grid.helper_input(name)[0] for name in ntt_grid.TUNING] + ["nofit"]
    out = ntt_grid.run_helper(helper, lines).strip().splitlines()[-1]
    m = re.match(r"nofit (.*) elements=(\d+)$", out)
    assert m, out
    elements = int(m.group(2))
    print(f"smallest fixed8 launch outside fixed_offsets_fit: {m.group(1)}, {elements} elements")
    assert elements == 0 or 2 * 16 * elements > DEVICE_BUDGET, out

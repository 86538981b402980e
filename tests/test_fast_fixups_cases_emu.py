"""The sparse-flag cases of fast_fixups_cases.py on the CPU: each input really is what it claims.  Per case, with the emulation of
tests/emu/ntt_fast_emu.cpp (fx_*) and the C oracle: the exact emulated passes chained give the oracle's transform of every column; the
FAST emulation of every pass flags exactly the planted workgroups, in the planted waves and first in the planted round; a launch that
missed the redo of any one planted tile would return a wrong result (inside that tile's stores for a tile of the last pass); and the
state the case chose -- a pass's input, or a tile's LDS image at the input of a round -- is the one the exact transform of the input
passes through."""
import numpy as np
import pytest

import fast_fixups_cases as fxc


@pytest.mark.parametrize("shape,inverse,name", fxc.case_ids())
def test_case_flags_exactly_where_planted(shape, inverse, name):
    case = fxc.build(shape, inverse, name)
    plan = case.plan
    assert (case.logn, case.cols) == fxc.SHAPES[shape] and len(case.data) == 16 * plan.count
    want = np.frombuffer(plan.oracle(case.data), dtype=np.uint64).reshape(-1, 2)
    runs = fxc.emulate(case)
    npass = len(runs)
    # the exact passes chained are the transform, every column
    assert np.array_equal(runs[-1][1], want)
    # the flagged set, with waves and first round
    got = {(k, int(g), int(words[g])) for k, (_, _, words) in enumerate(runs) for g in np.nonzero(words)[0]}
    assert got == {(f.k, f.grid, fxc.word_of(f.waves, f.round)) for f in case.flagged}
    assert case.flagged and all(plan.grid_tile(f.k, f.grid) == f.tile for f in case.flagged)
    # one missing redo changes the result
    for f in case.flagged:
        fast, exact, _ = runs[f.k]
        fp = fxc.footprint(case, f)
        buf = exact.copy()
        buf[fp] = fast[fp]
        assert not np.array_equal(buf[fp], exact[fp]), f
        for k in range(f.k + 1, npass):
            buf = plan.run_pass(k, buf, fast=False)[1]
        if f.k == npass - 1:
            assert not np.array_equal(buf[fp], want[fp]), f
        else:
            assert not np.array_equal(buf, want), f
    # the chosen state occurs
    x = np.frombuffer(case.data, dtype=np.uint64).reshape(-1, 2)
    inputs = [x] + [r[1] for r in runs]
    assert case.chosen
    for c in case.chosen:
        if c[0] == "buffer":
            assert np.array_equal(inputs[c[1]], c[2]), c[:2]
        else:
            _, k, tile, rnd, state = c
            lds = np.zeros_like(state)
            plan.tile(k, tile, 0, rnd, False, inp=inputs[k], state=lds)
            assert np.array_equal(lds, state), c[:4]


def test_cases_cover_what_they_claim():
    """the case list: every eight-element shape, both passes, a workgroup that xcd_remap moves, wave 0 and the last wave, first and
    last round, both directions"""
    ids = fxc.case_ids()
    assert len(ids) == len(set(ids)) == 28
    shapes = set()
    for s, (logn, cols) in fxc.SHAPES.items():
        for inv in (0, 1):
            plan = fxc.Plan(logn, cols, inv)
            assert all(p.fast and p.loge == 3 for p in plan.passes)
            shapes |= {(p.logR, p.logC) for p in plan.passes}
            assert all(plan.nwg(k) % 2 == 0 for k in range(2))
    assert shapes == {(10, 2), (9, 3), (8, 4)}
    three = fxc.build("A", 0, "three")
    assert {f.k for f in three.flagged} == {0, 1}
    p1 = [f for f in three.flagged if f.k == 1]
    assert {f.grid for f in p1} >= {0, three.plan.nwg(1) - 1} and any(f.grid != f.tile for f in p1)
    assert {w for f in p1 for w in f.waves} >= {0, 7}

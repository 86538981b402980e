"""The NTT planner (csrc/ntt_plan.h) plans every case of tests/emu/plan_dump.cpp exactly as recorded in tests/golden/ntt_plans.json:
every pass descriptor field, digit split, pass count and which shapes are refused.  See tests/golden/make_ntt_plans.py."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, PKG

_spec = importlib.util.spec_from_file_location("make_ntt_plans", os.path.join(GOLDEN, "make_ntt_plans.py"))
make_ntt_plans = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_ntt_plans)


@pytest.fixture(scope="module")
def plans():
    return make_ntt_plans.dump(os.path.join(PKG, "csrc"), tuple(os.environ.get("NTT_PLAN_CXXFLAGS", "-O2").split()))


def test_plans_match_fixture(plans):
    with open(make_ntt_plans.FIXTURE) as f:
        want = json.load(f)
    got = make_ntt_plans.digests(plans)
    assert list(got) == list(want), "the harness enumerates other cases than the fixture holds"
    for name, digest in got.items():
        assert digest == want[name], f"plans of case '{name}' changed; its dump:\n{plans[name]}"

"""sc_stark_combination_batch on the device -- combination_point_kernel, mpoly_eval_columns_kernel under the prover's plan,
combination_sum_kernel (csrc/combination.cuh) -- against the model of tests/combination_cases.py, verdict for verdict: the honest
and the changed cases of the CPU walk (tests/test_combination_emu.py), the largest case through at least three staging chunks, the
Rescue-Prime AIR, and the errors of the entry's list."""
import ctypes

import numpy as np
import pytest

import combination_cases as cases
from combination_cases import ACCEPT, REJECT, UNDECIDED, P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible"
    starkcore.init()


import starkcore as sc                             # noqa: E402

SC_ERR_BAD_ARG = -6
UNTOUCHED = 0xEE


def verdicts_of(case):
    """the case through the binding (starkcore.Combination, combination_batch)"""
    nterms, exps, coefs, weights, polys, pool = case.tables()
    shared = sc.Combination(case.w, nterms, exps, coefs, case.generator, case.omega, case.n, case.step, case.transition_shifts, case.boundary_shifts,
                            len(case.members), weights, np.asarray(polys, dtype=np.uint64), pool)
    rows = np.frombuffer(case.packed_rows(), dtype=sc.combination_row_dtype(case.w))
    return [int(v) for v in sc.combination_batch(shared, rows)]


@pytest.mark.parametrize("name", cases.NAMES)
def test_honest_rows_are_accepted(name):
    case = cases.honest(name)
    assert verdicts_of(case) == cases.expected(name)[0] == [ACCEPT] * len(case.rows)


@pytest.mark.parametrize("name,what", [(name, what) for name in cases.NAMES for what in cases.MUTATIONS if what != "coefficient" or cases.SHAPES[name][1]])
def test_changed_inputs_get_the_models_verdicts(name, what):
    case, hit = cases.mutated(name, what)
    want = cases.expected(name, what)[0]
    assert all(want[i] == verdict for i, verdict in hit.items())
    assert verdicts_of(case) == want


def test_largest_case_through_three_staging_chunks():
    case = cases.honest(cases.LARGEST)
    case.rows[5]["claimed"] = (case.rows[5]["claimed"] + 1) % P
    case.rows[-1]["zerofier"] = 0
    want = [ACCEPT] * len(case.rows)
    want[5], want[-1] = REJECT, UNDECIDED
    sc._check(sc.lib().sc_set_tuning(b"verify_stage_kb", 32))            # 32 KiB / (128 + 1) bytes: 250 rows per chunk, 4 chunks
    try:
        got = verdicts_of(case)
    finally:
        sc._check(sc.lib().sc_set_tuning(b"verify_stage_kb", 65536))
    assert got == want
    assert verdicts_of(case) == want


def test_rescue_prime_air_128_rows():
    """the constraints of RescuePrime.transition_constraints under the plan the prover uses (364 products per point)"""
    case, (want, _) = cases.rescue_prime_case(128)
    assert want.count(ACCEPT) == 126 and want[:2] == [REJECT, REJECT]
    assert verdicts_of(case) == want


def test_undecided_when_a_shared_residue_is_not_below_p():
    case = cases.honest("w2_c1_n8_r255")
    case.generator = P
    assert verdicts_of(case) == [UNDECIDED] * len(case.rows)
    case = cases.honest("w2_c1_n8_r255")
    member = case.rows[0]["member"]
    case.members[member]["weights"][2] = P + 1
    assert verdicts_of(case) == [UNDECIDED if r["member"] == member else ACCEPT for r in case.rows]


def test_errors_of_the_entrys_list_run_nothing():
    case = cases.honest("w2_c1_n8_r255")
    n = len(case.rows)
    call = sc.lib().sc_stark_combination_batch

    def status(case, rows="case", out="buffer", **overrides):
        shared, keep = case.shared(**overrides)
        packed = case.packed_rows()
        row_buffer = ctypes.create_string_buffer(packed, len(packed)) if rows == "case" else None
        verdicts = ctypes.create_string_buffer(bytes([UNTOUCHED]) * n, n)
        rc = call(ctypes.byref(shared), row_buffer, n, verdicts if out == "buffer" else None)
        assert verdicts.raw == bytes([UNTOUCHED]) * n or rc == 0
        return rc

    assert status(case) == 0
    assert call(None, None, 0, None) == 0                                 # n == 0
    assert status(case, rows=None) == SC_ERR_BAD_ARG and status(case, out=None) == SC_ERR_BAD_ARG
    for field in ("boundary_shifts", "weights", "polys", "pool", "nterms", "transition_shifts", "exps", "coefs"):
        assert status(case, **{field: None}) == SC_ERR_BAD_ARG, field
    for overrides in ({"registers": 0}, {"registers": 128}, {"domain_length": 12}, {"domain_length": 0}, {"step": 0},
                      {"pool_len": len(case.tables()[5]) // 16 - 1}):
        assert status(case, **overrides) == SC_ERR_BAD_ARG, overrides
    for field, bad in (("index", case.n), ("member", len(case.members))):
        broken = cases.honest(case.name)
        broken.rows[n - 1][field] = bad
        assert status(broken) == SC_ERR_BAD_ARG, field
    broken = cases.honest(case.name)
    broken.constraints[0][0] = (broken.constraints[0][0][0], P)
    assert status(broken) == SC_ERR_BAD_ARG
    assert status(case) == 0                                              # the library is none the worse

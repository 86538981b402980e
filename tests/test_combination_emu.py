"""CPU walk of the verifier's combination rows (csrc/combination.cuh: combination_point_kernel, the plan walk of
mpoly_eval_columns_kernel, combination_sum_kernel) compiled for the host by tests/emu/combination_emu.cpp, thread by thread over the
launched grids and chunk by chunk, against the model of tests/combination_cases.py: the verdicts and the intermediate point matrix,
the undecided rows, every error of the entry's list with nothing written -- and the same walk as a stand-alone program built under
ASan + UBSan (COMBINATION_EMU_CXXFLAGS overrides the flags)."""
import ctypes
import os
import struct
import subprocess

import pytest

from conftest import REPO
import combination_cases as cases
from combination_cases import ACCEPT, REJECT, UNDECIDED, P, pack, unpack

EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "stark-anatomy_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "combination_emu.cpp")] + [os.path.join(CSRC, f) for f in ("combination.cuh", "combination_plan.h", "mpoly_plan.h", "columns.cuh",
                                                                                          "ntt_tile.cuh", "field.cuh")]
u64, vp = ctypes.c_uint64, ctypes.c_void_p
STAGE = 64 << 20                 # the library's default staging buffer
UNTOUCHED = 0xEE


def stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in SOURCES)


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libcombination_emu.so")
    if stale(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SOURCES[0]])
    lib = ctypes.CDLL(so)
    lib.emu_stark_combination_batch.restype = ctypes.c_int
    lib.emu_stark_combination_batch.argtypes = [vp, vp, u64, vp, u64, vp, vp]
    lib.emu_combination_products.restype = ctypes.c_longlong
    lib.emu_combination_products.argtypes = [vp, u64]
    return lib


def run(emu, case, stage=STAGE, rows="case", verdicts="buffer", **overrides):
    """-> (status, verdicts, point matrix as [variable][row], chunks); what is not written keeps UNTOUCHED bytes"""
    shared, keep = case.shared(**overrides)
    packed = case.packed_rows() if rows == "case" else rows
    n = len(case.rows)
    row_buffer = ctypes.create_string_buffer(packed, max(16, len(packed))) if packed is not None else None
    out = ctypes.create_string_buffer(bytes([UNTOUCHED]) * n, n)
    points = ctypes.create_string_buffer(bytes([UNTOUCHED]) * (16 * case.nvars * n), 16 * case.nvars * n)
    chunks = u64(0)
    rc = emu.emu_stark_combination_batch(ctypes.byref(shared), row_buffer, n, out if verdicts == "buffer" else None, stage, points, ctypes.byref(chunks))
    flat = unpack(points.raw)
    return rc, list(out.raw), [flat[j * n:(j + 1) * n] for j in range(case.nvars)], chunks.value


def check(case, verdicts, matrix, want):
    want_verdicts, want_points = want
    assert verdicts == want_verdicts, case.name
    for i, point in enumerate(want_points):
        if point is not None:
            assert [matrix[j][i] for j in range(case.nvars)] == point, (case.name, i)


@pytest.mark.parametrize("name", cases.NAMES)
def test_honest_rows_are_accepted_and_the_point_matrix_is_the_models(emu, name):
    case = cases.honest(name)
    rc, verdicts, matrix, chunks = run(emu, case)
    assert rc == 0 and chunks == 1
    assert cases.expected(name)[0] == [ACCEPT] * len(case.rows)
    check(case, verdicts, matrix, cases.expected(name))


@pytest.mark.parametrize("name,what", [(name, what) for name in cases.NAMES for what in cases.MUTATIONS if what != "coefficient" or cases.SHAPES[name][1]])
def test_changed_inputs_get_the_models_verdicts(emu, name, what):
    case, hit = cases.mutated(name, what)
    want = cases.expected(name, what)
    for i, verdict in hit.items():
        assert want[0][i] == verdict, (what, i)                        # the change is seen where it was made ...
    if what != "list_coefficient":
        assert all(v == ACCEPT for i, v in enumerate(want[0]) if i not in hit)       # ... and nowhere else
    rc, verdicts, matrix, _ = run(emu, case)
    assert rc == 0
    check(case, verdicts, matrix, want)


def test_a_changed_list_coefficient_is_seen_through_the_air(emu):
    want = cases.expected("w3_c3_n4096_r256", "list_coefficient")[0]
    assert REJECT in want and ACCEPT in want


@pytest.mark.parametrize("stage_kb", [16, 32])
def test_chunks_through_a_small_staging_buffer(emu, stage_kb):
    case = cases.honest(cases.LARGEST)
    rc, verdicts, matrix, chunks = run(emu, case, stage=stage_kb << 10)
    assert rc == 0 and chunks >= 3
    check(case, verdicts, matrix, cases.expected(cases.LARGEST))


def test_case_table_covers_what_it_claims():
    table = [cases.honest(name) for name in cases.NAMES]
    assert {c.w for c in table} == {1, 2, 3, 5} and {len(c.constraints) for c in table} == {0, 1, 3}
    assert {c.n for c in table} == {8, 1 << 12} and {c.step for c in table} == {4}
    assert {len(c.rows) for c in table} == {1, 255, 256, 257, 1000}
    assert any(terms == [] for c in table for terms in c.constraints)
    shifts = {s for c in table for s in c.transition_shifts + c.boundary_shifts}
    assert {0, 1} <= shifts and any(s >= 1 << 32 for s in shifts)
    for c in table:
        indices = [r["index"] for r in c.rows]
        assert c.n - c.step in indices and (len(indices) < 3 or {0, c.n - 1} <= set(indices))
        assert any(m["zerofiers"][s] == [1] and m["interpolants"][s] == [] for m in c.members for s in range(c.w))
    assert any(len({len(m["zerofiers"][0]) for m in c.members}) > 1 for c in table)


def test_undecided_when_generator_or_omega_is_not_a_residue(emu):
    case = cases.honest("w2_c1_n8_r255")
    words = lambda v: (u64 * 2)(v & (2 ** 64 - 1), v >> 64)
    for field in ("generator", "omega"):
        rc, verdicts, _, _ = run(emu, case, **{field: words(P)})
        assert rc == 0 and verdicts == [UNDECIDED] * len(case.rows)


def test_undecided_when_a_weight_or_a_list_coefficient_is_not_a_residue(emu):
    for what in ("weights", "zerofiers"):
        case = cases.honest("w3_c3_n4096_r256")
        member = case.rows[0]["member"]
        if what == "weights":
            case.members[member]["weights"][-1] = P
        else:
            case.members[member]["zerofiers"][1][0] = (1 << 128) - 1
        rc, verdicts, _, _ = run(emu, case)
        assert rc == 0
        assert verdicts == [UNDECIDED if r["member"] == member else ACCEPT for r in case.rows]


def test_every_error_of_the_entrys_list_writes_nothing(emu):
    case = cases.honest("w2_c1_n8_r255")
    n = len(case.rows)
    untouched = lambda result: result[0] == 1 and result[1] == [UNTOUCHED] * n and all(v == int.from_bytes(bytes([UNTOUCHED]) * 16, "little") for row in result[2] for v in row)
    assert run(emu, case)[0] == 0
    # null pointers
    assert untouched(run(emu, case, rows=None))
    assert run(emu, case, verdicts=None)[0] == 1
    for field in ("boundary_shifts", "weights", "polys", "pool", "nterms", "transition_shifts", "exps", "coefs"):
        assert untouched(run(emu, case, **{field: None})), field
    shared, keep = case.shared()
    assert emu.emu_stark_combination_batch(None, keep[0], n, keep[0], STAGE, None, None) == 1
    # no register; more than 255 variables
    assert untouched(run(emu, case, registers=0)) and untouched(run(emu, case, registers=128))
    # a domain length that is no power of two; step 0
    for bad in (0, 12, (1 << 12) + 1):
        assert untouched(run(emu, case, domain_length=bad)), bad
    assert untouched(run(emu, case, step=0))
    # a row's index outside the domain, its member outside the table
    for field, bad in (("index", case.n), ("member", len(case.members))):
        broken = cases.honest(case.name)
        broken.rows[n - 1][field] = bad
        assert untouched(run(emu, broken)), field
    # a coefficient list outside the pool: the pool one element shorter than the lists need, a length that wraps
    pool_len = len(case.tables()[5]) // 16
    assert untouched(run(emu, case, pool_len=pool_len - 1))
    nterms, exps, coefs, weights, polys, pool = case.tables()
    wrapped = list(polys)
    wrapped[1] = (1 << 64) - 1
    wrapped = (u64 * len(wrapped))(*wrapped)
    assert untouched(run(emu, case, polys=ctypes.addressof(wrapped)))
    # a coefficient of the AIR that is not below p
    for bad in (P, (1 << 128) - 1):
        broken = cases.honest(case.name)
        terms = broken.constraints[0]
        terms[0] = (terms[0][0], bad)
        assert untouched(run(emu, broken)), bad
    # n == 0 is fine, whatever else is passed
    assert emu.emu_stark_combination_batch(None, None, 0, None, STAGE, None, None) == 0


def test_rescue_prime_air_runs_under_the_provers_plan(emu):
    """the signature's AIR: two constraints over 5 variables, 364 products per point in the plan (tests/test_mpoly_columns_emu.py)"""
    case, want = cases.rescue_prime_case(16)
    shared, keep = case.shared()
    assert [emu.emu_combination_products(ctypes.byref(shared), k) for k in range(2)] == [364, 364]
    rc, verdicts, matrix, _ = run(emu, case)
    assert rc == 0
    check(case, verdicts, matrix, want)
    assert want[0].count(ACCEPT) == len(case.rows) - 2 and want[0][:2] == [REJECT, REJECT]


def call_file(case, stage):
    """one call as the stand-alone program reads it (tests/emu/combination_emu.cpp, main)"""
    nterms, exps, coefs, weights, polys, pool = case.tables()
    words = lambda v: [v & (2 ** 64 - 1), v >> 64]
    head = [case.w, len(nterms), case.n, case.step, len(case.members), len(case.rows), stage, sum(nterms), len(pool) // 16] + words(case.generator) + words(case.omega) + [0, 0, 0]
    tables = nterms + case.transition_shifts + case.boundary_shifts + polys
    tables += [0] * (len(tables) & 1)
    return struct.pack("<%dQ" % len(head), *head) + coefs + weights + pool + struct.pack("<%dQ" % len(tables), *tables) + case.packed_rows() + exps


def test_standalone_walk_under_sanitizers(tmp_path):
    """the walk with a main of its own, built under ASan + UBSan and run as a program: honest rows, undecided rows and three chunks"""
    flags = os.environ.get("COMBINATION_EMU_CXXFLAGS", "-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer").split()
    program = os.path.join(EMU_DIR, "combination_emu_main")
    if stale(program) or "COMBINATION_EMU_CXXFLAGS" in os.environ:
        subprocess.check_call(["g++", "-std=c++17", "-DCOMBINATION_EMU_MAIN"] + flags + ["-o", program, SOURCES[0]])
    for name, what, stage in ((cases.LARGEST, None, 32 << 10), ("w5_c3_n4096_r257", "leaf_is_p", STAGE), ("w1_c0_n8_r1", None, STAGE)):
        case = cases.honest(name) if what is None else cases.mutated(name, what)[0]
        path = tmp_path / "call.bin"
        path.write_bytes(call_file(case, stage))
        done = subprocess.run([program, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert done.returncode == 0, done.stderr[-2000:]
        status, chunks, verdicts, points = done.stdout.split("\n")[:4]
        n = len(case.rows)
        assert int(status) == 0 and (int(chunks) >= 3) == (stage < STAGE)
        flat = [int(points[32 * k:32 * k + 32], 16) for k in range(case.nvars * n)]
        check(case, list(bytes.fromhex(verdicts)), [flat[j * n:(j + 1) * n] for j in range(case.nvars)], cases.expected(name, what))

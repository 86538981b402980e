"""CPU walk of mpoly_eval_columns_kernel (csrc/columns.cuh) under the plan of csrc/mpoly_plan.h, compiled for the host by
tests/emu/mpoly_columns_emu.cpp, against Python integers: every member and every constraint of the cases of
tests/mpoly_columns_cases.py, thread by thread over the launched grids -- one launch and several (rows of 65 535 and of 4 pairs) --,
the values left as they were, the gaps of the output untouched, the plan's Horner variables and product counts, the errors of the
entry's list that the plan decides, and the product count of the Rescue-Prime AIR."""
import ctypes
import os
import subprocess

import pytest

from conftest import REPO
import mpoly_columns_cases as cases
from mpoly_columns_cases import P, SENTINEL, pack, unpack

EMU_DIR = os.path.join(REPO, "tests", "emu")
u64, vp, u32 = ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libmpoly_columns_emu.so")
    srcs = [os.path.join(EMU_DIR, "mpoly_columns_emu.cpp")] + [os.path.join(REPO, "stark-anatomy_amd", "csrc", f) for f in ("mpoly_plan.h", "columns.cuh", "ntt_tile.cuh", "field.cuh")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, srcs[0]])
    lib = ctypes.CDLL(so)
    lib.emu_mpoly_eval_columns.restype = ctypes.c_int
    lib.emu_mpoly_eval_columns.argtypes = [vp, u64, u64, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, u32, vp, vp, vp]
    lib.emu_scale_cols.restype = None
    lib.emu_scale_cols.argtypes = [vp, u64, vp, u64, u64, u64, vp]
    return lib


def array(kind, values):
    return None if values is None else (kind * len(values))(*values)


def run(emu, c, rows, var_src="case", var_rot="case", coefs=None, n=None):
    """-> (status, flat output, ld_out, products, term-by-term products, Horner variables)"""
    n = c.n if n is None else n
    ncons, ld_out = len(c.constraints), c.n + c.pad
    vals = ctypes.create_string_buffer(c.buf, len(c.buf))
    out = ctypes.create_string_buffer(pack([SENTINEL] * (c.members * ncons * ld_out)), 16 * c.members * ncons * ld_out)
    products, flat, horner = (u64 * ncons)(), (u64 * ncons)(), (u32 * ncons)()
    rc = emu.emu_mpoly_eval_columns(vals, c.nvars, n, c.members, array(u64, c.var_base), array(u64, c.var_ld), array(u32, c.var_src if var_src == "case" else var_src),
                                    array(u64, c.var_rot if var_rot == "case" else var_rot), ncons, array(u64, c.nterms), c.exps, c.coefs if coefs is None else coefs, out,
                                    ld_out, rows, products, flat, horner)
    assert vals.raw[:len(c.buf)] == c.buf, "the values were modified"
    return rc, unpack(out.raw), ld_out, list(products), list(flat), list(horner)


def check(c, flat_out, ld_out):
    ncons = len(c.constraints)
    for m in range(c.members):
        for k in range(ncons):
            row = flat_out[(m * ncons + k) * ld_out:(m * ncons + k + 1) * ld_out]
            assert row[:c.n] == c.expected[m][k], (c.name, m, k)
            assert row[c.n:] == [SENTINEL] * c.pad, "the gap behind row (%d, %d) was written" % (m, k)


@pytest.mark.parametrize("name", cases.NAMES)
@pytest.mark.parametrize("rows", [65535, 4], ids=["one_launch", "rows_of_4"])
def test_walk_matches_python_integers(emu, name, rows):
    c = cases.case(name)
    rc, flat_out, ld_out, products, flat, horner = run(emu, c, rows)
    assert rc == 0
    check(c, flat_out, ld_out)
    for k, terms in enumerate(c.constraints):
        h = cases.horner_variable(terms, c.nvars)
        assert horner[k] == (cases.ABSENT if h is None else h), k
        assert (products[k], flat[k]) == cases.products(terms, c.nvars), k
    assert c.expected[0][3] == [0] * c.n and c.nterms[3] == 0          # the constraint without terms writes zeros
    assert products[0] < flat[0]


def test_walk_of_more_pairs_than_one_launch_takes(emu):
    c = cases.case(cases.MANY_PAIRS)
    assert c.members * len(c.constraints) > 65535
    rc, flat_out, ld_out, _, _, _ = run(emu, c, 65535)
    assert rc == 0
    check(c, flat_out, ld_out)


def test_case_table_covers_what_it_claims():
    """the shapes, roles, exponent lists and special values the cases are there for are in them"""
    table = [cases.case(name) for name in cases.NAMES]
    assert {c.nvars for c in table} == {1, 2, 3, 4, 5, 6}
    assert {c.n for c in table if "turned" not in c.role} == {1, 3, 256, 257} and {c.n for c in table if "turned" in c.role} == {2, 512}
    assert {c.members for c in table} == {1, 3}
    for role in ("shared", "absent", "turned"):
        assert any(role in c.role for c in table)
    for c in table:
        horner, tie, constant, empty, tall = c.constraints
        h = cases.horner_variable(horner, c.nvars)
        steps = sorted({k[h] for k, _ in horner}, reverse=True)
        assert steps[0] == 78 and steps[-1] > 0 and any(a - b > 1 for a, b in zip(steps, steps[1:])) and len(steps) < len(horner)
        assert max(k[j] for k, _ in tall for j in range(c.nvars)) == 255 and min(max(k) for k, _ in tall) <= 1
        tops = [max(k[j] for k, _ in tie) for j in range(c.nvars)]
        assert c.nvars - len([r for r in c.role if r == "absent"]) < 2 or tops.count(max(tops)) >= 2
        assert constant[0][0] == (0,) * c.nvars and empty == []
    seen = {v for c in table for per in c.values for row in per if row is not None for v in row}
    assert {0, 1, P - 1} <= seen


def test_errors_the_plan_decides(emu):
    c = cases.case("n512_v4_k3_turned")                 # roles: shared, stored, turned (off variable 1), absent
    assert c.role == ["shared", "stored", "turned", "absent"]
    untouched = lambda result: result[1] == [SENTINEL] * len(result[1])
    # a coefficient that is not canonical (p itself; 2^128 - 1)
    for bad in (P, SENTINEL):
        values = unpack(c.coefs)
        values[-1] = bad
        result = run(emu, c, 65535, coefs=pack(values))
        assert result[0] == 1 and untouched(result)
    # a term that uses an absent variable: mark the stored variable 1's reader and variable 0 absent in turn
    result = run(emu, c, 65535, var_src=[cases.ABSENT, 1, 1, cases.ABSENT])
    assert result[0] == 1 and untouched(result)
    # a turned variable that points at a turned one, at itself with a turn, past the end
    for src, rot in (([0, 2, 1, cases.ABSENT], [0, 3, 3, 0]), ([0, 1, 2, cases.ABSENT], [0, 0, 3, 0]), ([0, 1, 4, cases.ABSENT], [0, 0, 3, 0]),
                     ([0, 1, 1, cases.ABSENT], [0, 1, 3, 0])):
        result = run(emu, c, 65535, var_src=src, var_rot=rot)
        assert result[0] == 1 and untouched(result), (src, rot)
    # turned variables over a count that is no power of two
    result = run(emu, c, 65535, n=511)
    assert result[0] == 2 and untouched(result)
    # ... which nothing objects to when nothing is turned
    plain = cases.case("n257_v4_k3")
    assert "absent" in plain.role and run(emu, plain, 65535)[0] == 0


def test_rescue_prime_air_needs_364_products_per_point(emu):
    """the two transition constraints of the signature's AIR: 272 live terms over 5 variables with highest exponents [78, 3, 3, 3, 3];
    7 176 products per point term by term, 78 + 286 = 364 in the plan"""
    from algebra import Field
    from rescue_prime import RescuePrime
    rp = RescuePrime()
    omicron = Field.main().primitive_nth_root(1 << 9)         # the trace domain's generator: 27 rounds + 1 rows, padded with the randomizers
    constraints = rp.transition_constraints(omicron)
    assert len(constraints) == 2
    plans = [a.value_domain_terms([1] * 5) for a in constraints]
    nvars = 5
    terms = [plan[1] for plan in plans]
    for t in terms:
        assert len(t) == 272 and [max(k[j] for k, _ in t) for j in range(nvars)] == [78, 3, 3, 3, 3]
    ncons, n = 2, 4
    values = [[(7 * j + 3 * i + 1) % P for i in range(n)] for j in range(nvars)]
    vals = ctypes.create_string_buffer(pack([v for row in values for v in row]))
    out = ctypes.create_string_buffer(16 * ncons * n)
    products, flat, horner = (u64 * ncons)(), (u64 * ncons)(), (u32 * ncons)()
    rc = emu.emu_mpoly_eval_columns(vals, nvars, n, 1, array(u64, [j * n for j in range(nvars)]), array(u64, [n] * nvars), None, None, ncons,
                                    array(u64, [len(t) for t in terms]), bytes(e for t in terms for k, _ in t for e in k), pack([v for t in terms for _, v in t]),
                                    out, n, 65535, products, flat, horner)
    assert rc == 0
    assert list(products) == [364, 364] and list(flat) == [7176, 7176] and list(horner) == [0, 0]
    got = unpack(out.raw)
    for k, t in enumerate(terms):
        assert got[k * n:(k + 1) * n] == [cases._evaluate(t, values, i) for i in range(n)]


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_scaling_of_rows_matches_python_powers(emu, n):
    """scale_cols_kernel: out[c][i] = in[c][i] * factor^i, strides above n, the gaps untouched, in place too (4099: past the first
    level of the power table)"""
    import random
    rng = random.Random(n)
    cols, ld_in, ld_out = 3, n + 2, n + 1
    factor = rng.randrange(2, P)
    rows = [[rng.choice([0, 1, P - 1, rng.randrange(P)]) for _ in range(n)] for _ in range(cols)]
    powers = [1]
    for _ in range(n - 1):
        powers.append(powers[-1] * factor % P)
    want = [[v * w % P for v, w in zip(row, powers)] for row in rows]
    packed = pack([v for row in rows for v in row + [SENTINEL] * (ld_in - n)])
    source = ctypes.create_string_buffer(packed, len(packed))
    out = ctypes.create_string_buffer(pack([SENTINEL] * (cols * ld_out)), 16 * cols * ld_out)
    emu.emu_scale_cols(source, ld_in, out, ld_out, n, cols, pack([factor]))
    assert source.raw == packed
    flat = unpack(out.raw)
    assert [flat[c * ld_out:(c + 1) * ld_out] for c in range(cols)] == [row + [SENTINEL] for row in want]
    emu.emu_scale_cols(source, ld_in, source, ld_in, n, cols, pack([factor]))
    flat = unpack(source.raw)
    assert [flat[c * ld_in:(c + 1) * ld_in] for c in range(cols)] == [row + [SENTINEL] * 2 for row in want]

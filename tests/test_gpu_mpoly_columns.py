"""sc_mpoly_eval_columns_dev (include/starkcore.h) called directly on the cases of tests/mpoly_columns_cases.py: every member and every
constraint equal to sc_mpoly_eval_rot_dev -- called per member and per constraint on copies of the values -- and to Python integers,
the values left as they were, the gaps between the rows of the output untouched; more (member, constraint) pairs than one grid takes;
and every error of the entry's list with nothing written."""
import ctypes

import pytest

import mpoly_columns_cases as cases
from mpoly_columns_cases import ABSENT, P, SENTINEL, pack, unpack

pytestmark = pytest.mark.gpu
SC_ERR_NOT_POW2, SC_ERR_BAD_ARG = -2, -6         # include/starkcore.h
u64, u32 = ctypes.c_uint64, ctypes.c_uint32


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


def array(kind, values):
    return None if values is None else (kind * len(values))(*values)


KEEP = object()


def call(sc, c, vals, out, ld_out, n=KEEP, members=KEEP, nvars=KEEP, var_base=KEEP, var_ld=KEEP, var_src=KEEP, var_rot=KEEP, ncons=KEEP, nterms=KEEP, exps=KEEP, coefs=KEEP):
    """the entry on case c's operands, any of them replaced; -> return code"""
    pick = lambda given, own: own if given is KEEP else given
    return sc.lib().sc_mpoly_eval_columns_dev(vals, pick(nvars, c.nvars), pick(n, c.n), pick(members, c.members), pick(var_base, array(u64, c.var_base)),
                                              pick(var_ld, array(u64, c.var_ld)), pick(var_src, array(u32, c.var_src)), pick(var_rot, array(u64, c.var_rot)),
                                              pick(ncons, len(c.constraints)), pick(nterms, array(u64, c.nterms)), pick(exps, c.exps), pick(coefs, c.coefs), out, ld_out, None)


def run(sc, c):
    """-> the output matrix as integers, [members * ncons][ld_out]; checks that the values survive"""
    ld_out = c.n + c.pad
    rows = c.members * len(c.constraints)
    vals = sc.DeviceVector.from_bytes(c.buf)
    out = sc.DeviceVector.from_bytes(pack([SENTINEL]) * (rows * ld_out))
    sc._check(call(sc, c, vals.ptr, out.ptr, ld_out))
    flat = unpack(out.to_bytes())
    assert vals.to_bytes() == c.buf, "the values were modified"
    return [flat[r * ld_out:(r + 1) * ld_out] for r in range(rows)]


def oracle(sc, c, m, k):
    """constraint k on member m's values through sc_mpoly_eval_rot_dev, on a [nvars][n] copy of its own (which that entry converts)"""
    turned = "turned" in c.role
    rows = [row if (row is not None and not (turned and c.role[j] == "turned")) else [0] * c.n for j, row in enumerate(c.values[m])]
    vals = sc.DeviceVector.from_ints([v for row in rows for v in row])
    out = sc.DeviceVector(c.n)
    terms = c.constraints[k]
    exps = bytes(e for key, _ in terms for e in key)
    coefs = pack([v for _, v in terms])
    src, rot = (array(u32, c.var_src), array(u64, c.var_rot)) if turned else (None, None)
    sc._check(sc.lib().sc_mpoly_eval_rot_dev(vals.ptr, c.nvars, c.n, exps, coefs, len(terms), out.ptr, 0, src, rot, None))
    return unpack(out.to_bytes())


@pytest.mark.parametrize("name", cases.NAMES)
def test_equals_the_single_constraint_entry_and_python_integers(sc, name):
    c = cases.case(name)
    ncons = len(c.constraints)
    got = run(sc, c)
    for m in range(c.members):
        for k in range(ncons):
            row = got[m * ncons + k]
            assert row[:c.n] == oracle(sc, c, m, k), (m, k)
            assert row[:c.n] == c.expected[m][k], (m, k)
            assert row[c.n:] == [SENTINEL] * c.pad, "the gap behind row (%d, %d) was written" % (m, k)


def test_more_pairs_than_one_grid_takes(sc):
    """n = 1, 32 769 members x 2 constraints = 65 538 rows: the second launch starts at pair 65 535, in the middle of a member"""
    c = cases.case(cases.MANY_PAIRS)
    ncons = len(c.constraints)
    assert c.members * ncons > 65535 and 65535 % ncons
    got = run(sc, c)
    for m in range(c.members):
        for k in range(ncons):
            assert got[m * ncons + k] == c.expected[m][k] + [SENTINEL] * c.pad, (m, k)
    for m in (0, 32766, 32767, 32768):
        for k in range(ncons):
            assert got[m * ncons + k][:1] == oracle(sc, c, m, k), (m, k)


def test_nothing_to_do_is_not_an_error(sc):
    c = cases.case("n3_v2_k1")
    out = sc.DeviceVector.from_bytes(pack([SENTINEL]) * 64)
    vals = sc.DeviceVector.from_bytes(c.buf)
    assert call(sc, c, vals.ptr, out.ptr, c.n, members=0) == 0
    assert call(sc, c, vals.ptr, out.ptr, c.n, ncons=0) == 0
    assert call(sc, c, None, None, c.n, members=0, nterms=None, exps=None, coefs=None) == 0
    assert out.to_bytes() == pack([SENTINEL]) * 64


def test_every_error_leaves_the_output_alone(sc):
    c = cases.case("n512_v4_k3_turned")                 # roles: shared, stored, turned (off variable 1), absent
    assert c.role == ["shared", "stored", "turned", "absent"]
    ld_out = c.n + c.pad
    rows = c.members * len(c.constraints)
    blank = pack([SENTINEL]) * (rows * ld_out)
    vals = sc.DeviceVector.from_bytes(c.buf + pack([SENTINEL]) * (rows * ld_out))        # room for an output inside the same allocation
    out = sc.DeviceVector.from_bytes(blank)
    bad_coefs = []
    for bad in (P, SENTINEL):
        values = unpack(c.coefs)
        values[len(values) // 2] = bad
        bad_coefs.append(pack(values))
    # where the shared variable 0 and member 2's rows of variable 1 lie: an output over either overlaps an input
    over_shared = vals.ptr + 16 * c.var_base[0]
    over_last_member = vals.ptr + 16 * (c.var_base[1] + 2 * c.var_ld[1] + c.n - 1)
    wrong = [("null values", dict(vals=None), SC_ERR_BAD_ARG),
             ("null output", dict(out=None), SC_ERR_BAD_ARG),
             ("null var_base", dict(var_base=None), SC_ERR_BAD_ARG),
             ("null var_ld", dict(var_ld=None), SC_ERR_BAD_ARG),
             ("null nterms", dict(nterms=None), SC_ERR_BAD_ARG),
             ("null exps", dict(exps=None), SC_ERR_BAD_ARG),
             ("null coefs", dict(coefs=None), SC_ERR_BAD_ARG),
             ("var_src without var_rot", dict(var_rot=None), SC_ERR_BAD_ARG),
             ("no variables", dict(nvars=0), SC_ERR_BAD_ARG),
             ("256 variables", dict(nvars=256), SC_ERR_BAD_ARG),
             ("ld_out below n", dict(ld_out=c.n - 1), SC_ERR_BAD_ARG),
             ("output over the shared variable", dict(out=over_shared), SC_ERR_BAD_ARG),
             ("output over the last member's last value", dict(out=over_last_member), SC_ERR_BAD_ARG),
             ("coefficient p", dict(coefs=bad_coefs[0]), SC_ERR_BAD_ARG),
             ("coefficient 2^128 - 1", dict(coefs=bad_coefs[1]), SC_ERR_BAD_ARG),
             ("a term uses an absent variable", dict(var_src=array(u32, [ABSENT, 1, 1, ABSENT])), SC_ERR_BAD_ARG),
             ("turned off a turned variable", dict(var_src=array(u32, [0, 2, 1, ABSENT]), var_rot=array(u64, [0, 3, 3, 0])), SC_ERR_BAD_ARG),
             ("stored in its own place, but turned", dict(var_src=array(u32, [0, 1, 2, ABSENT])), SC_ERR_BAD_ARG),
             ("turned off a variable past the end", dict(var_src=array(u32, [0, 1, 4, ABSENT])), SC_ERR_BAD_ARG),
             ("turned, and n no power of two", dict(n=511), SC_ERR_NOT_POW2)]
    for what, change, code in wrong:
        change = dict(change)
        v = change.pop("vals", vals.ptr)
        o = change.pop("out", out.ptr)
        ld = change.pop("ld_out", ld_out)
        assert call(sc, c, v, o, ld, **change) == code, what
        sc.synchronize()
        assert out.to_bytes() == blank, what
        assert vals.to_bytes()[:len(c.buf)] == c.buf, what
    # and the same operands, unchanged, are taken
    assert call(sc, c, vals.ptr, out.ptr, ld_out) == 0
    assert unpack(out.to_bytes())[:c.n] == c.expected[0][0]

"""That the cases of tests/domain_tables_cases.py reach what they claim -- from the sources' own constants, not from copies -- and that
their expectations hold for the Python models of the device algorithms (tests/emu/geoseq_model.py, tests/emu/polytree_model.py), which
then stand between the definitions and tests/test_gpu_domain_tables_edges.py.  CPU only."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
from oracle import py_oracle as po
import domain_tables_cases as dc
import geoseq_model as gm
import ntt_grid
import polytree_model as pm
import synth

P = po.P
MODEL_LIMIT = 2368


# ---- the orders ---------------------------------------------------------------------------------------------------------------

def test_elements_of_the_stated_orders():
    assert P - 1 == 11 * 37 * (1 << 119)
    for d in dc.ODD_ORDERS:
        h = dc.element_of_order(d)
        assert pow(h, d, P) == 1 and all(pow(h, d // r, P) != 1 for r in dc.prime_factors(d)), d
        assert len({pow(h, i, P) for i in range(d)}) == d
    for case in dc.GEO_CASES:
        if case.kind == "full":
            assert pow(case.ratio, case.n, P) == 1 and all(pow(case.ratio, case.n // r, P) != 1 for r in dc.prime_factors(case.n)), case.id
        elif case.kind == "prewrap":
            assert pow(case.ratio, case.n + 1, P) == 1 and (case.n + 1) in (11, 37, 407, 2368), case.id
    assert len({c.id for c in dc.GEO_CASES}) == len(dc.GEO_CASES)


# ---- the scans ----------------------------------------------------------------------------------------------------------------

def scan_block():
    text = open(os.path.join(ntt_grid.CSRC, "geoseq.cuh")).read()
    e, t = (int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1)) for name in ("GS_E", "GS_T"))
    assert re.search(r"GS_BLOCK\s*=\s*\(uint64_t\)GS_E\s*\*\s*GS_T\s*;", text)
    return e * t


def scan_depth(count, block):
    """launch levels of scan_products (csrc/polytree_geo.hip): one workgroup scans alone, more of them scan their totals first"""
    nb = -(-count // block)
    return 1 if nb <= 1 else 1 + scan_depth(nb, block)


def scans_of(n):
    """the lengths geodomain_create scans: t_j (M of them), 1 / t_j and A_j (n each), the reversed products (n - 1)"""
    M = 1
    while M < 2 * n - 1:
        M *= 2
    return {"t": M, "tinv": n, "A": n, "rev": n - 1}


def test_scan_depths():
    block = scan_block()
    depth = {c.id: {k: scan_depth(v, block) for k, v in scans_of(c.n).items()} for c in dc.GEO_CASES}
    for case in dc.GEO_CASES:
        assert (max(depth[case.id].values()) == 3) == (case.kind == "deep"), case.id
    for case in dc.DEEP_CASES:
        assert depth[case.id] == {"t": 3, "tinv": 2, "A": 2, "rev": 2} and scans_of(case.n)["t"] == 1 << 23
    # what of the middle level reaches an output: the results read t_j for j <= 2n - 2, and workgroup b of the top level takes the
    # scanned total b - 1, so the middle level's second workgroup (scanned totals block .. ) is first read by workgroup block + 1
    assert dc.DEEP_CASES == (dc.DEEP_CASE, dc.GEO_CASES[-1])
    assert (2 * dc.DEEP_N - 2) // block == block and (2 * dc.DEEP_N_SEEN - 2) // block == block + 2
    assert scans_of(dc.DEEP_N)["t"] == 1 << 23 and scans_of(dc.DEEP_N - 1)["t"] == 1 << 22        # the smallest n with a third level
    assert scan_depth(1 << 22, block) == 2
    by_n = {c.n: depth[c.id] for c in dc.GEO_CASES if c.kind == "scan"}
    assert by_n[1024] == {"t": 1, "tinv": 1, "A": 1, "rev": 1}
    assert by_n[1025] == {"t": 2, "tinv": 1, "A": 1, "rev": 1}            # M = 4096: the first two-workgroup scan
    assert by_n[2048] == {"t": 2, "tinv": 1, "A": 1, "rev": 1}
    assert by_n[2049] == {"t": 2, "tinv": 2, "A": 2, "rev": 1}            # the n scans: one element in the second workgroup
    assert by_n[2050] == {"t": 2, "tinv": 2, "A": 2, "rev": 2}            # the n - 1 scan follows
    assert by_n[4096]["t"] == by_n[4097]["t"] == 2 and scans_of(4096)["t"] == 8192 and scans_of(4097)["t"] == 16384
    # the odd orders: M is not 2n and the reversed scan has an odd length where n is even
    for d in dc.ODD_ORDERS:
        assert scans_of(d)["t"] != 2 * d
    assert {(d - 1) % 2 for d in dc.ODD_ORDERS} == {0, 1}


# ---- the per-column fallback of ntt_cols ------------------------------------------------------------------------------------------

def test_big_tree_takes_the_per_column_transforms(tmp_path):
    exe = ntt_grid.build_helper(str(tmp_path))
    lines = ["tune default"] + ["batch L%d 0 %d 1 0 0 0 0 0 0 0 0 4" % (lg, lg) for lg in (18, 19, 20)]
    res = dict((line.split() + [""])[:2] for line in ntt_grid.run_helper(exe, lines).splitlines())
    assert res["L19"] == "unsupported" and res["L20"] == "unsupported"
    assert res["L18"] not in ("", "unsupported")
    # polytree_build transforms level l at length 2^(l+1) in batches of 2^(L-l): a tree of L levels reaches length 2^L with batch 2
    levels = lambda k: (k - 1).bit_length()
    assert levels(dc.BIG_TREE_K) == 19 and levels(dc.BIG_TREE_K - 1) == 18
    assert (1 << levels(dc.BIG_TREE_K)) - dc.BIG_TREE_K == (1 << 18) - 1       # the heaviest padding a tree carries


# ---- the sentinel -------------------------------------------------------------------------------------------------------------

def test_sentinel_is_a_residue_no_operand_equals():
    """... and the packed forms of the operands, which the device is given, are the lists the expectations are computed from"""
    assert 0 < dc.SENTINEL_INT < P and dc.SENTINEL == dc.SENTINEL_INT.to_bytes(16, "little") and dc.GUARD >= 3
    for case in dc.SMALL_GEO_CASES + dc.TREE_CASES:
        assert dc.SENTINEL_INT not in dc.points(case)
        for m in dc.lengths(case):
            for name in dc.evaluation_operands(m):
                coeffs = dc.coefficients(case, name)
                assert len(coeffs) == m and dc.SENTINEL_INT not in coeffs, (case.id, name)
                assert dc.packed_coefficients(case, name) == synth.pack_ints(coeffs), (case.id, name)
                if name[0] == "T" and m >= 4:
                    assert not any(coeffs[m - m // 4:]) and all(coeffs[:m - m // 4])
        for name in dc.INTERPOLATION_OPERANDS:
            vals = dc.interpolation_values(case, name)
            assert len(vals) == case.n and dc.SENTINEL_INT not in vals, (case.id, name)
            assert dc.packed_interpolation_values(case, name) == synth.pack_ints(vals), (case.id, name)


# ---- the models on every case they reach ---------------------------------------------------------------------------------------

def run_model(case, zerofier, evaluate, interpolate):
    outputs = []
    z = zerofier()
    dc.check_zerofier(case, z)
    outputs += z
    for m in dc.lengths(case):
        if m == 0:
            assert evaluate([]) == [0] * case.n
        for name in dc.evaluation_operands(m):
            got = evaluate(dc.coefficients(case, name))
            dc.check_values(case, name, got)
            outputs += got
    for name in dc.INTERPOLATION_OPERANDS:
        got = interpolate(dc.interpolation_values(case, name))
        got = got + [0] * (case.n - len(got))
        dc.check_interpolant(case, name, got)
        outputs += got
    assert dc.SENTINEL_INT not in outputs, "an expected value equals the sentinel"


@pytest.mark.parametrize("case", [c for c in dc.GEO_CASES if c.n <= MODEL_LIMIT], ids=lambda c: c.id)
def test_progression_model(case):
    dom = gm.GeometricDomain(case.first, case.ratio, case.n)
    assert tuple(dom.points()) == dc.points(case) and len(set(dc.points(case))) == case.n
    run_model(case, dom.zerofier, dom.evaluate, dom.interpolate)


@pytest.mark.parametrize("case", dc.TREE_CASES, ids=lambda c: c.id)
def test_tree_model(case):
    pts = list(dc.points(case))
    assert len(set(pts)) == case.n and pts.index(0) >= 2 and 1 in pts and P - 1 in pts
    tree = pm.Tree(pts)
    assert tree.pad == tree.K - case.n and tree.pad >= tree.K // 2 - 2           # all but the heaviest padding of its K
    run_model(case, tree.zerofier, lambda f: tree.evaluate_chunked(f, pts), tree.interpolate)


def test_big_cases_are_what_the_issue_names():
    assert dc.DEEP_CASE.n == (1 << 21) + 1 and dc.DEEP_CASE.first == po.GENERATOR and pow(dc.DEEP_CASE.ratio, 1 << 22, P) == P - 1
    assert dc.lengths(dc.DEEP_CASE) == (3, dc.DEEP_N, dc.DEEP_N + 1) and dc.lengths(dc.BIG_TREE_CASE) == (3, dc.BIG_TREE_K, dc.BIG_TREE_K + 1)
    assert {2047, 2048, 2049, 0, dc.DEEP_N - 2, dc.DEEP_N - 1} <= set(dc.sampled_positions(dc.DEEP_CASE))
    assert {0, dc.BIG_TREE_K - 1} <= set(dc.sampled_positions(dc.BIG_TREE_CASE))


@pytest.mark.parametrize("r", dc.REFUSALS, ids=lambda r: r.id)
def test_model_refuses_what_the_library_refuses(r):
    if r.n < 2 or not 0 < r.first < P or not 0 < r.ratio < P:
        return                                                        # argument checks: nothing to model
    with pytest.raises(ValueError, match="not distinct"):
        gm.GeometricDomain(r.first, r.ratio, r.n)
    pts = [r.first * pow(r.ratio, i, P) % P for i in range(r.n)]
    assert len(set(pts)) < r.n

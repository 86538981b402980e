"""Membership in a Rescue-Prime Merkle tree without a GPU: rescue_membership.RescueMembership's host specification (trace, boundary
conditions, public columns, constraints with public columns) against RescueMerkle and the plain-integer model of
tests/rescue_membership_cases.py; the constraints' structured form against their expansion into real MPolynomial dictionaries; a g++
build of the trace kernels' lane functions (tests/emu/rescue_membership_emu.cpp) against the model; every refusal of the host classes.

Traces here stay below 64 transitions: from 64 points on Polynomial.interpolate_domain takes the GPU."""
import ctypes
import functools
import os
import random
import subprocess

import pytest

from conftest import REPO
from algebra import FieldElement
from univariate import Polynomial
from multivariate import MPolynomial, XColumnsConstraint
import rescue_prime
import rescue_merkle
import rescue_membership
import rescue_membership_cases as mc
import rescue_wide_cases as wc

P = mc.P
EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = [os.path.join(REPO, "stark-anatomy_amd", "csrc", f) for f in ("field.cuh", "field_asm.cuh", "rescue_prime.cuh", "rescue_merkle.cuh")]
# (m, capacity, d, rounds, depth): depth (rounds + 1) transitions, all below 64
SETS = ((4, 1, 1, 3, 2), (5, 2, 1, 2, 3), (6, 1, 2, 1, 3), (7, 2, 2, 2, 1), (8, 3, 2, 27, 2), (8, 1, 3, 2, 2))
TINY = ((4, 1, 1, 1, 3), (6, 1, 2, 1, 2))         # T = 7 and 5 rows: small enough to expand into dictionaries


@functools.lru_cache(maxsize=None)
def scheme(m, capacity, d, rounds, depth):
    tree = rescue_merkle.RescueMerkle(rescue_prime.RescuePrime(m=m, capacity=capacity, rounds=rounds), digest_len=d)
    return rescue_membership.RescueMembership(tree, depth, expansion_factor=4, num_colinearity_checks=2, security_level=4)


@functools.lru_cache(maxsize=None)
def witness(m, capacity, d, rounds, depth, index):
    """(root, leaf digest, path) of leaf `index` of a tree of 2^depth seeded rows"""
    tree = scheme(m, capacity, d, rounds, depth).tree
    rng = random.Random(100 * m + depth)
    rows = [[rng.randrange(P) for _ in range(3)] for _ in range(1 << depth)]
    assert tree.verify(tree.commit(rows), index, tree.open(index, rows), rows[index])
    return tree.commit(rows), tree.leaf(rows[index]), tree.open(index, rows)


def indices_of(depth):
    return sorted({0, (1 << depth) - 1, 5 % (1 << depth)})


def values(trace):
    return [[v.value for v in row] for row in trace]


def nonzero_at(sch, rows):
    """{(transition, constraint)} where a constraint's evaluator does not vanish on the trace `rows` (lists of residues)"""
    at = [c.evaluator() for c in sch.transition_constraints()]
    fe = lambda v: FieldElement(v % P, sch.field)
    out, x = set(), sch.field.one()
    for t in range(len(rows) - 1):
        point = [x] + [fe(v) for v in rows[t]] + [fe(v) for v in rows[t + 1]]
        out |= {(t, i) for i, evaluate in enumerate(at) if evaluate(point).value != 0}
        x = x * sch.stark.omicron
    return out


@pytest.mark.parametrize("m,capacity,d,rounds,depth", SETS)
def test_host_trace_ends_in_the_root_and_equals_the_model(m, capacity, d, rounds, depth):
    sch = scheme(m, capacity, d, rounds, depth)
    assert (sch.W, sch.C, sch.T) == (m + d + 1, rounds + 1, depth * (rounds + 1) + 1) == (mc.registers(m, d), rounds + 1, mc.rows_of(depth, rounds))
    mds, rc = [v for row in sch.rp._mds for v in row], sch.rp._constants
    for index in indices_of(depth):
        root, leaf, path = witness(m, capacity, d, rounds, depth, index)
        rows = values(sch.trace(leaf, index, path))
        assert len(rows) == sch.T and all(len(r) == sch.W for r in rows)
        assert rows[-1][:d] == root == mc.walk(leaf, index, path, m, m - capacity, d, mds, rc, rounds)
        assert rows == mc.trace_rows(leaf, index, path, m, d, mds, rc, rounds)
        assert rows[0] == leaf + [0] * (sch.W - d)
        boundary = sch.boundary_constraints(root, leaf)
        assert sorted({s for _, s, _ in boundary}) == list(range(sch.W))                      # every register has a condition
        assert all(rows[cycle][s] == v.value for cycle, s, v in boundary) and len(boundary) == sch.W + d
        assert {cycle for cycle, _, _ in boundary} == {0, sch.T - 1}                          # none of them pins a secret row
        # a flipped index bit or a changed sibling: a walk that misses the root
        for j in range(depth):
            assert values(sch.trace(leaf, index ^ (1 << j), path))[-1][:d] != root
            changed = [list(s) for s in path]
            changed[j][j % d] = (changed[j][j % d] + 1) % P
            assert values(sch.trace(leaf, index, changed))[-1][:d] != root


@pytest.mark.parametrize("m,capacity,d,rounds,depth", SETS)
def test_constraints_vanish_on_honest_traces_only(m, capacity, d, rounds, depth):
    sch = scheme(m, capacity, d, rounds, depth)
    assert len(sch.transition_constraints()) == 2 * m + 1 and sch.transition_constraints() is sch.transition_constraints()
    assert len(sch.x_columns()) == 1 + 2 * m and sch.x_columns() is sch.x_columns()
    C, T = sch.C, sch.T
    for index in indices_of(depth):
        root, leaf, path = witness(m, capacity, d, rounds, depth, index)
        honest = values(sch.trace(leaf, index, path))
        assert nonzero_at(sch, honest) == set()
        if index != indices_of(depth)[-1]:
            continue
        j = depth - 1
        level = range(1 + j * C, 1 + (j + 1) * C)

        def changed(edit):
            rows = [list(r) for r in honest]
            edit(rows)
            return {t for t, _ in nonzero_at(sch, rows)}

        def set_register(register, value):
            def edit(rows):
                for t in level:
                    rows[t][register] = value(rows[t][register])
            return edit
        junction = j * C
        assert junction in changed(set_register(m + d, lambda v: 1 - v)), "a flipped index bit"
        assert junction in changed(set_register(m, lambda v: (v + 1) % P)), "a changed sibling"
        bit_two = [list(r) for r in honest]
        for t in level:
            bit_two[t][m + d] = 2
        assert (junction, m) in nonzero_at(sch, bit_two), "the constraint J bit (bit - 1) itself"

        def capacity_register(rows):
            rows[junction + 1][m - 1] = 1
        assert junction in changed(capacity_register), "a nonzero capacity register after a junction"

        def forged_root(rows):
            rows[T - 1][:d] = [(v + 1) % P for v in rows[T - 1][:d]]
        assert changed(forged_root) == {T - 2}, "a forged last row breaks the last round"


def expand(constraint, W):
    """the constraint as a real MPolynomial over [X, previous, next]: the columns substituted by MPolynomial arithmetic"""
    field = constraint.columns.polynomials[0].coefficients[0].field
    nvars = 1 + 2 * W
    variables = MPolynomial.variables(nvars, field)
    lifted = [MPolynomial.lift(Polynomial(q.coefficients[:q.degree() + 1]), 0) for q in constraint.columns.polynomials]
    powers = {}

    def power(base, key, e):
        if (key, e) not in powers:
            powers[(key, e)] = base ^ e
        return powers[(key, e)]
    acc = MPolynomial({})
    for exponents, coefficient in constraint.inner.dictionary.items():
        term = MPolynomial({(0,) * nvars: coefficient})
        for v, e in enumerate(exponents):
            if e:
                term = term * (power(variables[v], v, e) if v < nvars else power(lifted[v - nvars], v, e))
        acc = acc + term
    return acc


@pytest.mark.parametrize("m,capacity,d,rounds,depth", TINY)
def test_the_expanded_dictionaries_agree(m, capacity, d, rounds, depth):
    sch = scheme(m, capacity, d, rounds, depth)
    assert sch.T <= 9
    rng = random.Random(m)
    points = [[FieldElement(rng.randrange(P), sch.field) for _ in range(1 + 2 * sch.W)] for _ in range(3)]
    root, leaf, path = witness(m, capacity, d, rounds, depth, 1)
    honest = sch.trace(leaf, 1, path)
    points.append([sch.stark.omicron ^ 2] + honest[2] + honest[3])
    for i, constraint in enumerate(sch.transition_constraints()):
        assert type(constraint.dictionary) is not dict and constraint.value_domain_terms([1] * (1 + 2 * sch.W)) is NotImplemented
        plain = expand(constraint, sch.W)
        assert type(plain) is MPolynomial and max(k[0] for k in plain.dictionary) >= 1
        generic = XColumnsConstraint(constraint.inner, constraint.columns).evaluator()          # the inner dictionary, term by term
        structured, reference = constraint.evaluator(), plain.evaluator()
        for point in points:
            assert structured(point) == reference(point) == generic(point), i
        assert reference(points[-1]).value == 0
        assert sch.stark.transition_degree_bounds([constraint]) == sch.stark.transition_degree_bounds([plain]), i
    bounds = sch.stark.transition_degree_bounds(sch.transition_constraints())
    trace_degree, selector_degree = sch.stark.randomized_trace_length - 1, sch.x_columns().degrees[0]
    assert bounds[:m] == [selector_degree + 3 * trace_degree] * m and bounds[m] == selector_degree + 2 * trace_degree
    assert max(bounds) < sch.stark.omicron_domain_length
    # the host data flow's symbolic evaluation on an honest trace: the transition polynomial vanishes on the transitions
    x = Polynomial([sch.field.zero(), sch.field.one()])
    domain = [sch.stark.omicron ^ t for t in range(sch.T)]
    columns = [Polynomial.interpolate_domain(domain, [row[s] for row in honest]) for s in range(sch.W)]
    point = [x] + columns + [q.scale(sch.stark.omicron) for q in columns]
    junction = sch.transition_constraints()[m + 1]
    symbolic = junction.inner._evaluate_symbolic_host(point + junction.columns.polynomials)
    assert all(symbolic.evaluate(domain[t]).value == 0 for t in range(sch.T - 1)) and not symbolic.is_zero()


def build(target, extra):
    srcs = [os.path.join(EMU_DIR, "rescue_membership_emu.cpp")] + CSRC
    out = os.path.join(EMU_DIR, target)
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17"] + extra + ["-o", out, srcs[0]])
    return out


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(build("librescue_membership_emu.so", ["-O2", "-shared", "-fPIC"]))
    u64, vp, i = ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int
    lib.emu_rm_path_trace.restype = i
    lib.emu_rm_path_trace.argtypes = [i, vp, vp, vp, u64, i, i, i, vp, i, vp, i]
    return lib


@pytest.mark.parametrize("shape", mc.SHAPES)
def test_emulated_lane_functions_equal_the_model(emu, shape):
    for m, capacity, d, rounds, depth, k, kind in mc.kernel_cases():
        if (m, capacity, d) != shape:
            continue
        leaves, indices, paths = mc.packed_inputs(m, d, depth, kind, k)
        want = mc.expected_matrix(m, capacity, d, rounds, depth, kind, k)
        params = wc.params_bytes(*wc.seeded_params(m, rounds))
        idx = (ctypes.c_uint64 * k)(*indices)
        for split in (0, 1):
            out = ctypes.create_string_buffer(16 * len(want))
            assert emu.emu_rm_path_trace(m, leaves, idx, paths, k, depth, d, m - capacity, params, rounds, out, split) == 0
            got = wc.unpack(out.raw)
            assert got == want, (rounds, depth, k, kind, split, next(i for i in range(len(want)) if got[i] != want[i]))


def test_the_cases_cover_what_they_promise():
    cases = mc.kernel_cases()
    assert {c[:3] for c in cases} == set(mc.SHAPES) and all(2 * d < m - capacity for m, capacity, d in mc.SHAPES)
    assert {c[3] for c in cases} == {1, 2, 27} and {c[4] for c in cases} == {1, 2, 3, 63} and {c[6] for c in cases} == set(mc.KINDS)
    for m, capacity, d in mc.SHAPES:
        assert {c[5] for c in cases if c[:3] == (m, capacity, d)} >= set(mc.counts(m))
        words = {v for i in range(9) for s in mc.item(m, d, 3, "random", i)[2] for v in s}
        assert {0, P - 1, P, wc.TOP} <= words                                              # sibling words 0, p - 1 and words >= p
    assert mc.item(6, 2, 63, "random", 0)[1] >> 62 == 1


def test_standalone_program_under_sanitizers():
    """the emulated code with a main of its own, built with ASan + UBSan and run as a program: every width on buffers of exactly the
    promised size, both forms, every element written"""
    program = build("rescue_membership_emu_main", ["-DRESCUE_MEMBERSHIP_MAIN", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                   "-fno-omit-frame-pointer"])
    done = subprocess.run([program], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert done.returncode == 0 and "rescue membership ok" in done.stdout, (done.stdout + done.stderr)[-2000:]


def test_refusals():
    rp = rescue_prime.RescuePrime(m=4, capacity=1, rounds=1)
    for bad in (rescue_merkle.RescueMerkle(rescue_prime.RescuePrime(m=3, capacity=1, rounds=1)),          # rate 2: 2 d = rate
                rescue_merkle.RescueMerkle(rescue_prime.RescuePrime(m=4, capacity=2, rounds=1)),          # rate 2
                rescue_merkle.RescueMerkle(rp, digest_len=2),                                             # 2 d = 4 > rate
                rescue_merkle.RescueMerkle(rescue_prime.RescuePrime(m=8, capacity=1, rounds=1), digest_len=4)):
        with pytest.raises(AssertionError, match="one permutation"):
            rescue_membership.RescueMembership(bad, 2, 4, 2, 4)
    tree = rescue_merkle.RescueMerkle(rp)
    for depth in (0, 64):
        with pytest.raises(AssertionError, match="a depth of 1 .. 63"):
            rescue_membership.RescueMembership(tree, depth, 4, 2, 4)
    sch = rescue_membership.RescueMembership(tree, 2, 4, 2, 4)
    with pytest.raises(AssertionError, match="cannot verify invalid index"):
        sch.trace([1], 4, [[2], [3]])
    with pytest.raises(AssertionError, match="cannot verify invalid index"):
        sch.trace([1], -1, [[2], [3]])
    with pytest.raises(AssertionError, match="`depth` entries"):
        sch.trace([1], 0, [[2]])
    with pytest.raises(AssertionError, match="digest_len elements"):
        sch.trace([1, 2], 0, [[2], [3]])
    with pytest.raises(AssertionError, match="digest_len elements"):
        sch.trace([1], 0, [[2], [3, 4]])
    with pytest.raises(AssertionError, match="digest_len elements"):
        sch.boundary_constraints([1, 2], [1])
    constraint = sch.transition_constraints()[0]
    for operation in (lambda: constraint + constraint, lambda: constraint * constraint, lambda: -constraint, lambda: constraint ^ 2):
        with pytest.raises(TypeError):
            operation()
    assert sch.stark._combination_tables(sch.transition_constraints()) is None                # verify_batch keeps the host loop

"""tests/vector_primitive_cases.py on the host: every shape is where the table of tests/test_gpu_vector_primitives.py says it is, worked
out from the same constants of stark-anatomy_amd/csrc/core.hip, and the expectations agree with the C oracle where it has the
operation (scale, pointwise product and quotient, fold).  No GPU, no library."""
import pytest

from oracle import py_oracle as po
import vector_primitive_cases as vc

C = po.C
P = po.P


def test_operands_are_canonical_and_carry_every_edge_residue():
    vals = vc.operands(1, 64)
    assert all(0 <= v < P for v in vals) and set(vc.EDGES) <= set(vals[0::3])
    assert all(all(vc.divisors(2, 300, s)) for s in range(5)) and set(vc.NONZERO_EDGES) <= set(vc.divisors(2, 64)[0::3])
    assert int.from_bytes(vc.SENTINEL, "little") >= P                       # no residue: a kernel cannot produce it
    assert all(0 <= f < P for _, f in vc.SCALE_FACTORS + vc.SLAB_FACTORS) and all(0 <= v < P for v in vc.FIELD_EDGES)
    w = po.primitive_nth_root(8192)
    assert pow(w, 4096, P) == P - 1 and dict(vc.SCALE_FACTORS)["root of order 8192"] == w      # the high table alternates 1, -1


def test_the_high_power_table_is_read_above_its_first_entry():
    """claim 1: each of the slab scale, the twiddle matrix and the slab fold has an exponent from 4096 up and one with e >> 12 >= 2"""
    for name, shapes, exponents in (("scale slab", vc.SLAB_SHAPES, vc.slab_exponents), ("twiddle matrix", vc.TWIDDLE_SHAPES, vc.twiddle_exponents),
                                    ("fold slab", vc.FOLD_SLAB_SHAPES, vc.fold_slab_exponents)):
        top = [max(exponents(s)) for s in shapes]
        assert any(t >= 4096 for t in top), name                          # past the low table ...
        assert any(t >> 12 >= 2 for t in top), name                       # ... and past the second entry of the high one
        assert any(t < 4096 for t in top), name
    assert max(vc.slab_exponents((3, 4, 2048, 2044))) == 6143
    assert vc.slab_exponents((5, 1, 4097, 4096)) == [4096, 8193, 12290, 16387, 20484]
    assert max(vc.twiddle_exponents((8, 4, 1020, 1020, 1 << 21))) == 1027 * 1023 and (1027 * 1023) >> 12 == 256
    assert sorted(vc.fold_slab_exponents((4, 8, 4096, 4088))) == list(range(4088, 4096)) + list(range(8184, 8192))
    assert max(vc.fold_slab_exponents((16, 1, 1024, 1023))) == 8191
    assert max(vc.fold_slab_exponents((8, 2, 4096, 4094))) == 16383
    # every exponent has its entry: below the order (twiddle matrix, whose tables have `order` powers) and below the count handed to get_pow
    for s in vc.TWIDDLE_SHAPES:
        assert max(vc.twiddle_exponents(s)) < s[4], s
    assert max(vc.twiddle_exponents(vc.TWIDDLE_SHAPES[-1])) == 63 and max(vc.twiddle_exponents(vc.TWIDDLE_REFUSED)) == 64 == vc.TWIDDLE_REFUSED[4]
    for s in vc.SLAB_SHAPES:
        assert max(vc.slab_exponents(s)) < s[0] * s[2] and s[1] & (s[1] - 1) == 0 and s[3] + s[1] <= s[2], s
    for s in vc.FOLD_SLAB_SHAPES:
        assert max(vc.fold_slab_exponents(s)) < s[0] * s[2] // 2 and s[3] + s[1] <= s[2], s
    bad_cols, past_end = vc.SLAB_REFUSED
    assert bad_cols[1] == 3 and past_end[3] + past_end[1] == past_end[2] + 1


def test_scale_sizes_sit_on_both_sides_of_every_table_size():
    """claim 2: the high table has 1, 2 and 4 entries, and the run of one factor moves between all three"""
    entries = {n: vc.hi_entries(n) for n in vc.SCALE_SIZES}
    assert set(entries.values()) == {1, 2, 4}
    assert [entries[n] for n in (4095, 4096, 8191, 8192)] == [1, 2, 2, 4]
    assert max(n - 1 for n in vc.SCALE_SIZES) >> 12 == 3                    # exponent 12288: the last entry of a table of four
    run = [vc.hi_entries(n) for n in vc.SCALE_ORDER_RUN]
    assert run == [2, 1, 4, 2] and all(a != b for a, b in zip(run, run[1:]))
    assert not {f for f in vc.SCALE_ORDER_FACTORS} & {f for _, f in vc.SCALE_FACTORS}


def test_strided_degree_cases_reach_the_second_step():
    """claim 3: more entries than the capped grid takes in one step, leaders in both steps, decoys that share the leader's result word"""
    assert vc.DEGREE_WG == 256 * vc.DEGREE_PER_THREAD and vc.DEGREE_STEP == vc.DEGREE_MAX_BLOCKS * vc.DEGREE_WG
    assert vc.DEGREE_STRIDED_SCANNED > vc.DEGREE_STEP and vc.DEGREE_STRIDED_N - vc.DEGREE_TOP == vc.DEGREE_STRIDED_SCANNED
    assert (vc.DEGREE_STRIDED_SCANNED + vc.DEGREE_WG - 1) // vc.DEGREE_WG > vc.DEGREE_MAX_BLOCKS      # the grid is capped
    cases = vc.degree_strided_cases()
    steps = [vc.degree_workgroup(lead)[1] for lead, _, _ in cases]
    assert steps == [0, 0, 1, 1, 1] and cases[-1][0] == vc.DEGREE_STRIDED_SCANNED - 1
    for lead, same, other in cases:
        assert same and all(0 <= d < lead for d in same + other), lead
        for d in same:
            assert (vc.degree_workgroup(d)[0] - vc.degree_workgroup(lead)[0]) % vc.DEGREE_SLOTS == 0, (lead, d)
        if lead >= vc.DEGREE_STEP:                                            # a leader of the second step has a decoy in another workgroup of the first
            assert any(vc.degree_workgroup(d) != vc.degree_workgroup(lead) and vc.degree_workgroup(d)[1] == 0 for d in same), lead
            assert other == [vc.DEGREE_STEP - 1]
            assert lead % vc.DEGREE_STEP < max(same + other)                  # index arithmetic that forgets the step ranks the leader below its decoys
    small = vc.degree_small_cases()
    assert {n for n, _, _ in small} == set(vc.DEGREE_SMALL_SIZES)
    assert all(lead < n and (decoy is None or 0 <= decoy < lead) for n, lead, decoy in small)
    assert {lead for n, lead, _ in small if n == 1025} == {-1, 0, 63, 64, 255, 256, 1023, 1024}
    assert max(vc.DEGREE_SMALL_SIZES) < vc.DEGREE_TOP                         # one launch each


def test_columns_degree_cases_stride_and_take_a_second_launch():
    """claim 4"""
    n = vc.DEGREE_COLS_STRIDED["n"]
    assert n > vc.DEGREE_COL_PARTS * 256 * vc.DEGREE_PER_THREAD
    assert (n + vc.DEGREE_WG - 1) // vc.DEGREE_WG > vc.DEGREE_COL_PARTS       # the workgroups per column are capped
    (lead0, decoy0), (lead1, decoy1), (lead2, _) = vc.DEGREE_COLS_STRIDED_LEADS
    step = vc.DEGREE_COL_PARTS * vc.DEGREE_WG
    assert (lead0 % step // vc.DEGREE_WG, lead0 // step) == (0, 1) and (lead1 % step // vc.DEGREE_WG, lead1 // step) == (vc.DEGREE_COL_PARTS - 1, 0)
    assert lead2 == -1 and decoy0 < lead0 < n and decoy1 < lead1 < n
    cols = vc.DEGREE_COLS_MANY["cols"]
    assert cols > vc.DEGREE_COLS_PER_LAUNCH
    want = vc.degree_cols_many_expected()
    # every degree from -1 to 2 in the first launch, right up to its last column; -1, 0 and 1 in the three columns of the second
    assert set(want[:vc.DEGREE_COLS_PER_LAUNCH]) == {-1, 0, 1, 2} and want[vc.DEGREE_COLS_PER_LAUNCH - 1] == 2
    assert want[vc.DEGREE_COLS_PER_LAUNCH:] == [-1, 0, 1]
    vals = vc.degree_cols_many_values()
    assert len(vals) == 4 * cols and all(vals[4 * c + 3] for c in range(cols))      # junk between the columns
    assert [po.degree(vals[4 * c:4 * c + 3]) for c in range(cols)] == want


def test_division_shapes_by_layout():
    """claim 5: (workgroups, full threads, partial threads, padding slots) of every shape for K = 16 and K = 8.  Thread t takes the
    elements t, t + T, t + 2 T, ... of T threads in all, so the padding sits in every thread's last slots -- no thread is "the"
    partial one except at n = 1, and since the first slot of thread t is element t < ceil(n / K) <= n in every workgroup but
    possibly the last, no workgroup is padding only: asserted below for every shape, instead of the class that cannot occur."""
    for K in vc.DIV_KS:
        layout = {n: vc.div_layout(n, K) for n in vc.DIV_SIZES[K]}
        assert layout[1] == (1, 0, 1, 256 * K - 1, 0)                                   # one partial thread
        assert layout[K - 1][:3] == (1, 0, K - 1) and layout[K][:3] == (1, 0, K) and layout[K + 1][:3] == (1, 0, K + 1)
        assert layout[256 * K] == (1, 256, 0, 0, 0)                                     # exactly one full workgroup, no padding
        assert layout[256 * K - 1] == (1, 255, 1, 1, 0)                                 # one padding slot, next to real ones
        assert layout[256 * K + 1] == (2, 0, 512, 512 * K - 256 * K - 1, 0)            # two workgroups, every thread half padding
        assert all(l[4] == 0 for l in layout.values())
        assert set(vc.DIV_ZERO_SIZES[K]) <= set(vc.DIV_SIZES[K])
    assert vc.div_layout(8193, 16)[0] == 3
    assert vc.div_companions(4097, 16, 4096) == {512 * k for k in range(9)} and vc.div_companions(17, 16, 5) == {5}
    for n in vc.DIV_SIZES[16] + vc.DIV_SIZES[8]:
        a, b = vc.div_operands(n)
        assert all(b) and (n < 15 or 0 in a)
        assert vc.pack(vc.div_expected(n)) == C.pointwise_div(vc.pack(a), vc.pack(b), n), n


def test_mpoly_payloads_sit_on_both_sides_of_the_kernel_argument_limit():
    """claim 6"""
    cases = vc.mpoly_cases()
    assert vc.SMALL_PAYLOAD == 8192
    sizes = {name: vc.mpoly_payload(nvars, terms) for name, (nvars, n, terms) in cases.items()}
    assert sizes["512 terms: coefficients at the limit"] == (8192, 512)
    assert sizes["513 terms: coefficients over the limit"] == (8208, 513)
    assert sizes["482 terms of 17 variables: exponents over the limit"] == (7712, 8194)
    assert sizes["no term"] == (16, 0)
    for name, (nvars, n, terms) in cases.items():
        assert 1 <= nvars <= 255 and all(len(e) == nvars and max(e, default=0) <= 255 and 0 <= c < P for e, c in terms), name
    assert any(255 in e for e, _ in cases["255 variables of 2 points"][2]) and cases["255 variables of 2 points"][0] == 255
    assert all(max(e) <= 2 for name in sizes if "terms" in name for e, _ in cases[name][2])
    for n, turns in vc.MPOLY_ROT_CASES.values():
        assert n & (n - 1) == 0
    a, b = [vc.MPOLY_ROT_CASES[k] for k in ("n = 256, turns 3 and n - 1", "n = 256, turns n + 3 and 2 n - 1")]
    assert vc.mpoly_rot_expected(*a) == vc.mpoly_rot_expected(*b) and max(b[1]) >= b[0] and a[1][1] == a[0] - 1


def test_expectations_agree_with_the_c_oracle():
    for n in vc.SCALE_SIZES:
        for _, f in vc.SCALE_FACTORS:
            assert vc.pack(vc.scale_expected(n, f)) == C.scale(vc.pack(vc.scale_input(n)), n, f), (n, f)
    f = dict(vc.SCALE_FACTORS)["zero"]
    assert vc.scale_expected(257, f) == [vc.scale_input(257)[0]] + [0] * 256                      # 0^0 = 1
    for shape in vc.SLAB_SHAPES:                                       # a slab is the whole vector's scaling read at the slab's places
        rows, cols, row_len, col_base = shape
        whole = [0] * (rows * row_len)
        for v, e in zip(vc.slab_input(shape), vc.slab_exponents(shape)):
            whole[e] = v
        for _, f in vc.SLAB_FACTORS:
            scaled = vc.unpack(C.scale(vc.pack(whole), len(whole), f))
            assert vc.slab_expected(shape, f) == [scaled[e] for e in vc.slab_exponents(shape)], (shape, f)
    for n in vc.MUL_SIZES[1:]:
        a, b = vc.mul_operands(n)
        assert vc.pack([x * y % P for x, y in zip(a, b)]) == C.pointwise_mul(vc.pack(a), vc.pack(b), n)
    assert len(vc.EDGE_PAIRS) == 225 and vc.mul_operands(257)[0][:225] == [x for x, _ in vc.EDGE_PAIRS]


@pytest.mark.parametrize("N", sorted({s[0] * s[2] for s in vc.FOLD_SLAB_SHAPES} | set(vc.FOLD_SIZES)))
def test_fold_expectations_agree_with_the_c_oracle(N):
    for _, alpha in vc.ALPHAS if N < 1 << 15 else vc.ALPHAS[2:]:          # (the GPU test runs the 2^15 codeword with p - 1 and the random alpha)
        assert vc.pack(vc.fold_expected(N, alpha)) == C.fold(vc.pack(vc.codeword(N)), N, alpha, po.GENERATOR, po.primitive_nth_root(N)), (N, alpha)


def test_axpy_and_gather_cases():
    for shape in vc.AXPY_SHAPES:
        n_acc, n_src, shift = shape
        acc, src = vc.axpy_operands(shape)
        assert shift + n_src <= n_acc and len(acc) == n_acc and len(src) == n_src and P - 1 in acc
        out = vc.axpy_expected(shape, P - 1)
        assert out[:shift] == list(acc[:shift]) and out[shift + n_src:] == list(acc[shift + n_src:])
    wraps = vc.axpy_expected((300, 100, 57), 1)
    acc, src = vc.axpy_operands((300, 100, 57))
    assert any(a + s >= P for a, s in zip(acc[57:], src)) and all(0 <= v < P for v in wraps)
    (_, _, shift_a, _), (_, n_b, shift_b, _), (_, _, _, w_c) = vc.AXPY_REFUSED
    assert shift_a + 100 == 301 and (shift_b + n_b) % (1 << 64) < shift_b and w_c == P
    for k in vc.GATHER_COUNTS:
        idx = vc.gather_indices(k)
        assert len(idx) == k and all(0 <= i < vc.GATHER_N for i in idx) and (k < 2 or len(set(idx)) < k or k <= vc.GATHER_N)
    assert len(set(vc.gather_indices(1000))) < 1000 and vc.GATHER_N - 1 in vc.gather_indices(1)

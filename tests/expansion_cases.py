"""Instances for the proofs at expansion factors other than 4 (tests/golden/expansion.json; tests/test_expansion_factors_cpu.py,
tests/test_gpu_expansion_factors.py) -- the workloads of workloads.py restated for any expansion factor, and the places of a
FastStark proof stream that the recorded alterations change.  tests/golden/make_golden.py --expansion imports this module with
the REFERENCE's algebra / multivariate on its path (it hands them in), the tests with the package's: the same trace, constraints
and boundary on either side.  Nothing here runs on a GPU."""
import itertools


def pack(column):
    return b"".join(map(int.to_bytes, column, itertools.repeat(16), itertools.repeat("little")))


def trace_length(log_fri, expansion_factor, s):
    """T with a randomized trace of T + 4 s = 2^(log_fri - 2 - log2 ef) rows: the omicron domain (twice the next power of two,
    constraints of degree 2) then has 2^(log_fri - log2 ef) points and the FRI domain 2^log_fri"""
    assert expansion_factor & (expansion_factor - 1) == 0
    return (1 << (log_fri - 2 - (expansion_factor.bit_length() - 1))) - 4 * s


def _modules(algebra, multivariate):
    if algebra is None:
        import algebra
    if multivariate is None:
        import multivariate
    return algebra, multivariate


def synthetic_instance(log_fri, expansion_factor, s, algebra=None, multivariate=None):
    """workloads.synthetic_stark_instance -- the 2-register AIR (a, b) -> (b, a*a + b) -- for any expansion factor.
    Returns (field, T, packed columns, host rows, air, boundary)."""
    import synth
    algebra, multivariate = _modules(algebra, multivariate)
    field = algebra.Field.main()
    fe = lambda v: algebra.FieldElement(v, field)
    T = trace_length(log_fri, expansion_factor, s)
    assert T >= 2, (log_fri, expansion_factor, s)
    col_a, col_b = synth.synthetic_air_columns(T)
    rows = [[fe(a), fe(b)] for a, b in zip(col_a, col_b)]
    v = multivariate.MPolynomial.variables(5, field)                  # X, a, b, a', b'
    air = [v[3] - v[2], v[4] - v[1] * v[1] - v[2]]
    boundary = [(0, 0, fe(col_a[0])), (0, 1, fe(col_b[0])), (T - 1, 1, fe(col_b[T - 1]))]
    return field, T, [pack(col_a), pack(col_b)], rows, air, boundary


def wide_instance(log_fri, registers, expansion_factor, s, algebra=None, multivariate=None):
    """workloads.synthetic_wide_instance -- r_i' = r_i^2 + r_((i+1) mod w), row 0 = (7 i + 3); boundary: every register's first
    cell and register 0's last -- for any expansion factor.  Returns (field, T, packed columns, host rows, air, boundary)."""
    algebra, multivariate = _modules(algebra, multivariate)
    field = algebra.Field.main()
    fe = lambda v: algebra.FieldElement(v, field)
    w = registers
    T = trace_length(log_fri, expansion_factor, s)
    assert T >= 2, (log_fri, expansion_factor, s)
    row, ints = [7 * i + 3 for i in range(w)], []
    for _ in range(T):
        ints.append(row)
        row = [(row[i] * row[i] + row[(i + 1) % w]) % field.p for i in range(w)]
    rows = [[fe(x) for x in r] for r in ints]
    v = multivariate.MPolynomial.variables(1 + 2 * w, field)          # X, r_0 .. r_(w-1), r_0' .. r_(w-1)'
    air = [v[1 + w + i] - v[1 + i] * v[1 + i] - v[1 + (i + 1) % w] for i in range(w)]
    boundary = [(0, i, fe(ints[0][i])) for i in range(w)] + [(T - 1, 0, fe(ints[T - 1][0]))]
    return field, T, [pack([r[i] for r in ints]) for i in range(w)], rows, air, boundary


def false_claim(boundary, one):
    """the boundary with its last value one higher"""
    c, r, v = boundary[-1]
    return boundary[:-1] + [(c, r, v + one)]


def opened_positions(top_level_indices, expansion_factor, domain_length):
    """fast_stark.py:154-156: {i, i + ef, i + N/2, i + ef + N/2} for every sampled index, sorted"""
    twice = list(top_level_indices) + [(i + expansion_factor) % domain_length for i in top_level_indices]
    return sorted(twice + [(i + domain_length // 2) % domain_length for i in twice])


def alteration_places(num_objects, registers, expansion_factor, domain_length, top_level_indices):
    """Objects of a FastStark proof stream to change, from the END of the stream: it closes with (leaf, path) at every opened
    position for each register's boundary quotient codeword, then the randomizer codeword, then the transition zerofier codeword
    (fast_stark.py:158-175).  The companion positions index + ef are where trace(omicron X) is read."""
    opened = opened_positions(top_level_indices, expansion_factor, domain_length)
    per_codeword = 2 * len(opened)
    base = num_objects - (registers + 2) * per_codeword
    first = top_level_indices[0]
    companion = (first + expansion_factor) % domain_length
    far_companion = (companion + domain_length // 2) % domain_length
    at = lambda codeword, position: base + codeword * per_codeword + 2 * opened.index(position)
    return [
        {"what": "register 0, leaf at a companion position index + ef", "object": at(0, companion), "how": "add one", "position": companion, "companion_of": first},
        {"what": "register 0, path of that opening", "object": at(0, companion) + 1, "how": "flip a bit of digest 0", "position": companion, "companion_of": first},
        {"what": "last register, leaf at index + ef + N/2", "object": at(registers - 1, far_companion), "how": "add one", "position": far_companion, "companion_of": first},
        {"what": "randomizer codeword, value at a sampled index", "object": at(registers, first), "how": "add one", "position": first},
        {"what": "transition zerofier codeword, path at a companion position", "object": at(registers + 1, companion) + 1, "how": "flip a bit of the last digest", "position": companion,
         "companion_of": first},
    ]


def altered(objects, place, one):
    """the stream's objects with `place` (an entry of alteration_places) applied; one = field.one() of the objects' field"""
    out = list(objects)
    target = out[place["object"]]
    if place["how"] == "add one":
        assert not isinstance(target, (list, tuple, bytes)), type(target)
        out[place["object"]] = target + one
    else:
        assert isinstance(target, list) and isinstance(target[0], bytes), type(target)
        k = 0 if place["how"] == "flip a bit of digest 0" else len(target) - 1
        out[place["object"]] = target[:k] + [bytes([target[k][0] ^ 1]) + target[k][1:]] + target[k + 1:]
    return out

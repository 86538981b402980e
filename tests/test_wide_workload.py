"""The wide workload (workloads.synthetic_wide_instance) on the CPU, in plain ints: the trace satisfies its own AIR and boundary
on every row, and the golden record of the reference's proofs of it (tests/golden/fast_stark_wide.json, make_wide_golden.py) is
the one the GPU tests compare against."""
from conftest import load_golden


def test_wide_instance_satisfies_its_air_and_boundary_on_every_row():
    import workloads
    log_fri, w, s = 10, 16, 8
    field, T, rows, packed, air, boundary = workloads.synthetic_wide_instance(log_fri, w, s)
    p = field.p
    assert T == (1 << (log_fri - 4)) - 4 * s == 32
    assert len(rows) == T and all(len(row) == w for row in rows) and len(packed) == w and len(air) == w
    ints = [[e.value for e in row] for row in rows]
    assert ints[0] == [7 * i + 3 for i in range(w)]
    for c in range(w):
        assert packed[c] == b"".join(ints[t][c].to_bytes(16, "little") for t in range(T))
    # the transition, restated
    for t in range(T - 1):
        for i in range(w):
            assert ints[t + 1][i] == (ints[t][i] ** 2 + ints[t][(i + 1) % w]) % p
    # the AIR polynomials themselves, term by term in ints: sum coef * prod point^exponent over (X, row, next row) vanishes
    for t in range(T - 1):
        point = [0] + ints[t] + ints[t + 1]
        for i, a in enumerate(air):
            total = 0
            for exponents, coefficient in a.dictionary.items():
                assert len(exponents) == 1 + 2 * w
                term = coefficient.value
                for x, e in zip(point, exponents):
                    if e:
                        term = term * pow(x, e, p) % p
                total = (total + term) % p
            assert total == 0, (t, i)
    # one constraint per register, each of degree 2 in its own register and linear in its neighbour and successor
    for i, a in enumerate(air):
        used = sorted({j for exponents in a.dictionary for j, e in enumerate(exponents) if e})
        assert used == sorted({1 + i, 1 + (i + 1) % w, 1 + w + i})
    assert len(boundary) == w + 1
    assert [(c, r) for c, r, _ in boundary] == [(0, i) for i in range(w)] + [(T - 1, 0)]
    for cycle, register, value in boundary:
        assert value.value == ints[cycle][register]


def test_wide_golden_holds_both_records():
    runs = load_golden("fast_stark_wide.json")["runs"]
    assert [(r["log_fri"], r["registers"], r["num_colinearity_checks"], r["urandom_seed"]) for r in runs] == [(10, 16, 8, 31), (12, 16, 8, 31)]
    for r, (length, prefix) in zip(runs, [(467157, "9a649f9d6070b141"), (581796, "d15bdb0e3dedbcc3")]):
        assert r["expansion_factor"] == 4 and r["security_level"] == 16 and r["verifies"] is True
        assert r["original_trace_length"] == (1 << (r["log_fri"] - 4)) - 32 and r["fri_domain_length"] == 1 << r["log_fri"]
        assert r["proof_len"] == length and r["proof_sha256"].startswith(prefix) and len(r["proof_sha256"]) == 64
        assert "proof" not in r                            # digests only, no proof bytes

#!/usr/bin/env python3
"""Generate tests/golden/fast_stark_wide.json by importing the reference implementation.

The wide workload of workloads.synthetic_wide_instance -- w registers, r_i' = r_i^2 + r_((i+1) mod w), row 0 = (7 i + 3),
T = 2^(log_fri - 4) - 4 s rows, boundary = every register's first cell and register 0's last -- proven by the REFERENCE's
FastStark(field, 4, s, 2 s, w, T) with os.urandom replaced by a seeded generator.  Only DATA is written: the parameters, the
proof's length and its SHA-256 (no proof bytes); no reference source is copied.  The instance is restated here with the
reference's own classes, so the record does not depend on this repository's workloads.py.

usage:  python tests/golden/make_wide_golden.py REFERENCE_CODE_DIR [log_fri:registers:s:seed ...]
        (default records: 10:16:8:31 and 12:16:8:31 -- about 12 s and 2 minutes of reference proving)

make_golden.py --expansion calls prove_with_reference with another expansion factor (T = 2^(log_fri - 2 - log2 ef) - 4 s) and puts
that record into expansion.json; this file's own records stay at expansion factor 4.
"""
import hashlib
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def prove_with_reference(log_fri, w, s, seed, ef=4, describe=None):
    """ef: the expansion factor (the records of fast_stark_wide.json have 4; make_golden.py --expansion asks for another and writes
    its record elsewhere); describe(stark, proof, air, boundary, zerofier_root, top_level_indices): further fields of the record"""
    import algebra as ref_algebra
    import fast_stark as ref_fast_stark
    import multivariate as ref_multivariate
    field = ref_algebra.Field.main()
    fe = lambda v: ref_algebra.FieldElement(v, field)
    rng = random.Random(seed)
    ref_fast_stark.os.urandom = lambda k, rng=rng: bytes(rng.getrandbits(8) for _ in range(k))
    T = (1 << (log_fri - 2 - (ef.bit_length() - 1))) - 4 * s
    row, rows = [7 * i + 3 for i in range(w)], []
    for _ in range(T):
        rows.append(row)
        row = [(row[i] * row[i] + row[(i + 1) % w]) % field.p for i in range(w)]
    trace = [[fe(v) for v in r] for r in rows]
    v = ref_multivariate.MPolynomial.variables(1 + 2 * w, field)
    air = [v[1 + w + i] - v[1 + i] * v[1 + i] - v[1 + (i + 1) % w] for i in range(w)]
    boundary = [(0, i, fe(rows[0][i])) for i in range(w)] + [(T - 1, 0, fe(rows[T - 1][0]))]
    stark = ref_fast_stark.FastStark(field, ef, s, 2 * s, w, T)
    assert stark.fri_domain_length == 1 << log_fri, (stark.fri_domain_length, log_fri)
    sampled, fri_prove = [], stark.fri.prove
    stark.fri.prove = lambda codeword, proof_stream: (sampled.append(fri_prove(codeword, proof_stream)), sampled[-1])[1]
    tz, tzc, tzr = stark.preprocess()
    t0 = time.time()
    proof = stark.prove(trace, air, boundary, tz, tzc)
    seconds = time.time() - t0
    ok = stark.verify(proof, air, boundary, tzr)
    rec = {"log_fri": log_fri, "registers": w, "num_colinearity_checks": s, "urandom_seed": seed, "expansion_factor": ef, "security_level": 2 * s,
           "original_trace_length": T, "omicron_domain_length": stark.omicron_domain_length, "fri_domain_length": stark.fri_domain_length,
           "zerofier_root": tzr.hex(), "proof_len": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest(), "verifies": ok,
           "reference_prove_seconds": round(seconds, 1)}
    if describe is not None:
        rec.update(describe(stark, proof, air, boundary, tzr, sampled[0]))
    return rec


if __name__ == "__main__":
    if len(sys.argv) < 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    sys.setrecursionlimit(10000)
    cases = [tuple(int(x) for x in a.split(":")) for a in sys.argv[2:]] or [(10, 16, 8, 31), (12, 16, 8, 31)]
    path = os.path.join(HERE, "fast_stark_wide.json")
    key = lambda r: (r["log_fri"], r["registers"], r["num_colinearity_checks"], r["urandom_seed"])
    for case in cases:
        rec = prove_with_reference(*case)
        out = {"runs": []}
        if os.path.exists(path):
            with open(path) as f:
                out = json.load(f)
        out["runs"] = sorted([r for r in out["runs"] if key(r) != key(rec)] + [rec], key=key)
        with open(path, "w") as f:
            json.dump(out, f, indent=0, separators=(",", ":"))
            f.write("\n")
        print("wide AIR, fri 2^%d w=%d s=%d seed %d: prove %.1fs, %d bytes, sha256 %s, verifies %s"
              % (case + (rec["reference_prove_seconds"], rec["proof_len"], rec["proof_sha256"][:16], rec["verifies"])), flush=True)

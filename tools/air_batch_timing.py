#!/usr/bin/env python3
"""FastStark.transition_quotients_batch against K calls of the per-member method at the signature scheme's shape, on one MI355X (dev tool).

usage: air_batch_timing.py [--reps 15] [--ks 1,4,16,64] [--json OUT]

The shape is FastRPSSS().stark's (284 trace rows, omicron domain 2^10, the two Rescue-Prime transition constraints).  Per K: K members
from K random secret keys, their traces randomized as `prove` randomizes them, the K x 2 trace polynomials interpolated as the rows of
one matrix, the points built as `prove` builds them.  One repetition computes the K members' transition quotients once through
transition_quotients_batch and once through K calls of _transition_quotients_on_device as `prove` makes them (pending=None: both wait
for the "divide by zero" verdict, and both end with the degrees on the host, so the host clock around a call is the time to the
finished quotients), the two alternating so that both see the same machine.  Every timed window holds `inner` calls (at least 16
members' worth).  The first repetition of every K is a warm-up, checks that both give the same coefficients, and is dropped.  Median
and range in ms per member, and the products per point and constraint of the two evaluation plans."""
import argparse, json, os, random, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
sys.setrecursionlimit(10000)
import starkcore as sc
import fast_rpsss
from algebra import FieldElement
from ntt import DevicePolynomial, fast_interpolate_columns_device
from starkcore import DeviceCodeword, DeviceVector
from univariate import Polynomial

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--ks", default="1,4,16,64")
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)

scheme = fast_rpsss.FastRPSSS()
stark, rp, field = scheme.stark, scheme.rp, scheme.field
air = rp.transition_constraints(stark.omicron)
zerofier = stark._lift(scheme.transition_zerofier)
rng = random.Random(7)
rows = stark.randomized_trace_length
print("shape: %d trace rows, omicron domain 2^%d, FRI domain 2^%d, %d constraints" %
      (rows, stark.omicron_domain_length.bit_length() - 1, stark.fri_domain_length.bit_length() - 1, len(air)), flush=True)


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def product_counts():
    """per constraint (term by term: every exponent; Horner in the variable of highest exponent: its maximum + the others')"""
    out = []
    for a in air:
        _, terms = a.value_domain_terms([1] + [rows - 1] * (2 * stark.num_registers))
        tops = [max(k[j] for k, _ in terms) for j in range(len(terms[0][0]))]
        h = tops.index(max(tops))
        out.append({"terms": len(terms), "highest_exponents": tops, "term_by_term": sum(sum(k) for k, _ in terms),
                    "horner": tops[h] + sum(sum(k) - k[h] for k, _ in terms)})
    return out


def make_points(K):
    columns = []
    for _ in range(K):
        trace = rp.trace(FieldElement(rng.randrange(field.p), field))
        trace = [[e.value for e in row] for row in trace] + [[rng.randrange(field.p) for _ in range(stark.num_registers)] for _ in range(stark.num_randomizers)]
        columns += [[row[s] for row in trace] for s in range(stark.num_registers)]
    matrix = DeviceVector.from_ints([v for column in columns for v in column])
    views = [DeviceCodeword(DeviceVector.wrap(matrix.ptr + 16 * rows * c, rows, matrix), field) for c in range(len(columns))]
    polynomials = [DevicePolynomial.from_codeword(c) for c in fast_interpolate_columns_device(stark._trace_domain(rows), views)]
    DevicePolynomial.degrees(polynomials)
    x = DevicePolynomial.from_polynomial(Polynomial([field.zero(), field.one()]), field)
    R = stark.num_registers
    return [[x] + polynomials[m * R:(m + 1) * R] + [tp.scaled_later(stark.omicron) for tp in polynomials[m * R:(m + 1) * R]] for m in range(K)]


def batch(points):
    return stark.transition_quotients_batch(air, points, zerofier)


def singles(points):
    return [stark._transition_quotients_on_device(air, point, zerofier, None, False) for point in points]


def timed(fn, points, inner):
    sc.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn(points)
    sc.synchronize()
    return (time.perf_counter() - t0) / inner, out


as_data = lambda quotients: [[(q.degree(), q.vec.to_bytes(0, len(q))) for q in member] for member in quotients]
result = {"shape": {"trace_rows": rows, "omicron_domain": stark.omicron_domain_length, "fri_domain": stark.fri_domain_length}, "products_per_point": product_counts(), "K": {}}
print("products per point and constraint: " + "; ".join("%d terms, term by term %d, Horner %d" % (c["terms"], c["term_by_term"], c["horner"]) for c in result["products_per_point"]), flush=True)
for K in [int(k) for k in args.ks.split(",")]:
    points = make_points(K)
    inner = max(1, 16 // K)
    together, alone = [], []
    for rep in range(args.reps + 1):
        tb, qb = timed(batch, points, inner)
        ts, qs = timed(singles, points, inner)
        if rep == 0:
            assert as_data(qb) == as_data(qs), "transition_quotients_batch and the per-member method disagree"
        else:
            together.append(tb / K)
            alone.append(ts / K)
    entry = {"batch_per_member_s": stats(together), "per_member_path_per_member_s": stats(alone), "calls_per_window": inner}
    result["K"][K] = entry
    b, s = entry["batch_per_member_s"], entry["per_member_path_per_member_s"]
    print("K = %-3d batch %8.3f ms/member (%.3f .. %.3f)   K x per-member path %8.3f ms/member (%.3f .. %.3f)   ratio %.2f" %
          (K, b["median"] * 1e3, b["min"] * 1e3, b["max"] * 1e3, s["median"] * 1e3, s["min"] * 1e3, s["max"] * 1e3, s["median"] / b["median"]), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

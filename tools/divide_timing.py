#!/usr/bin/env python3
"""Division with remainder on one MI355X (dev tool): where the device path overtakes the long division, the columns entry against
a loop of the single entry, and what the remainder and the freedom from a coset cost beside sc_coset_divide_dev.

usage: divide_timing.py [--lens 32,64,128,256,512,1024] [--cols 4,16,128] [--col-logs 10,12,16] [--big-log 20] [--runs 3] [--json OUT]

Everything in ONE process; per shape the two sides are compared first, then a warm-up of each side and `runs` + `runs` alternating
repetitions, wall time from an idle stream to an idle stream.  Median with (min .. max).

 1. Polynomial._schoolbook_divide against ntt.fast_divide on host Polynomials (what Polynomial.divide's dispatch chooses between:
    packing, upload, sc_poly_divmod, download and unpacking are all inside the device side) at nb = m = each of --lens and at the
    lopsided (m, nb) = (shortest, longest) and (longest, shortest).  Prints the smallest length from which the device side is at least
    1.5x faster there and at every longer one: Polynomial.FAST_DIV_MIN_LEN (never below 32).
 2. sc_poly_divmod_columns_dev against a loop of sc_poly_divmod_dev over the same resident columns, nb = na / 2.
 3. sc_poly_divmod_dev at (2^big, 2^(big-1)) beside sc_coset_divide_dev of the same degrees on an exact product."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
import starkcore as sc
import synth
from algebra import Field, FieldElement
from univariate import Polynomial
import ntt

ap = argparse.ArgumentParser()
ap.add_argument("--lens", default="32,64,128,256,512,1024")
ap.add_argument("--cols", default="4,16,128")
ap.add_argument("--col-logs", default="10,12,16")
ap.add_argument("--big-log", type=int, default=20)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)
lib, field = sc.lib(), Field.main()
MARGIN = 1.5


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": 1e3 * xs[len(xs) // 2], "min_ms": 1e3 * xs[0], "max_ms": 1e3 * xs[-1]}


def show(st):
    return "%9.3f ms (%.3f .. %.3f)" % (st["median_ms"], st["min_ms"], st["max_ms"])


def timed(call):
    def leg():
        sc.synchronize()
        t0 = time.perf_counter()
        call()
        sc.synchronize()
        return time.perf_counter() - t0
    return leg


def alternate(legs, runs, warmup=1):
    """legs: {name: callable returning seconds}; warm-up calls of each, then `runs` rounds of one call of each in turn"""
    for _ in range(warmup):
        for leg in legs.values():
            leg()
    times = {name: [] for name in legs}
    for _ in range(runs):
        for name, leg in legs.items():
            times[name].append(leg())
    return {name: stats(xs) for name, xs in times.items()}


result = {"runs": args.runs, "margin": MARGIN, "host_divide": {}, "columns": {}, "big": {}}

# ---- 1. the long division against fast_divide ---------------------------------------------------------------------------------------
LENS = [int(x) for x in args.lens.split(",")]
shapes = [(n, n) for n in LENS] + [(LENS[0], LENS[-1]), (LENS[-1], LENS[0])]
for m, nb in shapes:
    na = m + nb - 1
    num = Polynomial([FieldElement(v, field) for v in synth.synth_ints(91, na)])
    den = Polynomial([FieldElement(v, field) for v in synth.synth_ints(92, nb - 1) + [3]])
    want, got = num._schoolbook_divide(den), ntt.fast_divide(num, den)
    assert all([c.value for c in g.coefficients] == [c.value for c in w.coefficients] for g, w in zip(got, want)), "the two divisions disagree"
    entry = alternate({"schoolbook": timed(lambda: num._schoolbook_divide(den)), "device": timed(lambda: ntt.fast_divide(num, den))}, args.runs)
    entry["schoolbook_over_device"] = entry["schoolbook"]["median_ms"] / entry["device"]["median_ms"]
    result["host_divide"]["m=%d nb=%d" % (m, nb)] = entry
    print("divide   m = %4d, nb = %4d:  long division %s   fast_divide %s   x%.2f" %
          (m, nb, show(entry["schoolbook"]), show(entry["device"]), entry["schoolbook_over_device"]), flush=True)
threshold = None
for n in reversed(LENS):
    if result["host_divide"]["m=%d nb=%d" % (n, n)]["schoolbook_over_device"] < MARGIN:
        break
    threshold = n
lopsided = min(result["host_divide"]["m=%d nb=%d" % s]["schoolbook_over_device"] for s in shapes[len(LENS):])
result["threshold"] = {"smallest_length_with_margin": threshold, "lopsided_worst_ratio": lopsided,
                       "fast_div_min_len": max(32, threshold) if threshold is not None else LENS[-1]}
print("device side at least x%.1f faster from nb = m = %s on (lopsided shapes: x%.2f at worst)  ->  FAST_DIV_MIN_LEN = %d" %
      (MARGIN, threshold, lopsided, result["threshold"]["fast_div_min_len"]), flush=True)

# ---- 2. the columns entry against a loop of the single entry ------------------------------------------------------------------------
for logn in [int(x) for x in args.col_logs.split(",")]:
    na = 1 << logn
    nb = na // 2
    m, nr = na - nb + 1, nb - 1
    divisor = sc.DeviceVector.from_bytes(synth.synth_packed(93, nb - 1).tobytes() + (5).to_bytes(16, "little"))
    for cols in [int(x) for x in args.cols.split(",")]:
        src = sc.DeviceVector.from_bytes(synth.synth_packed(94, cols * na).tobytes())
        qa, ra, qb, rb = sc.DeviceVector(cols * m), sc.DeviceVector(cols * nr), sc.DeviceVector(cols * m), sc.DeviceVector(cols * nr)

        def columns():
            sc._check(lib.sc_poly_divmod_columns_dev(src.ptr, na, na, cols, divisor.ptr, nb, qa.ptr, m, ra.ptr, nr, None))

        def loop():
            for c in range(cols):
                sc._check(lib.sc_poly_divmod_dev(src.ptr + 16 * na * c, na, divisor.ptr, nb, qb.ptr + 16 * m * c, rb.ptr + 16 * nr * c, None))
        columns()
        loop()
        sc.synchronize()
        assert qa.to_bytes() == qb.to_bytes() and ra.to_bytes() == rb.to_bytes(), "the column entry and the loop disagree"
        entry = alternate({"loop": timed(loop), "columns": timed(columns)}, args.runs)
        entry["loop_over_columns"] = entry["loop"]["median_ms"] / entry["columns"]["median_ms"]
        result["columns"]["%d x 2^%d" % (cols, logn)] = entry
        print("columns  %3d numerators of 2^%d by 2^%d:  loop of the single entry %s   column entry %s   x%.2f" %
              (cols, logn, logn - 1, show(entry["loop"]), show(entry["columns"]), entry["loop_over_columns"]), flush=True)
        del src, qa, ra, qb, rb

# ---- 3. beside the coset division ---------------------------------------------------------------------------------------------------
na = 1 << args.big_log
nb = na // 2
m, nr = na - nb + 1, nb - 1
root = field.primitive_nth_root(na).value
b_raw = synth.synth_packed(95, nb - 1).tobytes() + (7).to_bytes(16, "little")
q_raw = synth.synth_packed(96, m).tobytes()
a_raw = ctypes.create_string_buffer(16 * na)
sc._check(lib.sc_poly_mul(q_raw, m, b_raw, nb, sc.fe_bytes(root), na, a_raw, na))
a, b = sc.DeviceVector.from_bytes(a_raw.raw), sc.DeviceVector.from_bytes(b_raw)
q1, r1, q2 = sc.DeviceVector(m), sc.DeviceVector(nr), sc.DeviceVector(m)
offset = sc.fe_bytes(field.generator().value)


def divmod_both():
    sc._check(lib.sc_poly_divmod_dev(a.ptr, na, b.ptr, nb, q1.ptr, r1.ptr, None))


def divmod_quotient():
    sc._check(lib.sc_poly_divmod_dev(a.ptr, na, b.ptr, nb, q1.ptr, None, None))


def coset():
    sc._check(lib.sc_coset_divide_dev(a.ptr, na, b.ptr, nb, offset, sc.fe_bytes(root), na, q2.ptr, m, None, None))


divmod_both()
coset()
sc.synchronize()
assert q1.to_bytes() == q2.to_bytes() == q_raw and r1.to_bytes() == bytes(16 * nr), "the divisions disagree on an exact product"
entry = alternate({"divmod": timed(divmod_both), "divmod_quotient_only": timed(divmod_quotient), "coset_divide": timed(coset)}, args.runs)
entry["divmod_over_coset"] = entry["divmod"]["median_ms"] / entry["coset_divide"]["median_ms"]
result["big"]["2^%d by 2^%d" % (args.big_log, args.big_log - 1)] = entry
print("exact product of 2^%d by 2^%d coefficients:  sc_poly_divmod_dev %s   quotient only %s   sc_coset_divide_dev %s   x%.2f" %
      (args.big_log, args.big_log - 1, show(entry["divmod"]), show(entry["divmod_quotient_only"]), show(entry["coset_divide"]), entry["divmod_over_coset"]), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

#!/usr/bin/env python3
"""Products, powers and products of many on one MI355X (dev tool): where ntt.fast_power overtakes the binary method, and what the
columns entry and the product tree buy over loops of single products.

usage: multiply_timing.py [--lens 32,64,128,256,512,1024] [--exponents 2,3,7,255] [--cols 2,3,4,8,16,64] [--col-lens 64,1024]
                          [--col-logs 10,12,16] [--counts 4,16,64,256] [--row-lens 2,33,257] [--runs 3] [--json OUT]

Everything in ONE process; per shape the two sides are compared for equality first, then a warm-up of each side and `runs` + `runs`
alternating repetitions, wall time from an idle stream to an idle stream.  Median with (min .. max).

 1. Polynomial.__xor__ by the binary method (Polynomial._binary_power: ~2 log2(e) products through Polynomial.__mul__, each a host ->
    device -> host round trip above FAST_MUL_MIN_LEN) against ntt.fast_power on host Polynomials of each of --lens coefficients, at
    each of --exponents.  Prints the smallest length from which fast_power is at least 1.5x faster at every exponent measured, there
    and at every longer length: Polynomial.FAST_POW_MIN_LEN (never below 32).
 2. a loop of ntt.fast_multiply against ntt.fast_multiply_columns on host Polynomials (one shared multiplicand), and
 3. a loop of DevicePolynomial.multiply against ntt.multiply_columns_device on resident rows of one matrix (one shared multiplicand
    and one per column).  Prints the smallest number of resident columns from which the columns route is at least 1.5x faster at
    every shape measured, there and at every larger number: ntt.MULTIPLY_COLUMNS_MIN; and what the host-list form gains, whose two
    sides both pack and unpack every coefficient in Python.
 4. the left-to-right product through Polynomial.__mul__ against ntt.fast_product."""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
import starkcore as sc
import synth
from algebra import Field, FieldElement
from univariate import Polynomial
import ntt

ap = argparse.ArgumentParser()
ap.add_argument("--lens", default="32,64,128,256,512,1024")
ap.add_argument("--exponents", default="2,3,7,255")
ap.add_argument("--cols", default="2,3,4,8,16,64")
ap.add_argument("--col-lens", default="64,1024")
ap.add_argument("--col-logs", default="10,12,16")
ap.add_argument("--counts", default="4,16,64,256")
ap.add_argument("--row-lens", default="2,33,257")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)
field = Field.main()
MARGIN = 1.5
ints = lambda text: [int(x) for x in text.split(",")]


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


def poly(seed, n):
    return Polynomial([FieldElement(v, field) for v in synth.synth_ints(seed, n - 1) + [3]])


def values(p):
    return [c.value for c in p.coefficients]


def smallest_with_margin(grid, ratios_at):
    """the smallest entry of the ascending `grid` from which min(ratios_at(entry)) >= MARGIN there and at every larger entry"""
    found = None
    for x in reversed(grid):
        if min(ratios_at(x)) < MARGIN:
            break
        found = x
    return found


result = {"runs": args.runs, "margin": MARGIN, "power": {}, "host_columns": {}, "device_columns": {}, "product": {}}
ntt.MULTIPLY_COLUMNS_MIN = 1                          # measure the columns route at every number of columns

# ---- 1. the binary method against fast_power ------------------------------------------------------------------------------------------
LENS, EXPONENTS = ints(args.lens), ints(args.exponents)
for n in LENS:
    base = poly(71, n)
    for e in EXPONENTS:
        if e * (n - 1) + 1 > 1 << 16:
            continue                                      # (the host side's packing dominates long before; keep the tool quick)
        assert values(base._binary_power(e)) == values(ntt.fast_power(base, e)), "the two powers disagree"
        entry = alternate({"binary": timed(lambda: base._binary_power(e)), "device": timed(lambda: ntt.fast_power(base, e))}, args.runs)
        entry["binary_over_device"] = entry["binary"]["median_ms"] / entry["device"]["median_ms"]
        result["power"]["len=%d e=%d" % (n, e)] = entry
        print("power    len = %4d, e = %3d:  binary method %s   fast_power %s   x%.2f" %
              (n, e, show(entry["binary"]), show(entry["device"]), entry["binary_over_device"]), flush=True)
power_ratios = lambda n: [v["binary_over_device"] for k, v in result["power"].items() if k.startswith("len=%d " % n)]
threshold = smallest_with_margin(LENS, power_ratios)
result["power_threshold"] = {"smallest_length_with_margin": threshold, "fast_pow_min_len": max(32, threshold) if threshold is not None else None}
print("fast_power at least x%.1f faster at every exponent from len = %s on  ->  FAST_POW_MIN_LEN = %s" %
      (MARGIN, threshold, result["power_threshold"]["fast_pow_min_len"]), flush=True)

# ---- 2. a loop of fast_multiply against fast_multiply_columns -------------------------------------------------------------------------
COLS = ints(args.cols)
for n in ints(args.col_lens):
    order = 1 << (2 * n - 2).bit_length()
    root = field.primitive_nth_root(order)
    rhs = poly(72, n)
    for cols in COLS:
        lhs = [poly(73 + c, n) for c in range(cols)]
        loop = lambda: [ntt.fast_multiply(l, rhs, root, order) for l in lhs]
        columns = lambda: ntt.fast_multiply_columns(lhs, rhs)
        assert [values(p) for p in loop()] == [values(p) for p in columns()], "the loop and the columns call disagree"
        entry = alternate({"loop": timed(loop), "columns": timed(columns)}, args.runs)
        entry["loop_over_columns"] = entry["loop"]["median_ms"] / entry["columns"]["median_ms"]
        result["host_columns"]["%d x %d" % (cols, n)] = entry
        print("host     %3d products of %4d by %4d:  loop of fast_multiply %s   fast_multiply_columns %s   x%.2f" %
              (cols, n, n, show(entry["loop"]), show(entry["columns"]), entry["loop_over_columns"]), flush=True)

# ---- 3. a loop of DevicePolynomial.multiply against multiply_columns_device ----------------------------------------------------------
for logn in ints(args.col_logs):
    n = 1 << logn
    for cols in COLS:
        matrix = sc.DeviceVector.from_bytes(synth.synth_packed(74, cols * n).tobytes())
        other = sc.DeviceVector.from_bytes(synth.synth_packed(75, cols * n).tobytes())
        rows = [ntt.DevicePolynomial(sc.DeviceVector.wrap(matrix.ptr + 16 * n * c, n, matrix), field, n) for c in range(cols)]
        others = [ntt.DevicePolynomial(sc.DeviceVector.wrap(other.ptr + 16 * n * c, n, other), field, n) for c in range(cols)]
        for name, rhs in (("shared", others[0]), ("per column", others)):
            loop = lambda: [l.multiply(rhs if name == "shared" else rhs[c]) for c, l in enumerate(rows)]
            columns = lambda: ntt.multiply_columns_device(rows, rhs)
            assert [p.vec.to_bytes() for p in loop()] == [p.vec.to_bytes() for p in columns()], "the loop and the columns call disagree"
            entry = alternate({"loop": timed(loop), "columns": timed(columns)}, args.runs)
            entry["loop_over_columns"] = entry["loop"]["median_ms"] / entry["columns"]["median_ms"]
            result["device_columns"]["%d x 2^%d %s" % (cols, logn, name)] = entry
            print("resident %3d products of 2^%d by 2^%d, %-10s:  loop of multiply %s   multiply_columns_device %s   x%.2f" %
                  (cols, logn, logn, name, show(entry["loop"]), show(entry["columns"]), entry["loop_over_columns"]), flush=True)
        del rows, others, matrix, other
column_ratios = lambda part: lambda cols: [v["loop_over_columns"] for k, v in result[part].items() if k.startswith("%d x" % cols)]
columns_min = smallest_with_margin(COLS, column_ratios("device_columns"))
host_ratios = [v["loop_over_columns"] for v in result["host_columns"].values()]
result["columns_threshold"] = {"multiply_columns_min": columns_min, "host_lists_smallest_with_margin": smallest_with_margin(COLS, column_ratios("host_columns")),
                               "host_lists_worst_ratio": min(host_ratios), "host_lists_best_ratio": max(host_ratios)}
print("multiply_columns_device at least x%.1f faster at every shape from %s columns on  ->  MULTIPLY_COLUMNS_MIN = %s" % (MARGIN, columns_min, columns_min), flush=True)
print("fast_multiply_columns (host lists: packing and unpacking are on both sides) x%.2f at worst, x%.2f at best; at least x%.1f at every length from %s columns on" %
      (min(host_ratios), max(host_ratios), MARGIN, result["columns_threshold"]["host_lists_smallest_with_margin"]), flush=True)

# ---- 4. the left-to-right product against fast_product --------------------------------------------------------------------------------
for n in ints(args.row_lens):
    for count in ints(args.counts):
        if count * (n - 1) + 1 > 1 << 15:
            continue
        members = [poly(76 + j, n) for j in range(count)]

        def left_to_right():
            out = members[0]
            for m in members[1:]:
                out = out * m
            return out
        tree = lambda: ntt.fast_product(members)
        assert values(left_to_right()) == values(tree()), "the two products disagree"
        entry = alternate({"left_to_right": timed(left_to_right), "tree": timed(tree)}, args.runs)
        entry["left_to_right_over_tree"] = entry["left_to_right"]["median_ms"] / entry["tree"]["median_ms"]
        result["product"]["%d x %d" % (count, n)] = entry
        print("product  %3d polynomials of %3d:  left to right %s   fast_product %s   x%.2f" %
              (count, n, show(entry["left_to_right"]), show(entry["tree"]), entry["left_to_right_over_tree"]), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

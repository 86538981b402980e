#!/usr/bin/env python3
"""Multipoint evaluation and interpolation of MANY COLUMNS per call against a loop of the single-column entry, on one MI355X (dev tool).

usage: tree_columns_timing.py [--tree-logs 6,12,16] [--geo-logs 10,16] [--cols 4,16,128] [--runs 3] [--json OUT]

Per shape, in ONE process: the column entry (sc_polytree_evaluate_columns_dev, sc_polytree_interpolate_columns_dev on k arbitrary
points; sc_geodomain_evaluate_columns_dev on a progression of n points) against a loop of the single entry (sc_polytree_evaluate_dev,
sc_polytree_interpolate_dev, sc_geodomain_evaluate_dev) over the same device-resident columns of k (n) coefficients or values each.
The results of both sides are compared first (that call also builds the tree's cached tables, so neither side pays for them
below); then a warm-up of each side and `runs` + `runs` alternating repetitions, wall time from an idle stream to an idle stream
(the single tree entries wait before they return, the column entries only enqueue).  Median with (min .. max)."""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
import starkcore as sc
import synth
from algebra import Field

ap = argparse.ArgumentParser()
ap.add_argument("--tree-logs", default="6,12,16")
ap.add_argument("--geo-logs", default="10,16")
ap.add_argument("--cols", default="4,16,128")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)
lib, field = sc.lib(), Field.main()
COLS = [int(x) for x in args.cols.split(",")]


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


def measure(what, label, columns, loop, a, b, cols):
    columns()
    loop()
    sc.synchronize()
    assert a.to_bytes() == b.to_bytes(), "the column entry and the loop disagree"
    entry = alternate({"loop": timed(loop), "columns": timed(columns)}, args.runs)
    entry["loop_over_columns"] = entry["loop"]["median_ms"] / entry["columns"]["median_ms"]
    result[what]["%d x %s" % (cols, label)] = entry
    print("%-20s %3d columns of %s:  loop of the single entry %s   column entry %s   x%.2f" %
          (what, cols, label, show(entry["loop"]), show(entry["columns"]), entry["loop_over_columns"]), flush=True)


result = {"runs": args.runs, "tree_evaluate": {}, "tree_interpolate": {}, "progression_evaluate": {}}
for logk in [int(x) for x in args.tree_logs.split(",")]:
    k = 1 << logk
    tree = sc.PolyTree(synth.synth_packed(81, k).tobytes())           # arbitrary points
    for cols in COLS:
        src = sc.DeviceVector.from_bytes(synth.synth_packed(82, cols * k).tobytes())
        a, b = sc.DeviceVector(cols * k), sc.DeviceVector(cols * k)

        def evaluate_columns():
            sc._check(lib.sc_polytree_evaluate_columns_dev(tree._h, src.ptr, k, k, cols, tree.points.ptr, a.ptr, k, None))

        def evaluate_loop():
            for c in range(cols):
                sc._check(lib.sc_polytree_evaluate_dev(tree._h, src.ptr + 16 * k * c, k, tree.points.ptr, b.ptr + 16 * k * c, None))

        def interpolate_columns():
            sc._check(lib.sc_polytree_interpolate_columns_dev(tree._h, src.ptr, k, cols, a.ptr, k, None))

        def interpolate_loop():
            for c in range(cols):
                sc._check(lib.sc_polytree_interpolate_dev(tree._h, src.ptr + 16 * k * c, b.ptr + 16 * k * c, None))
        measure("tree_evaluate", "2^%d points" % logk, evaluate_columns, evaluate_loop, a, b, cols)
        measure("tree_interpolate", "2^%d points" % logk, interpolate_columns, interpolate_loop, a, b, cols)
        del src, a, b
    tree.free()

for logn in [int(x) for x in args.geo_logs.split(",")]:
    n = 1 << logn
    domain = sc.GeoDomain(field.generator().value, field.primitive_nth_root(4 * n).value, n)
    for cols in COLS:
        src = sc.DeviceVector.from_bytes(synth.synth_packed(83, cols * n).tobytes())
        a, b = sc.DeviceVector(cols * n), sc.DeviceVector(cols * n)

        def evaluate_columns():
            sc._check(lib.sc_geodomain_evaluate_columns_dev(domain._h, src.ptr, n, n, cols, a.ptr, n, None))

        def evaluate_loop():
            for c in range(cols):
                sc._check(lib.sc_geodomain_evaluate_dev(domain._h, src.ptr + 16 * n * c, n, b.ptr + 16 * n * c, None))
        measure("progression_evaluate", "2^%d points" % logn, evaluate_columns, evaluate_loop, a, b, cols)
        del src, a, b
    domain.free()
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

#!/usr/bin/env python3
"""Polynomial.evaluate_domain / interpolate_domain / zerofier_domain on one MI355X (dev tool): where the device routes overtake the
host methods, where the direct evaluation kernel overtakes the tree route, and what the kernel itself takes on resident operands.

usage: evaluate_timing.py [--points 32,64,...,4096] [--cross-k 16,64,256,1024,4096] [--cross-m 16,64,256,1024,4096,16384]
                          [--res-k 1,4,64,1024] [--res-logs 12,16,20,24] [--res-cols 1,16] [--max-products-log 38] [--runs 3] [--json OUT]

Everything in ONE process; per shape the two sides are compared for equality first, then a warm-up of each side and `runs` + `runs`
alternating repetitions, wall time from an idle stream to an idle stream.  Median with (min .. max).

 1. The host methods' bodies (Polynomial._interpolate_domain_host, _zerofier_domain_host, _evaluate_domain_host) against
    ntt.fast_interpolate_domain, fast_zerofier_domain, fast_evaluate_domain with host lists in and out (packing, upload, the library
    calls, download and unpacking are inside the device side) at each of --points arbitrary points (evaluate_domain: as many
    coefficients as points, and the lopsided (fewest points, most coefficients) and the reverse).  The device side is timed COLD
    (ntt's memo of trees is cleared before the call: the tree, its inverse series and the weights are built in the call, what a first
    call on a new domain pays) and warm (memo hit).  Prints per method the smallest power of two from which the COLD device side is at
    least 1.5x faster there and at every larger shape measured: Polynomial.FAST_INTERPOLATE_MIN_POINTS, FAST_ZEROFIER_MIN_POINTS, FAST_EVAL_DOMAIN_MIN (never below 32).
 2. ntt.fast_evaluate_domain forced direct (sc_poly_eval_points) against forced through the tree, cold (the tree is built in the
    call) and warm (memo hit), for every (m, k) of --cross-m x --cross-k.  Prints the bounds the COLD figures give:
    EVAL_DIRECT_MAX_POINTS = the largest k at which direct wins at every m measured, EVAL_DIRECT_MAX_COEFFS likewise for m.
 3. sc_poly_eval_points_dev on resident operands at --res-k x 2^--res-logs x --res-cols beside its floor: the larger of the bytes
    read over the HBM peak (8.0 TB/s) and m * k * cols products over 8.2e11 products/s; from 32 points on also
    with each form of the kernel forced (sc_set_tuning("eval_points_across_min"), ("eval_across_min_products_log")).  Calls below a millisecond of floor are timed ten
    to a wait.  Shapes of more than 2^--max-products-log products are listed as not measured."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
import starkcore as sc
import synth
from algebra import Field, FieldElement
from univariate import Polynomial
import ntt

ap = argparse.ArgumentParser()
ap.add_argument("--points", default="32,64,128,256,512,1024,2048,4096")
ap.add_argument("--cross-k", default="16,64,256,1024,4096")
ap.add_argument("--cross-m", default="16,64,256,1024,4096,16384")
ap.add_argument("--res-k", default="1,4,64,1024")
ap.add_argument("--res-logs", default="12,16,20,24")
ap.add_argument("--res-cols", default="1,16")
ap.add_argument("--max-products-log", type=int, default=38)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)
lib, field = sc.lib(), Field.main()
MARGIN = 1.5
HBM_PEAK, PRODUCTS_PER_S = 8.0e12, 8.2e11
ints = lambda text: [int(x) for x in text.split(",") if x]
elements = lambda seed, n: [FieldElement(v, field) for v in synth.synth_ints(seed, n)]


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": 1e3 * xs[len(xs) // 2], "min_ms": 1e3 * xs[0], "max_ms": 1e3 * xs[-1]}


def show(st):
    return "%10.3f ms (%.3f .. %.3f)" % (st["median_ms"], st["min_ms"], st["max_ms"])


def timed(call, inner=1):
    def leg():
        sc.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        sc.synchronize()
        return (time.perf_counter() - t0) / inner
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


def same(a, b):
    values = lambda x: [c.value for c in (x.coefficients if isinstance(x, Polynomial) else x)]
    return values(a) == values(b)


def smallest_with_margin(sizes, ratio_of):
    """the smallest of `sizes` (ascending) from which every ratio is at least MARGIN; None if the largest already misses it"""
    found = None
    for n in reversed(sizes):
        if ratio_of(n) < MARGIN:
            break
        found = n
    return found


result = {"runs": args.runs, "margin": MARGIN, "host_methods": {}, "crossover": {}, "resident": {}, "not_measured": []}

# ---- 1. the host methods against their device routes --------------------------------------------------------------------------------
POINTS = ints(args.points)
METHODS = {
    "interpolate_domain": (lambda d, v, p: Polynomial._interpolate_domain_host(d, v), lambda d, v, p: ntt.fast_interpolate_domain(d, v)),
    "zerofier_domain": (lambda d, v, p: Polynomial._zerofier_domain_host(d), lambda d, v, p: ntt.fast_zerofier_domain(d)),
    "evaluate_domain": (lambda d, v, p: p._evaluate_domain_host(d), lambda d, v, p: ntt.fast_evaluate_domain(p, d)),
}


def clear_memo():
    """what a first call on a new domain finds: no tree, no tables, no weights"""
    for tree in ntt._tree_memo.values():
        tree.free()
    ntt._tree_memo.clear()


def host_shape(method, n, m):
    """-> host over device with the domain's tree BUILT IN THE CALL (cold): the figure the thresholds are chosen on"""
    domain, values, poly = elements(51 + n, n), elements(52 + n, n), Polynomial(elements(53 + m, m))
    host, device = METHODS[method]
    assert same(host(domain, values, poly), device(domain, values, poly)), "%s: the two sides disagree" % method

    def cold():
        clear_memo()
        device(domain, values, poly)
    entry = alternate({"host": timed(lambda: host(domain, values, poly)), "device_cold": timed(cold), "device_warm": timed(lambda: device(domain, values, poly))}, args.runs)
    entry["host_over_cold"] = entry["host"]["median_ms"] / entry["device_cold"]["median_ms"]
    entry["host_over_warm"] = entry["host"]["median_ms"] / entry["device_warm"]["median_ms"]
    label = "n=%d" % n if method != "evaluate_domain" else "n=%d m=%d" % (n, m)
    result["host_methods"].setdefault(method, {})[label] = entry
    print("%-18s %-16s host %s   device, cold %s   device, warm %s   host/cold x%.2f  host/warm x%.2f" %
          (method, label, show(entry["host"]), show(entry["device_cold"]), show(entry["device_warm"]), entry["host_over_cold"], entry["host_over_warm"]), flush=True)
    return entry["host_over_cold"]


result["thresholds"] = {}
for method in METHODS:
    ratios = {n: host_shape(method, n, n) for n in POINTS}
    lopsided = None
    if method == "evaluate_domain" and len(POINTS) > 1:
        lopsided = min(host_shape(method, POINTS[0], POINTS[-1]), host_shape(method, POINTS[-1], POINTS[0]))
    least = smallest_with_margin(POINTS, lambda n: ratios[n])
    chosen = max(32, least) if least is not None else 10**9
    result["thresholds"][method] = {"smallest_with_margin": least, "lopsided_worst_ratio": lopsided, "chosen": chosen}
    print("%s: device side, cold, at least x%.1f faster from %s points on%s  ->  threshold %d" %
          (method, MARGIN, least, "" if lopsided is None else " (lopsided shapes: x%.2f at worst)" % lopsided, chosen), flush=True)

# ---- 2. the direct kernel against the tree route, host lists in and out -------------------------------------------------------------
CROSS_K, CROSS_M = ints(args.cross_k), ints(args.cross_m)
committed = (ntt.EVAL_DIRECT_MAX_POINTS, ntt.EVAL_DIRECT_MAX_COEFFS)


def forced(direct, poly, domain, cold=False):
    ntt.EVAL_DIRECT_MAX_POINTS = ntt.EVAL_DIRECT_MAX_COEFFS = 10**9 if direct else 0
    if cold:
        clear_memo()
    try:
        return ntt.fast_evaluate_domain(poly, domain)
    finally:
        ntt.EVAL_DIRECT_MAX_POINTS, ntt.EVAL_DIRECT_MAX_COEFFS = committed


wins = {}
for m in CROSS_M:
    poly = Polynomial(elements(61 + m, m))
    for k in CROSS_K:
        domain = elements(62 + k, k)
        assert same(forced(True, poly, domain), forced(False, poly, domain)), "the two routes disagree"
        entry = alternate({"direct": timed(lambda: forced(True, poly, domain)), "tree_cold": timed(lambda: forced(False, poly, domain, cold=True)),
                           "tree_warm": timed(lambda: forced(False, poly, domain))}, args.runs)
        entry["cold_over_direct"] = entry["tree_cold"]["median_ms"] / entry["direct"]["median_ms"]
        entry["warm_over_direct"] = entry["tree_warm"]["median_ms"] / entry["direct"]["median_ms"]
        wins[(m, k)] = entry["cold_over_direct"] >= 1.0
        result["crossover"]["m=%d k=%d" % (m, k)] = entry
        print("route    m = %5d, k = %4d:  direct %s   tree, cold %s   tree, warm %s   cold/direct x%.2f  warm/direct x%.2f" %
              (m, k, show(entry["direct"]), show(entry["tree_cold"]), show(entry["tree_warm"]), entry["cold_over_direct"], entry["warm_over_direct"]), flush=True)
max_points = max([k for k in CROSS_K if all(wins[(m, kk)] for m in CROSS_M for kk in CROSS_K if kk <= k)], default=0)
max_coeffs = max([m for m in CROSS_M if all(wins[(mm, k)] for k in CROSS_K for mm in CROSS_M if mm <= m)], default=0)
result["crossover_constants"] = {"EVAL_DIRECT_MAX_POINTS": max_points, "EVAL_DIRECT_MAX_COEFFS": max_coeffs}
print("direct at least as fast as the cold tree at every m up to k = %d, and at every k up to m = %d  ->  EVAL_DIRECT_MAX_POINTS = %d, EVAL_DIRECT_MAX_COEFFS = %d" %
      (max_points, max_coeffs, max_points, max_coeffs), flush=True)

# ---- 3. the kernel on resident operands beside its floor ----------------------------------------------------------------------------
RES_K, RES_LOGS, RES_COLS = ints(args.res_k), ints(args.res_logs), ints(args.res_cols)
if RES_K and RES_LOGS and RES_COLS:
    biggest = 1 << max(RES_LOGS)
    base = sc.DeviceVector.from_bytes(synth.synth_packed(71, biggest).tobytes())
    base_ints = synth.synth_ints(71, min(biggest, 1 << 18))
    all_points = synth.synth_ints(72, max(RES_K))
    for logm in RES_LOGS:
        m = 1 << logm
        for cols in RES_COLS:
            matrix = None
            for k in RES_K:
                label = "k=%d m=2^%d cols=%d" % (k, logm, cols)
                if m * k * cols > 1 << args.max_products_log:
                    result["not_measured"].append(label)
                    print("kernel   %-26s not measured (more than 2^%d products)" % (label, args.max_products_log), flush=True)
                    continue
                if matrix is None:                            # every column is the same m coefficients
                    matrix = sc.DeviceVector(cols * m)
                    for c in range(cols):
                        sc._check(lib.sc_memcpy_dev(ctypes.c_void_p(int(matrix.ptr) + 16 * m * c), base.ptr, m, None))
                points, out = sc.DeviceVector.from_ints(all_points[:k]), sc.DeviceVector(cols * k)
                call = lambda: sc._check(lib.sc_poly_eval_points_dev(matrix.ptr, m, m, cols, points.ptr, k, out.ptr, k, None))
                call()
                got = out.to_bytes()
                assert all(got[16 * k * c:16 * k * (c + 1)] == got[:16 * k] for c in range(cols)), "equal columns, different values"
                checked = m * k <= 1 << 18
                if checked:
                    horner = Polynomial([FieldElement(v, field) for v in base_ints[:m]])
                    assert sc.unpack(got[:16 * k]) == [horner.evaluate(FieldElement(x, field)).value for x in all_points[:k]], "not Horner's values"
                floor_bytes = 16.0 * (m * cols + k + k * cols) / HBM_PEAK
                floor_products = float(m) * k * cols / PRODUCTS_PER_S
                floor = max(floor_bytes, floor_products)
                inner = 10 if floor < 1e-3 else 1
                legs = {"call": timed(call, inner)}
                if k >= 32:                                   # each form of the kernel forced, beside the library's own choice
                    def forced_form(least, products_log):
                        sc.set_tuning("eval_points_across_min", least)
                        sc.set_tuning("eval_across_min_products_log", products_log)
                        call()
                        sc.set_tuning("eval_points_across_min", 32)
                        sc.set_tuning("eval_across_min_products_log", 26)
                    legs["coefficients_across"] = timed(lambda: forced_form(1 << 30, 26), inner)
                    legs["points_across"] = timed(lambda: forced_form(1, 0), inner)
                entry = alternate(legs, args.runs)
                entry.update(floor_ms=1e3 * floor, floor_bound="products" if floor_products > floor_bytes else "bytes",
                             over_floor=entry["call"]["median_ms"] / (1e3 * floor), checked_against_horner=checked)
                result["resident"][label] = entry
                print("kernel   %-26s %s   floor %9.4f ms (%s)   x%.1f of the floor%s%s" %
                      (label, show(entry["call"]), entry["floor_ms"], entry["floor_bound"], entry["over_floor"], "" if checked else "   (values: equal columns only)",
                       "" if k < 32 else "   forced coefficients across lanes %s, points across lanes %s" % (show(entry["coefficients_across"]), show(entry["points_across"]))), flush=True)
            del matrix
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

#!/usr/bin/env python3
"""FastStark.prove on a WIDE trace, column batches against the per-register loop, on one MI355X (dev tool).

usage: wide_trace_timing.py [--logs 16,20] [--registers 16] [--checks 40] [--runs 3] [--json OUT]

Per FRI size: workloads.synthetic_wide_instance(log_fri, registers, checks) with a device-resident trace and the operating system's
os.urandom, proved with FastStark.COLUMN_BATCH_MIN = 10**9 (every stage once per register: what the prover did before column
batches) and with the default, in ONE process on one box: warm-up proofs of both kinds, then `runs` + `runs` proofs alternating,
median and range of each.  A third leg alternates with them: the default path with FastStark.COLUMN_DIVIDE and COLUMN_COMBINE both on
("columns"; "batches" runs with both off, whatever the class ships).  A proof of each kind is verified.  Then interpolation alone:
sc_geodomain_interpolate_columns_dev against a loop of sc_geodomain_interpolate_dev at 16 and 128 columns of 2^10 and 2^16 rows, same
form, device time to the end of the stream (the entries only enqueue); and division alone: sc_coset_divide_columns_later_dev against
a loop of sc_coset_divide_later_dev at 16 and 128 columns of order 2^10 and 2^16 (a three-coefficient divisor per column), likewise."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
sys.setrecursionlimit(10000)
import starkcore as sc
import synth
import workloads
from algebra import Field
from fast_stark import DeviceTrace, FastStark, os_urandom_is_genuine

ap = argparse.ArgumentParser()
ap.add_argument("--logs", default="16,20")
ap.add_argument("--registers", type=int, default=16)
ap.add_argument("--checks", type=int, default=40)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)
assert os_urandom_is_genuine()
DEFAULT_MIN, LOOP = FastStark.COLUMN_BATCH_MIN, 10 ** 9


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": 1e3 * xs[len(xs) // 2], "min_ms": 1e3 * xs[0], "max_ms": 1e3 * xs[-1]}


def show(st):
    return "%9.3f ms (%.3f .. %.3f)" % (st["median_ms"], st["min_ms"], st["max_ms"])


def alternate(legs, runs, warmup=2):
    """legs: {name: callable returning seconds}; warm-up calls of each, then `runs` rounds of one call of each in turn"""
    for _ in range(warmup):
        for leg in legs.values():
            leg()
    times = {name: [] for name in legs}
    for _ in range(runs):
        for name, leg in legs.items():
            times[name].append(leg())
    return {name: stats(xs) for name, xs in times.items()}


result = {"registers": args.registers, "colinearity_checks": args.checks, "column_batch_min": DEFAULT_MIN, "prove": {}, "interpolate": {}, "divide": {}}
for log_fri in [int(x) for x in args.logs.split(",")]:
    field, T, _, packed, air, boundary = workloads.synthetic_wide_instance(log_fri, args.registers, args.checks)
    stark = FastStark(field, 4, args.checks, 2 * args.checks, args.registers, T)
    assert stark.fri_domain_length == 1 << log_fri
    trace = DeviceTrace.from_packed(packed, field)
    tz, tz_codeword, tz_root = stark.preprocess(device_resident=True)
    proofs = {}

    def prove(name, batch_min, columns=False):
        shipped = FastStark.COLUMN_DIVIDE, FastStark.COLUMN_COMBINE
        FastStark.COLUMN_BATCH_MIN, FastStark.COLUMN_DIVIDE, FastStark.COLUMN_COMBINE = batch_min, columns, columns
        sc.synchronize()
        t0 = time.perf_counter()
        proofs[name] = stark.prove(trace, air, boundary, tz, tz_codeword)
        sc.synchronize()
        FastStark.COLUMN_BATCH_MIN, (FastStark.COLUMN_DIVIDE, FastStark.COLUMN_COMBINE) = DEFAULT_MIN, shipped
        return time.perf_counter() - t0
    entry = alternate({"loop": lambda: prove("loop", LOOP), "batches": lambda: prove("batches", DEFAULT_MIN),
                       "columns": lambda: prove("columns", DEFAULT_MIN, True)}, args.runs)
    entry["verify_accepts"] = {name: bool(stark.verify(proof, air, boundary, tz_root)) for name, proof in proofs.items()}
    entry["trace_rows"], entry["proof_bytes"] = T + 4 * args.checks, len(proofs["batches"])
    result["prove"][log_fri] = entry
    print("FastStark.prove, %d registers, FRI 2^%d (trace 2^%d rows):  per-register loop %s   column batches %s   + column divide and combine %s   verify %s" %
          (args.registers, log_fri, log_fri - 4, show(entry["loop"]), show(entry["batches"]), show(entry["columns"]), entry["verify_accepts"]), flush=True)
    del trace, tz, tz_codeword, stark, proofs

lib, field = sc.lib(), Field.main()
for log_rows in (10, 16):
    n = 1 << log_rows
    domain = sc.GeoDomain(1, field.primitive_nth_root(4 * n).value, n)
    for cols in (16, 128):
        values = sc.DeviceVector.from_bytes(synth.synth_packed(77, cols * n).tobytes())
        a, b = sc.DeviceVector(cols * n), sc.DeviceVector(cols * n)

        def columns():
            sc.synchronize()
            t0 = time.perf_counter()
            sc._check(lib.sc_geodomain_interpolate_columns_dev(domain._h, values.ptr, n, cols, a.ptr, n, None))
            sc.synchronize()
            return time.perf_counter() - t0

        def loop():
            sc.synchronize()
            t0 = time.perf_counter()
            for c in range(cols):
                sc._check(lib.sc_geodomain_interpolate_dev(domain._h, values.ptr + 16 * n * c, b.ptr + 16 * n * c, None))
            sc.synchronize()
            return time.perf_counter() - t0
        entry = alternate({"loop": loop, "columns": columns}, args.runs)
        assert a.to_bytes() == b.to_bytes(), "the column entry and the loop disagree"
        result["interpolate"]["%d x 2^%d" % (cols, log_rows)] = entry
        print("interpolation, %3d columns of 2^%d rows:  loop of the single entry %s   column entry %s" % (cols, log_rows, show(entry["loop"]), show(entry["columns"])), flush=True)
    domain.free()

G = field.generator().value
for log_order in (10, 16):
    order = 1 << log_order
    root = field.primitive_nth_root(order).value
    na, nb = order // 2, 3
    for cols in (16, 128):
        numerators = sc.DeviceVector.from_bytes(synth.synth_packed(78, cols * na).tobytes())
        divisors = sc.DeviceVector.from_bytes(synth.synth_packed(79, cols * nb).tobytes())
        n_out = na - nb + 1
        a, b = sc.DeviceVector(cols * n_out), sc.DeviceVector(cols * n_out)
        lengths = (ctypes.c_uint64 * cols)(*([n_out] * cols))
        words = (ctypes.c_int64 * 8)()

        def columns():
            sc.synchronize()
            t0 = time.perf_counter()
            h = ctypes.c_void_p()
            sc._check(lib.sc_coset_divide_columns_later_dev(numerators.ptr, na, na, divisors.ptr, nb, nb, cols, sc.fe_bytes(G), sc.fe_bytes(root), order, a.ptr, lengths, n_out,
                                                            ctypes.byref(h), None))
            sc.synchronize()
            dt = time.perf_counter() - t0
            sc._check(lib.sc_later_wait(h, words))
            return dt

        def loop():
            sc.synchronize()
            t0 = time.perf_counter()
            handles = []
            for c in range(cols):
                h = ctypes.c_void_p()
                sc._check(lib.sc_coset_divide_later_dev(numerators.ptr + 16 * na * c, na, divisors.ptr + 16 * nb * c, nb, sc.fe_bytes(G), sc.fe_bytes(root), order,
                                                        b.ptr + 16 * n_out * c, n_out, ctypes.byref(h), None))
                handles.append(h)
            sc.synchronize()
            dt = time.perf_counter() - t0
            for h in handles:
                sc._check(lib.sc_later_wait(h, words))
            return dt
        entry = alternate({"loop": loop, "columns": columns}, args.runs)
        assert a.to_bytes() == b.to_bytes(), "the column entry and the loop disagree"
        result["divide"]["%d x 2^%d" % (cols, log_order)] = entry
        print("coset division, %3d columns of order 2^%d:  loop of the single entry %s   column entry %s" % (cols, log_order, show(entry["loop"]), show(entry["columns"])), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

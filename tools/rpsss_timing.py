#!/usr/bin/env python3
"""Rescue-Prime kernels and FastRPSSS on one MI355X (dev tool).

usage: rpsss_timing.py [--reps 7] [--logs 10,12,...,22] [--verify-only] [--json OUT]

(a) RescuePrime.hash_device at 2^10 ... 2^22 inputs: hashes/s and modular products/s (7 994 per hash, csrc/rescue_prime.cuh), the
    host clock around one launch + sc_synchronize, after a warm-up launch;
(b) one input's trace: trace_device (launch, wait) against the host mirror RescuePrime.trace;
(c) FastRPSSS.sign (trace from the kernel, and from the host mirror);
(d) FastRPSSS.verify, and verify_batch at K = 1, 16 and 64, in ms per signature, with the AIR evaluation (the transition constraints at
    the opened points) timed inside the walk -- with the structured evaluator, and with the generic term-by-term one (what plain
    MPolynomial constraints pay) for comparison.  Every verify_batch shape runs in two legs that alternate inside each repetition:
    FastStark.COMBINATION_ON_DEVICE on (the opened points as rows of sc_stark_combination_batch; `combination` = the device call and
    the rows' packing) and off (the host loop, the code as it was before the rows).
--verify-only skips (a) to (c).  Median and range over the repetitions."""
import argparse, json, os, random, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
sys.setrecursionlimit(10000)
import starkcore as sc
import fast_rpsss
import fri
import rescue_prime
from fast_stark import FastStark
from multivariate import MPolynomial
from algebra import FieldElement

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--logs", default="10,12,14,16,18,20,22")
ap.add_argument("--json", default=None)
ap.add_argument("--verify-only", action="store_true")
args = ap.parse_args()
sc.init(0)
PRODUCTS_PER_HASH = 7994


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def clock(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return stats(out)


result = {"hash_device": {}}
rp = rescue_prime.RescuePrime()
if not args.verify_only:
    rng = random.Random(1)
    for log in [int(v) for v in args.logs.split(",")]:
        n = 1 << log
        vec = sc.DeviceVector.from_bytes(rng.randbytes(16 * n))
        out = sc.DeviceVector(n)
        run = lambda: (sc._check(sc.lib().sc_rescue_prime_hash_dev(vec.ptr, n, rp._params, rp.N, out.ptr, None)), sc.synchronize())
        run()
        s = clock(run, args.reps)
        med = s["median"]
        result["hash_device"][n] = {"seconds": s, "hashes_per_s": n / med, "products_per_s": n * PRODUCTS_PER_HASH / med}
        print("hash_device 2^%-2d  %9.3f ms   %.3e hashes/s   %.3e products/s" % (log, med * 1e3, n / med, n * PRODUCTS_PER_HASH / med), flush=True)
        del vec, out

    x = FieldElement(123456789, rp.field)
    rp.trace_device(x)
    dev = clock(lambda: (rp.trace_device(x), sc.synchronize()), args.reps * 3)
    host = clock(lambda: rp.trace(x), args.reps * 3)
    hhash = clock(lambda: rp.hash(x), args.reps * 3)
    result["trace_one"] = {"device": dev, "host": host, "host_hash": hhash}
    print("one trace: device %.3f ms, host mirror %.3f ms (host hash %.3f ms)" % (dev["median"] * 1e3, host["median"] * 1e3, hhash["median"] * 1e3), flush=True)

rpsss = fast_rpsss.FastRPSSS()
sk, pk = rpsss.keygen()
doc = b"timing document"
if not args.verify_only:
    rpsss.sign(sk, doc)
    sign_dev = clock(lambda: rpsss.sign(sk, doc), args.reps)
    fast_rpsss.FastRPSSS.SIGN_ON_DEVICE = False
    sign_host = clock(lambda: rpsss.sign(sk, doc), args.reps)
    fast_rpsss.FastRPSSS.SIGN_ON_DEVICE = True
    result["sign"] = {"device_trace": sign_dev, "host_trace": sign_host}
    print("sign: %.2f ms (kernel trace), %.2f ms (host-mirror trace)" % (sign_dev["median"] * 1e3, sign_host["median"] * 1e3), flush=True)

KS = (1, 16, 64)
K = max(KS)
sigs = [rpsss.sign(sk, doc) for _ in range(K)]
air = {"t": 0.0, "combination": 0.0}
structured = rescue_prime.RescueConstraint.evaluator


def timed(fn, key):
    def wrapper(*a, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*a, **kw)
        finally:
            air[key] += time.perf_counter() - t0
    return wrapper


def timed_evaluator(make):
    def evaluator(self):
        return timed(make(self), "t")
    return evaluator


for method in ("verdicts", "add", "member"):            # the device call and the rows' packing
    setattr(fri.CombinationRows, method, timed(getattr(fri.CombinationRows, method), "combination"))


def once(fn, per):
    air["t"] = air["combination"] = 0.0
    t0 = time.perf_counter()
    verdicts = fn()
    total = time.perf_counter() - t0
    assert all(verdicts)
    return total / per, air["t"] / per, air["combination"] / per


def report(label, samples):
    totals, airs, combinations = (stats([v[i] for v in samples]) for i in range(3))
    print("%-46s %8.3f ms/signature  (AIR %6.3f ms, combination rows %6.3f ms)" % (label, totals["median"] * 1e3, airs["median"] * 1e3, combinations["median"] * 1e3), flush=True)
    return {"ms_per_signature": {k: v * 1e3 for k, v in totals.items()}, "air_ms": {k: v * 1e3 for k, v in airs.items()},
            "combination_ms": {k: v * 1e3 for k, v in combinations.items()}}


shapes = [("verify_batch_%d" % k, (lambda k=k: [v for lo in range(0, max(k, 4), k) for v in rpsss.verify_batch([pk] * k, [doc] * k, sigs[lo:lo + k])]), max(k, 4)) for k in KS]
for name, make in (("structured", structured), ("generic", MPolynomial.evaluator)):
    rescue_prime.RescueConstraint.evaluator = timed_evaluator(make)
    samples = {}
    for on in (True, False):                             # warm-up of both legs
        FastStark.COMBINATION_ON_DEVICE = on
        rpsss.verify_batch([pk] * 2, [doc] * 2, sigs[:2])
    for _ in range(args.reps):
        samples.setdefault("verify", []).append(once(lambda: [rpsss.verify(pk, doc, s) for s in sigs[:4]], 4))
        for key, fn, per in shapes:
            for suffix, on in (("", True), ("_host_loop", False)):       # the two legs alternate
                FastStark.COMBINATION_ON_DEVICE = on
                samples.setdefault(key + suffix, []).append(once(fn, per))
    FastStark.COMBINATION_ON_DEVICE = True
    result["verify_" + name] = {key: report("%s (%s AIR)" % (key, name), v) for key, v in samples.items()}
rescue_prime.RescueConstraint.evaluator = structured
result["combination_device_min_rows"] = FastStark.COMBINATION_DEVICE_MIN_ROWS

if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

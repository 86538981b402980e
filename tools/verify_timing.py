#!/usr/bin/env python3
"""FastStark.verify against FastStark.verify_batch, per proof, at K = 1, 16 and 64 (dev tool).

usage: verify_timing.py [--sizes 16,20,24] [--rpsss] [--rpsss-generic] [--ks 1,16] [--reps 5] [--json OUT]

Synthetic AIR (workloads.synthetic_stark_instance, s = 40) at FRI 2^n for each n of --sizes, and --rpsss: the Rescue-Prime AIR at the
reference's FastRPSSS parameters (expansion factor 4, s = 64, FRI 4096).  Per size: 16 proofs of one statement (seeded randomizers),
then --reps repetitions of (a) verify over every proof, (b) verify_batch([proof]) over every proof, (c) verify_batch of all 16; the
phase split of (b) and (c): unpickling (pickle.loads of the proofs, timed on its own), host parse (the walk over the proofs, the
host checks included, minus unpickling), of which air_eval (the transition constraints evaluated at the opened points, timed
inside the walk), device calls (sc_merkle_verify_batch + sc_fri_colinearity_batch) and reduce (row packing and the per-proof
reduction).  Median and range over the repetitions.
--ks: the batch sizes (max(ks) proofs are made; K proofs go through max(ks) / K calls).  Every batch size is measured in two legs that
alternate inside each repetition: FastStark.COMBINATION_ON_DEVICE on (the combination at the opened points as rows of
sc_stark_combination_batch: phase `combination` = the device call, `combination_pack` = the rows' packing) and off ("..._host_ms":
the host loop, the code as it was before the rows).  --rpsss-generic: the FastRPSSS instance verified with plain MPolynomial
constraints (no hand-written evaluator), what an AIR a user brings pays."""
import argparse, json, os, pickle, random, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd")); sys.path.insert(0, os.path.join(REPO, "tests"))
sys.setrecursionlimit(10000)
import starkcore as sc
import fast_stark
import fri
import multivariate
import workloads
from fast_stark import DeviceTrace, FastStark
from algebra import Field

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="16,20,24")
ap.add_argument("--rpsss", action="store_true")
ap.add_argument("--rpsss-generic", action="store_true")
ap.add_argument("--ks", default="1,16")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)
KS = sorted({int(v) for v in args.ks.split(",") if v})
K = max(KS)

# phase clocks: the device calls and BatchChecks.run are wrapped
clock = {"device": 0.0, "run": 0.0, "air": 0.0, "combination": 0.0, "pack": 0.0}


def timed(fn, key):
    def wrapper(*a, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*a, **kw)
        finally:
            clock[key] += time.perf_counter() - t0
    return wrapper


sc.merkle_verify_batch = timed(sc.merkle_verify_batch, "device")
sc.colinearity_batch = timed(sc.colinearity_batch, "device")
sc.combination_batch = timed(sc.combination_batch, "combination")
fri.CombinationRows.verdicts = timed(fri.CombinationRows.verdicts, "pack")          # (includes the device call: taken off below)
fri.CombinationRows.add = timed(fri.CombinationRows.add, "pack")
fri.CombinationRows.member = timed(fri.CombinationRows.member, "pack")
fri.BatchChecks.run = timed(fri.BatchChecks.run, "run")
_evaluator = multivariate.MPolynomial.evaluator
multivariate.MPolynomial.evaluator = lambda self: timed(_evaluator(self), "air")


def instance(name):
    rng = random.Random(7)
    fast_stark.os.urandom = lambda k: bytes(rng.getrandbits(8) for _ in range(k))
    if name in ("rpsss", "rpsss-generic"):
        from workload_rescue_prime import RescuePrime
        field, rp = Field.main(), RescuePrime()
        stark = FastStark(field, 4, 64, 128, rp.m, rp.N + 1, transition_constraints_degree=3)
        tz, tzc, tzr = stark.preprocess()
        inp = field.sample(b"0xdeadbeef")
        air, boundary = rp.transition_constraints(stark.omicron), rp.boundary_constraints(rp.hash(inp))
        trace = rp.trace(inp)
    else:
        s = 40
        field, T, packed, air, boundary = workloads.synthetic_stark_instance(name, s)
        stark = FastStark(field, 4, s, 2 * s, 2, T)
        tz, tzc, tzr = stark.preprocess(device_resident=True)
        trace = DeviceTrace.from_packed(packed, field)
    proofs = [stark.prove(trace, air, boundary, tz, tzc) for _ in range(K)]
    if name == "rpsss-generic":
        air = [multivariate.MPolynomial(dict(a.dictionary)) for a in air]
    return stark, air, boundary, tzr, proofs


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def batch_phases(stark, air, boundary, tzr, proofs):
    """one verify_batch call over `proofs`: total, and the phase split (ms per proof)"""
    n = len(proofs)
    t0 = time.perf_counter()
    for p in proofs:
        pickle.loads(p)
    unpickle = time.perf_counter() - t0
    for key in clock:
        clock[key] = 0.0
    t0 = time.perf_counter()
    verdicts = stark.verify_batch(proofs, air, [boundary] * n, tzr)
    total = time.perf_counter() - t0
    assert verdicts == [True] * n, verdicts
    pack = clock["pack"] - clock["combination"]
    return {"total": 1e3 * total / n, "unpickle": 1e3 * unpickle / n, "host_parse": 1e3 * (total - clock["run"] - unpickle) / n,
            "air_eval": 1e3 * clock["air"] / n, "device": 1e3 * clock["device"] / n, "combination": 1e3 * clock["combination"] / n,
            "combination_pack": 1e3 * pack / n, "reduce": 1e3 * (clock["run"] - clock["device"] - clock["combination"]) / n}


def batches_of(k, stark, air, boundary, tzr, proofs):
    """all proofs in calls of k: the phases per proof"""
    per = [batch_phases(stark, air, boundary, tzr, proofs[lo:lo + k]) for lo in range(0, len(proofs), k)]
    return {key: sum(r[key] for r in per) / len(per) for key in per[0]}


results = []
names = [int(v) for v in args.sizes.split(",") if v] + (["rpsss"] if args.rpsss else []) + (["rpsss-generic"] if args.rpsss_generic else [])
LEGS = (("", True), ("_host", False))                # (suffix of the record's key, COMBINATION_ON_DEVICE)
for name in names:
    stark, air, boundary, tzr, proofs = instance(name)
    assert stark.verify(proofs[0], air, boundary, tzr) is True
    for _, on in LEGS:
        FastStark.COMBINATION_ON_DEVICE = on
        stark.verify_batch(proofs[:2], air, [boundary] * 2, tzr)        # warm-up (staging buffers, code objects)
    host, legs = [], {}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for p in proofs:
            assert stark.verify(p, air, boundary, tzr) is True
        host.append(1e3 * (time.perf_counter() - t0) / K)
        for k in KS:
            for suffix, on in LEGS:                  # the two legs alternate
                FastStark.COMBINATION_ON_DEVICE = on
                for key, v in batches_of(k, stark, air, boundary, tzr, proofs).items():
                    legs.setdefault("verify_batch_k%d%s_ms" % (k, suffix), {}).setdefault(key, []).append(v)
    FastStark.COMBINATION_ON_DEVICE = True
    label = {"rpsss": "FastRPSSS (Rescue-Prime, FRI 4096, s = 64)", "rpsss-generic": "FastRPSSS, generic MPolynomial constraints (FRI 4096, s = 64)"}.get(
        name, "synthetic AIR, FRI 2^%s, s = 40" % name)
    rec = {"config": label, "proof_bytes": len(proofs[0]), "reps": args.reps, "opened_points_per_proof": 2 * stark.num_colinearity_checks,
           "combination_device_min_rows": FastStark.COMBINATION_DEVICE_MIN_ROWS, "verify_ms": stats(host)}
    rec.update({leg: {k: stats(v) for k, v in phases.items()} for leg, phases in legs.items()})
    results.append(rec)
    h = rec["verify_ms"]["median"]
    print("%s: verify %.2f ms/proof" % (label, h))
    for k in KS:
        on, off = rec["verify_batch_k%d_ms" % k]["total"]["median"], rec["verify_batch_k%d_host_ms" % k]["total"]["median"]
        print("  K=%d: rows on the device %.3f ms/proof (%.2fx of verify), host loop %.3f ms/proof; device / host %.3f" % (k, on, h / on, off, on / off))
    for leg in sorted(legs):
        print("  %s: " % leg + ", ".join("%s %.3f [%.3f, %.3f]" % (p, v["median"], v["min"], v["max"]) for p, v in rec[leg].items()))
    sys.stdout.flush()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)

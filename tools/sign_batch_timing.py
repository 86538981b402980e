#!/usr/bin/env python3
"""FastRPSSS.sign_batch against K calls of FastRPSSS.sign, on one MI355X (dev tool).

usage: sign_batch_timing.py [--reps 5] [--ks 1,4,16,64] [--json OUT]

Per K: K secret keys and K distinct documents; one repetition signs them once through sign_batch and once through K calls of sign,
the two alternating so that both see the same machine, both under the same seeded os.urandom (random.Random, one getrandbits call per
draw), and the signatures are asserted equal.  The seeded stand-in costs both sides the same bytes; it
is what makes the comparison checkable.  Both calls end with the signatures on the host, so the host clock around a call is the
time to the finished signatures.  The first repetition of every K is a warm-up and is dropped.  Median and range, in ms per
signature, and their ratio; then one more sign_batch with FastStark.phase_log on (the device is waited for after every phase, so
these do not add up to the timed call): seconds per phase, summed over the chunks."""
import argparse, json, os, random, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
sys.setrecursionlimit(10000)
import starkcore as sc
import fast_rpsss
from algebra import FieldElement

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ks", default="1,4,16,64")
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)

rpsss = fast_rpsss.FastRPSSS()
stark = rpsss.stark
print("shape: %d trace rows, omicron domain 2^%d, FRI domain 2^%d, %d colinearity checks, %d FRI rounds" %
      (stark.randomized_trace_length, stark.omicron_domain_length.bit_length() - 1, stark.fri_domain_length.bit_length() - 1,
       stark.num_colinearity_checks, stark.fri.num_rounds()), flush=True)
genuine = os.urandom


def seeded(seed):
    rng = random.Random(seed)
    os.urandom = lambda k: rng.getrandbits(8 * k).to_bytes(k, "little") if k else b""


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def timed(fn, seed):
    seeded(seed)
    try:
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out
    finally:
        os.urandom = genuine


ks = [int(k) for k in args.ks.split(",")]
keys = [FieldElement(random.Random(5).randrange(rpsss.field.p) + k, rpsss.field) for k in range(max(ks))]
result = {"shape": {"trace_rows": stark.randomized_trace_length, "omicron_domain_length": stark.omicron_domain_length,
                    "fri_domain_length": stark.fri_domain_length, "num_colinearity_checks": stark.num_colinearity_checks}, "K": {}}
for K in ks:
    sks = keys[:K]
    batch, singles = [], []
    for rep in range(args.reps + 1):
        documents = [b"document %d of repetition %d" % (m, rep) for m in range(K)]
        tb, together = timed(lambda: rpsss.sign_batch(sks, documents), 1000 + rep)
        ts, one_by_one = timed(lambda: [rpsss.sign(sk, document) for sk, document in zip(sks, documents)], 1000 + rep)
        assert together == one_by_one, "sign_batch and sign disagree"
        if rep:
            batch.append(tb / K)
            singles.append(ts / K)
    stark.phase_log = []
    try:
        timed(lambda: rpsss.sign_batch(sks, documents), 1000)
        phases = {}
        for phase, seconds in stark.phase_log:
            phases[phase] = phases.get(phase, 0.0) + seconds
    finally:
        stark.phase_log = None
    b, s = stats(batch), stats(singles)
    result["K"][K] = {"sign_batch_per_signature_s": b, "sign_per_signature_s": s, "ratio_sign_over_sign_batch": s["median"] / b["median"],
                      "sign_batch_phases_s": phases}
    print("K = %-3d sign_batch %8.2f ms/signature (%.2f .. %.2f)   K x sign %8.2f ms/signature (%.2f .. %.2f)   K x sign / sign_batch = %.2f" %
          (K, b["median"] * 1e3, b["min"] * 1e3, b["max"] * 1e3, s["median"] * 1e3, s["min"] * 1e3, s["max"] * 1e3, s["median"] / b["median"]), flush=True)
    for phase, seconds in phases.items():
        print("          %-72s %8.2f ms/signature" % (phase, seconds * 1e3 / K), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

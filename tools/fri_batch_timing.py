#!/usr/bin/env python3
"""Fri.prove_batch against K calls of Fri.prove at the signature scheme's FRI shape, on one MI355X (dev tool).

usage: fri_batch_timing.py [--reps 9] [--ks 1,4,16,64,256] [--four-lane 256,0,1048576] [--json OUT]

The shape (domain length, expansion factor, colinearity tests) is read from FastRPSSS().stark.fri.  Per K: K device-resident codewords
of the shape's rate, K SignatureProofStreams with distinct documents (the route FastRPSSS.sign takes); one repetition proves them
once through prove_batch and once through K calls of prove, on fresh codeword wrappers and fresh streams, the two alternating so that
both see the same machine.  Both end with the proof on the host, so the host clock around a call is the time to the finished proof.
The first repetition of every K is a warm-up and is dropped.  Median and range, in ms per member; then the same batch under each
value of the tuning key "forest_four_lane_wgs" (one or four lanes per BLAKE2b compression on the forest's narrow levels), and the
forest counters, from which the launches per round follow (csrc/merkle_forest.cuh: ceil(log2 n / 8) per forest, one query launch)."""
import argparse, json, os, random, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
sys.setrecursionlimit(10000)
import starkcore as sc
import fast_rpsss
from algebra import FieldElement
from ntt import fast_coset_evaluate_device
from starkcore import DeviceCodeword
from univariate import Polynomial

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--ks", default="1,4,16,64,256")
ap.add_argument("--four-lane", default="256,0,1048576")
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)

fri = fast_rpsss.FastRPSSS().stark.fri
field, N = fri.field, fri.domain_length
rounds = fri.num_rounds()
print("shape: N = 2^%d, expansion factor %d, %d colinearity tests, %d rounds" % (N.bit_length() - 1, fri.expansion_factor, fri.num_colinearity_tests, rounds), flush=True)
rng = random.Random(7)


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def make_codeword():
    coeffs = [FieldElement(rng.randrange(field.p), field) for _ in range(N // fri.expansion_factor)]
    return fast_coset_evaluate_device(Polynomial(coeffs), fri.offset, fri.omega, N)


def streams(K, rep):
    return [fast_rpsss.SignatureProofStream(b"document %d of repetition %d" % (m, rep)) for m in range(K)]


def wrappers(codewords):
    return [DeviceCodeword(cw.vec, field) for cw in codewords]       # fresh object caches, no tree; the device data is shared


def time_batch(codewords, rep):
    cws, sts = wrappers(codewords), streams(len(codewords), rep)
    t0 = time.perf_counter()
    fri.prove_batch(cws, sts)
    return time.perf_counter() - t0, sts


def time_singles(codewords, rep):
    cws, sts = wrappers(codewords), streams(len(codewords), rep)
    t0 = time.perf_counter()
    for cw, st in zip(cws, sts):
        fri.prove(cw, st)
    return time.perf_counter() - t0, sts


result = {"shape": {"N": N, "expansion_factor": fri.expansion_factor, "num_colinearity_tests": fri.num_colinearity_tests, "rounds": rounds}, "K": {}}
pool = [make_codeword() for _ in range(max(int(k) for k in args.ks.split(",")))]
for K in [int(k) for k in args.ks.split(",")]:
    codewords = pool[:K]
    batch, singles = [], []
    for rep in range(args.reps + 1):
        tb, sb = time_batch(codewords, rep)
        ts, ss = time_singles(codewords, rep)
        assert [s.serialize() for s in sb] == [s.serialize() for s in ss], "prove_batch and prove disagree"
        if rep:
            batch.append(tb / K)
            singles.append(ts / K)
    before = sc.forest_stats()
    time_batch(codewords, 0)
    after = sc.forest_stats()
    entry = {"prove_batch_per_member_s": stats(batch), "prove_per_member_s": stats(singles),
             "forests_per_call": after[0] - before[0], "trees_per_call": after[1] - before[1]}
    variants = {}
    for v in [int(x) for x in args.four_lane.split(",")]:
        sc.set_tuning("forest_four_lane_wgs", v)
        time_batch(codewords, 0)
        variants[v] = stats([time_batch(codewords, rep)[0] / K for rep in range(1, args.reps + 1)])
    sc.set_tuning("forest_four_lane_wgs", 256)
    entry["forest_four_lane_wgs"] = variants
    result["K"][K] = entry
    b, s = entry["prove_batch_per_member_s"], entry["prove_per_member_s"]
    print("K = %-4d prove_batch %8.3f ms/member (%.3f .. %.3f)   K x prove %8.3f ms/member (%.3f .. %.3f)   forests per call %d" %
          (K, b["median"] * 1e3, b["min"] * 1e3, b["max"] * 1e3, s["median"] * 1e3, s["min"] * 1e3, s["max"] * 1e3, entry["forests_per_call"]), flush=True)
    print("          forest_four_lane_wgs: " + "   ".join("%d: %.3f ms (%.3f .. %.3f)" % (v, st["median"] * 1e3, st["min"] * 1e3, st["max"] * 1e3) for v, st in variants.items()), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

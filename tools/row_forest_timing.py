#!/usr/bin/env python3
"""Row forests against row trees, and row-committed sign_batch against K calls of sign, on one MI355X (dev tool).

usage: row_forest_timing.py [--reps 5] [--ks 1,4,16,64] [--inner 20] [--json OUT] [--txt OUT]

One process; per measurement a warm-up repetition that is dropped, then --reps repetitions in which the two legs alternate so that
both see the same machine; medians and ranges.  Every timed window ends with its result on the host (a root or a signature: the
device has been waited for), so the host clock around it is the time to the finished result.

(a) tree only: starkcore.RowForest.build + .roots over K trees against K x starkcore.RowTree.build (root fetched), at the signature's
    shape (w = 3, N = 2^12; K = --ks) and at w = 17, N = 2^16, K = 4; the roots are asserted equal first; a window is --inner builds.
(b) signatures: FastRPSSS(row_commitments=True).sign_batch against K sequential `sign` calls of the same scheme (what sign_batch did
    for a row-committed scheme before the batch was served by a row forest), both under the same seeded os.urandom (random.Random; the
    stand-in costs both legs the same bytes), the signatures asserted equal; then one more sign_batch with FastStark.phase_log on (the
    device is waited for after every phase, so the phases do not add up to the timed call).
(c) option off: FastRPSSS().sign_batch under the same seeds, for its time and signature size beside (b).
Without a GPU the tool exits with an error: nothing here can be measured on a CPU."""
import argparse, json, os, random, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
sys.setrecursionlimit(10000)
import starkcore as sc

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ks", default="1,4,16,64")
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--json", default=None)
ap.add_argument("--txt", default=None)
args = ap.parse_args()
if sc.device_count() == 0:
    sys.exit("row_forest_timing.py: no GPU visible; nothing is measured without one")
sc.init(0)
import fast_rpsss
from algebra import FieldElement

ks = [int(k) for k in args.ks.split(",")]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def alternate(legs, reps):
    """legs: {name: fn() -> seconds}; one dropped warm-up, then `reps` repetitions, the legs in turn within each"""
    times = {name: [] for name in legs}
    for rep in range(reps + 1):
        for name, fn in legs.items():
            seconds = fn()
            if rep:
                times[name].append(seconds)
    return {name: stats(xs) for name, xs in times.items()}


# ---- (a) tree only ---------------------------------------------------------------------------------------------------------------------
def residues(count, seed):
    raw = random.Random(seed).randbytes(16 * count)
    mask = int.from_bytes((b"\xff" * 15 + b"\x7f") * count, "little")
    return (int.from_bytes(raw, "little") & mask).to_bytes(16 * count, "little")


def tree_only(w, n, K):
    # the prover's layout: one matrix of K (w - 1) columns and one of K columns (w = 1: one segment)
    head, tail = sc.DeviceVector.from_bytes(residues(K * max(w - 1, 1) * n, 11 * K + w)), sc.DeviceVector.from_bytes(residues(K * n, 13 * K + w))
    segments = [(head, w - 1), (tail, 1)] if w > 1 else [(tail, 1)]
    views = [[sc.DeviceVector.wrap(head.ptr + 16 * n * (t * (w - 1) + c), n, head) for c in range(w - 1)] + [sc.DeviceVector.wrap(tail.ptr + 16 * n * t, n, tail)]
             for t in range(K)]
    sc.synchronize()

    def forest():
        f = sc.RowForest.build(segments, n, K)
        roots = f.roots
        f.free()
        return roots

    def trees():
        roots = []
        for columns in views:
            t = sc.RowTree.build(columns)
            roots.append(t.root)
            t.free()
        return roots
    assert forest() == trees(), "row forest and row trees disagree"

    def window(fn):
        def run():
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            return (time.perf_counter() - t0) / args.inner
        return run
    got = alternate({"forest": window(forest), "trees": window(trees)}, args.reps)
    f, t = got["forest"], got["trees"]
    say("w = %-3d N = 2^%-2d K = %-3d RowForest.build + roots %8.1f us (%.1f .. %.1f)   K x RowTree.build %8.1f us (%.1f .. %.1f)   trees / forest = %.2f" %
        (w, n.bit_length() - 1, K, f["median"] * 1e6, f["min"] * 1e6, f["max"] * 1e6, t["median"] * 1e6, t["min"] * 1e6, t["max"] * 1e6, t["median"] / f["median"]))
    return {"w": w, "N": n, "K": K, "forest_s": f, "trees_s": t, "ratio_trees_over_forest": t["median"] / f["median"]}


result = {"tree_only": [], "signatures": {}}
say("(a) tree only: one window = %d builds, %d repetitions after a warm-up" % (args.inner, args.reps))
for K in ks:
    result["tree_only"].append(tree_only(3, 1 << 12, K))
result["tree_only"].append(tree_only(17, 1 << 16, 4))

# ---- (b), (c) signatures ---------------------------------------------------------------------------------------------------------------
genuine = os.urandom


def seeded(seed):
    rng = random.Random(seed)
    os.urandom = lambda k: rng.getrandbits(8 * k).to_bytes(k, "little") if k else b""


def timed(fn, seed):
    seeded(seed)
    try:
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out
    finally:
        os.urandom = genuine


on, off = fast_rpsss.FastRPSSS(row_commitments=True), fast_rpsss.FastRPSSS()
stark = on.stark
say("(b), (c) signatures: %d trace rows, omicron domain 2^%d, FRI domain 2^%d, %d colinearity checks, %d FRI rounds; %d repetitions after a warm-up" %
    (stark.randomized_trace_length, stark.omicron_domain_length.bit_length() - 1, stark.fri_domain_length.bit_length() - 1,
     stark.num_colinearity_checks, stark.fri.num_rounds(), args.reps))
keys = [FieldElement(random.Random(5).randrange(on.field.p) + k, on.field) for k in range(max(ks))]
for K in ks:
    sks = keys[:K]
    times = {"batch": [], "singles": [], "off": []}
    sizes = {}
    for rep in range(args.reps + 1):
        documents = [b"document %d of repetition %d" % (m, rep) for m in range(K)]
        tb, together = timed(lambda: on.sign_batch(sks, documents), 1000 + rep)
        ts, one_by_one = timed(lambda: [on.sign(sk, document) for sk, document in zip(sks, documents)], 1000 + rep)
        to, plain = timed(lambda: off.sign_batch(sks, documents), 1000 + rep)
        assert together == one_by_one, "row-committed sign_batch and sign disagree"
        sizes = {"on": sum(map(len, together)) / K, "off": sum(map(len, plain)) / K}
        if rep:
            times["batch"].append(tb / K)
            times["singles"].append(ts / K)
            times["off"].append(to / K)
    stark.phase_log = []
    try:
        timed(lambda: on.sign_batch(sks, documents), 1000)
        phases = {}
        for phase, seconds in stark.phase_log:
            phases[phase] = phases.get(phase, 0.0) + seconds
    finally:
        stark.phase_log = None
    b, s, o = stats(times["batch"]), stats(times["singles"]), stats(times["off"])
    result["signatures"][K] = {"rows_sign_batch_per_signature_s": b, "rows_sign_per_signature_s": s, "ratio_sign_over_sign_batch": s["median"] / b["median"],
                               "option_off_sign_batch_per_signature_s": o, "signature_bytes": sizes, "rows_sign_batch_phases_s": phases}
    say("K = %-3d rows: sign_batch %8.2f ms/signature (%.2f .. %.2f)   K x sign %8.2f ms/signature (%.2f .. %.2f)   K x sign / sign_batch = %.2f   "
        "option off: sign_batch %8.2f ms/signature (%.2f .. %.2f)   bytes/signature %d on, %d off" %
        (K, b["median"] * 1e3, b["min"] * 1e3, b["max"] * 1e3, s["median"] * 1e3, s["min"] * 1e3, s["max"] * 1e3, s["median"] / b["median"],
         o["median"] * 1e3, o["min"] * 1e3, o["max"] * 1e3, sizes["on"], sizes["off"]))
    for phase, seconds in phases.items():
        say("          %-72s %8.2f ms/signature" % (phase, seconds * 1e3 / K))
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
if args.txt:
    with open(args.txt, "w") as f:
        f.write("\n".join(lines) + "\n")

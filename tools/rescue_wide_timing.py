#!/usr/bin/env python3
"""The generic-width Rescue-Prime entries on one MI355X (dev tool): sc_rescue_prime_permute_dev at several state widths beside its
floor, and at m = 2 the generic kernel (sc_rescue_prime_sponge_dev, rate 1, one block) against the fixed-width
sc_rescue_prime_hash_dev on the same inputs.

usage: rescue_wide_timing.py [--log-n 20] [--rounds 27] [--widths 2,3,4,8] [--runs 3] [--json OUT]

Everything in ONE process on resident operands; both sides are compared for equality first (the permutation's first lanes with the
host model RescuePrime.permutation, the sponge with the hash entry's bytes), then a warm-up of every leg and `runs` + `runs`
alternating repetitions, wall time from an idle stream to an idle stream.  Median with (min .. max).

The floor of a width is n (144 m + 2 m^2) rounds modular products over the 8.2e11 products/s hash_device reaches (DESIGN.md
section 6): per round and element 2 products for the cube and 142 for the inverse cube, and two m x m matrix products."""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
import starkcore as sc
import synth
from rescue_prime import RescuePrime

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--rounds", type=int, default=27)
ap.add_argument("--widths", default="2,3,4,8")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sc.init(0)
PRODUCTS_PER_SECOND = 8.2e11
n, rounds = 1 << args.log_n, args.rounds
lib = sc.lib()


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
    for _ in range(warmup):
        for leg in legs.values():
            leg()
    times = {name: [] for name in legs}
    for _ in range(runs):
        for name, leg in legs.items():
            times[name].append(leg())
    return {name: stats(xs) for name, xs in times.items()}


def spread(st):
    """(max - min) / median of one leg's repetitions"""
    return (st["max_ms"] - st["min_ms"]) / st["median_ms"]


result = {"n": n, "rounds": rounds, "runs": args.runs, "products_per_second": PRODUCTS_PER_SECOND, "permute": {}, "width_two": {}}

# ---- 1. the permutation at each width beside its floor ---------------------------------------------------------------------------
legs, floors = {}, {}
keep = []
for m in [int(x) for x in args.widths.split(",")]:
    rp = RescuePrime(m=m, capacity=1, rounds=rounds)
    states, out = sc.DeviceVector.from_bytes(synth.synth_packed(90 + m, m * n).tobytes()), sc.DeviceVector(m * n)

    def call(m=m, rp=rp, states=states, out=out):
        sc._check(lib.sc_rescue_prime_permute_dev(states.ptr, n, out.ptr, n, n, m, rp._params, rounds, None))
    call()
    lanes = min(n, 4)
    got, given = [sc.unpack(out.to_bytes(s * n, lanes)) for s in range(m)], [sc.unpack(states.to_bytes(s * n, lanes)) for s in range(m)]
    for k in range(lanes):
        assert [got[s][k] for s in range(m)] == rp.permutation([given[s][k] for s in range(m)]), "the kernel and the host model disagree"
    legs["m=%d" % m] = timed(call)
    floors["m=%d" % m] = n * (144 * m + 2 * m * m) * rounds / PRODUCTS_PER_SECOND
    keep.append((states, out))
for name, st in alternate(legs, args.runs).items():
    st["floor_ms"] = 1e3 * floors[name]
    st["over_floor"] = st["median_ms"] / st["floor_ms"]
    result["permute"][name] = st
    print("permute  %s, n = 2^%d, %d rounds:  %s   floor %8.3f ms   x%.2f" % (name, args.log_n, rounds, show(st), st["floor_ms"], st["over_floor"]), flush=True)
del keep

# ---- 2. m = 2: the generic kernel as a rate-1 sponge of one block against the fixed-width hash entry ---------------------------------
rp = RescuePrime(rounds=rounds)
xs = sc.DeviceVector.from_bytes(synth.synth_packed(99, n).tobytes())
by_hash, by_sponge = sc.DeviceVector(n), sc.DeviceVector(n)
hash_call = lambda: sc._check(lib.sc_rescue_prime_hash_dev(xs.ptr, n, rp._params, rounds, by_hash.ptr, None))
sponge_call = lambda: sc._check(lib.sc_rescue_prime_sponge_dev(xs.ptr, n, 1, by_sponge.ptr, n, 1, n, 2, 1, rp._params, rounds, None))
hash_call(), sponge_call()
assert by_hash.to_bytes() == by_sponge.to_bytes(), "the sponge entry and the hash entry disagree"
entry = alternate({"hash_dev": timed(hash_call), "sponge_dev": timed(sponge_call)}, args.runs)
entry["sponge_over_hash"] = entry["sponge_dev"]["median_ms"] / entry["hash_dev"]["median_ms"]
entry["spread"] = max(spread(entry["hash_dev"]), spread(entry["sponge_dev"]))
entry["floor_ms"] = 1e3 * n * (144 * 2 + 8) * rounds / PRODUCTS_PER_SECOND
result["width_two"] = entry
print("m = 2    n = 2^%d, %d rounds:  sc_rescue_prime_hash_dev %s   sc_rescue_prime_sponge_dev %s   sponge / hash x%.3f   (spread of the repetitions %.1f %%)" %
      (args.log_n, rounds, show(entry["hash_dev"]), show(entry["sponge_dev"]), entry["sponge_over_hash"], 100 * entry["spread"]), flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)

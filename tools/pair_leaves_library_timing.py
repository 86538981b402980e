#!/usr/bin/env python3
"""Fri.prove with pair leaves as one library call (Fri._prove_pairs_in_library, sc_fri_prove_pairs_dev) against its two yardsticks, on
one MI355X (dev tool).

usage: pair_leaves_library_timing.py [--parts a,d] [--runs 5] [--limit 300] [--json OUT]

The protocol of tools/pair_leaves_timing.py: one process on one box; every comparison checks its legs first, warms them up, then runs
`runs` repetitions of each leg ALTERNATING and takes medians with ranges; every part runs under a time limit of its own (--limit seconds,
SIGALRM: the process ends there).  Three legs:
    off      pair_leaves off (the one-call route sc_fri_prove_dev)
    on       pair_leaves on through the library route
    rounds   pair_leaves on, round by round (Fri.PAIRS_IN_LIBRARY = False): the behaviour before the library route existed
The yardsticks of `on` are `rounds` and `off` of the same run, never `on` itself.
(a) Fri.prove on a resident codeword of a polynomial of degree < N / 4: 2^12 with s = 64 (the signature scheme's FRI shape), 2^16 and 2^20
    with s = 40.  Checked first: all three proofs verify, `on` and `rounds` are the same bytes, and sc_fri_tail_stats counts one launch and
    no fall-back for `on`.
(d) FastStark.prove on workloads.synthetic_wide_instance (16 registers) at FRI 2^16, s = 40.  Checked first: all three proofs verify.
STARKCORE_FRI_TIMING=1 in the environment adds the library's own stamps on stderr: the phases of sc_fri_prove_pairs_dev and, per round of
the tail kernel, leaves | subtree | barrier | top levels | challenge back."""
import argparse, ctypes, json, os, signal, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
sys.setrecursionlimit(10000)
import starkcore as sc
import synth
import workloads
from algebra import Field
from fast_stark import DeviceTrace, FastStark, os_urandom_is_genuine
from fri import Fri
from ip import ProofStream

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="a,d")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--json", default=None)
args = ap.parse_args()
parts = args.parts.split(",")
sc.init(0)
assert os_urandom_is_genuine()
field = Field.main()
LEGS = ("off", "on", "rounds")


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": 1e3 * xs[len(xs) // 2], "min_ms": 1e3 * xs[0], "max_ms": 1e3 * xs[-1]}


def show(st):
    return "%8.3f ms (%.3f .. %.3f)" % (st["median_ms"], st["min_ms"], st["max_ms"])


def tail_stats():
    out = (ctypes.c_uint64 * 2)()
    sc._check(sc.lib().sc_fri_tail_stats(out))
    return out[0], out[1]


def leg_of(name, call):
    """the call with the route of leg `name` switched in, timed from a quiet device to a quiet device"""
    def leg(timing=True):
        Fri.PAIRS_IN_LIBRARY = name != "rounds"
        try:
            sc.synchronize()
            t0 = time.perf_counter()
            out = call()
            sc.synchronize()
            return (time.perf_counter() - t0) if timing else out
        finally:
            Fri.PAIRS_IN_LIBRARY = True
    return leg


def alternate(legs, runs, warmup=2):
    for _ in range(warmup):
        for leg in legs.values():
            leg()
    times = {name: [] for name in legs}
    for _ in range(runs):
        for name, leg in legs.items():
            times[name].append(leg())
    return {name: stats(xs) for name, xs in times.items()}


result = {"runs": args.runs, "fri_prove": {}, "stark": {}}

if "a" in parts:
    signal.alarm(args.limit)
    for log_n, s in ((12, 64), (16, 40), (20, 40)):
        n = 1 << log_n
        omega = field.primitive_nth_root(n)
        poly = sc.DeviceVector.from_bytes(synth.synth_packed(7, n // 4).tobytes())
        vec = sc.DeviceVector(n)
        sc._check(sc.lib().sc_coset_evaluate_dev(poly.ptr, n // 4, sc.fe_bytes(field.generator().value), sc.fe_bytes(omega.value), n, vec.ptr, None))
        provers = {"off": Fri(field.generator(), omega, n, 4, s), "on": Fri(field.generator(), omega, n, 4, s, pair_leaves=True)}
        provers["rounds"] = provers["on"]

        def prove(fri):
            stream = ProofStream()
            fri.prove(sc.DeviceCodeword(vec, field), stream)          # (a fresh view: a DeviceCodeword keeps the trees it was asked for)
            return stream.serialize()
        legs = {k: leg_of(k, lambda f=provers[k]: prove(f)) for k in LEGS}
        before = tail_stats()
        proofs = {"on": legs["on"](timing=False)}
        assert tail_stats() == (before[0] + 1, before[1]), "the library route launches the tail kernel once and does not fall back"
        proofs.update({k: legs[k](timing=False) for k in ("off", "rounds")})
        for k in LEGS:
            assert provers[k].verify(ProofStream().deserialize(proofs[k]), []) is True, "the proof of leg %s does not verify" % k
        assert proofs["on"] == proofs["rounds"], "the two routes of the option make different proofs"
        got = alternate(legs, args.runs)
        result["fri_prove"]["2^%d_s%d" % (log_n, s)] = {"prove": got, "proof_bytes": {k: len(v) for k, v in proofs.items()}}
        print("(a) Fri.prove 2^%d s = %d   off %s   on, library %s   on, round by round %s   bytes off %d  on %d" % (
            log_n, s, show(got["off"]), show(got["on"]), show(got["rounds"]), len(proofs["off"]), len(proofs["on"])), flush=True)
        del vec, poly
    signal.alarm(0)

if "d" in parts:
    signal.alarm(args.limit)
    checks = 40
    f, T, _, packed, air, boundary = workloads.synthetic_wide_instance(16, 16, checks)
    provers = {"off": FastStark(f, 4, checks, 2 * checks, 16, T), "on": FastStark(f, 4, checks, 2 * checks, 16, T, pair_leaves=True)}
    provers["rounds"] = provers["on"]
    tz, tz_codeword, root = provers["off"].preprocess(device_resident=True)
    trace = DeviceTrace.from_packed(packed, f)
    legs = {k: leg_of(k, lambda p=provers[k]: p.prove(trace, air, boundary, tz, tz_codeword)) for k in LEGS}
    proofs = {k: legs[k](timing=False) for k in LEGS}
    for k in LEGS:
        assert provers[k].verify(proofs[k], air, boundary, root) is True, "the proof of leg %s does not verify" % k
    assert max(len(proofs["on"]), len(proofs["rounds"])) < len(proofs["off"])       # (fresh randomness per proof: the two routes' bytes are compared by the tests, under seeded os.urandom)
    prove = alternate(legs, args.runs)
    result["stark"]["wide16_2^16"] = {"prove": prove, "proof_bytes": {k: len(v) for k, v in proofs.items()}}
    print("(d) FastStark 16 registers FRI 2^16   prove off %s   on, library %s   on, round by round %s   bytes off %d  on %d" % (
        show(prove["off"]), show(prove["on"]), show(prove["rounds"]), len(proofs["off"]), len(proofs["on"])), flush=True)
    signal.alarm(0)

if args.json:
    with open(args.json, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)

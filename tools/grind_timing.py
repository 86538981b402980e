#!/usr/bin/env python3
"""The proof-of-work search (sc_grind, csrc/grind.cuh) and the proofs that carry one, on one MI355X (dev tool).

usage: grind_timing.py [--out profiles/grinding] [--seeds 16] [--reps 5] [--skip-proofs] [--baseline-package DIR]

(a) the search: per bits in 20, 24, 28 the smallest nonce of `--seeds` seeds through sc_grind, host clock around each call (a call
    returns with the nonce on the host); trials = nonce + 1; median and range of the calls' trials per second and the sum of the
    trials over the sum of the times.  The kernel alone: a search that cannot succeed (63 bits) over 2^32 nonces.  The host loop
    (sc_grind_host, one core): the same over 2^23 nonces.  The yardstick: the one-lane Keccak of profiles/r05/keccak_wave_ubench.txt
    (8.87 us per permutation per wave = 64 trials) on every SIMD of the device's CUs.
(c) the window: the unsuccessful 2^30-nonce search and the 20-bit searches of (a) at "grind_window" = 2^14 .. 2^26; the loop
    (default) and the unrolled kernel alternating at the default window.
(b) the proofs: FastRPSSS at (colinearity checks, grinding bits) = (64, 0), (54, 20), (48, 32): signature bytes, sign and verify
    time, per-member time of sign_batch of 16; the first repetition of each is a warm-up and is dropped.  With --baseline-package
    (the stark-anatomy_amd directory of another checkout, the parent commit's) the default scheme's sign is timed in child processes
    that alternate between that package and this one, under the same seeded os.urandom, and the signatures' hashes are compared.
Writes grind_timing.txt, grind_timing.json and kernel_regs.txt (tools/kernel_regs.py grind_window) into --out."""
import argparse, hashlib, json, os, random, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grinding"))
ap.add_argument("--seeds", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-proofs", action="store_true")
ap.add_argument("--baseline-package", default=None)
ap.add_argument("--package", default=os.path.join(REPO, "stark-anatomy_amd"), help=argparse.SUPPRESS)
ap.add_argument("--default-sign-only", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
sys.path.insert(0, args.package)
sys.setrecursionlimit(10000)
import starkcore as sc
import fast_rpsss
from algebra import FieldElement

sc.init(0)
genuine = os.urandom


def seeded(seed):
    rng = random.Random(seed)
    os.urandom = lambda k: rng.getrandbits(8 * k).to_bytes(k, "little") if k else b""


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def sign_times(scheme, reps, seed=77):
    """[seconds] of reps + 1 signatures (the first dropped) under a seeded os.urandom, and the last signature"""
    sk = FieldElement(random.Random(5).randrange(scheme.field.p), scheme.field)
    times = []
    try:
        for rep in range(reps + 1):
            seeded(seed + rep)
            t, signature = timed(lambda: scheme.sign(sk, b"document %d" % rep))
            times.append(t)
    finally:
        os.urandom = genuine
    return times[1:], signature, sk


if args.default_sign_only:                                 # a child of the comparison with another checkout's package
    times, signature, _ = sign_times(fast_rpsss.FastRPSSS(), args.reps)
    print(json.dumps({"times": times, "sha256": hashlib.sha256(signature).hexdigest(), "bytes": len(signature)}))
    sys.exit(0)

import grinding
os.makedirs(args.out, exist_ok=True)
lines, result = [], {}


def say(text=""):
    print(text, flush=True)
    lines.append(text)


seeds = [hashlib.shake_256(b"grind timing seed %d" % k).digest(32) for k in range(args.seeds)]
cus = 256                                                  # MI355X: 256 CUs of 4 SIMDs
yardstick = cus * 4 * 64 / 8.87e-6
say("yardstick: one wave per SIMD at the one-lane Keccak of profiles/r05 (8.87 us per 64 trials) on %d CUs x 4 SIMDs = %.2f G trials/s (an estimate)" % (cus, yardstick / 1e9))
result["yardstick_trials_per_s"] = yardstick
result["yardstick_cus"] = cus

# warm-up: code objects, the pinned pool, the clock
for _ in range(3):
    grinding.grind(seeds[0], 63, 0, 1 << 28)


def fixed_work(nonces, reps=3):
    """trials per second of a search over `nonces` nonces that cannot succeed"""
    out = []
    for _ in range(reps):
        t, found = timed(lambda: grinding.grind(seeds[0], 63, 0, nonces))
        assert found is None
        out.append(nonces / t)
    return stats(out)


say()
say("(a) the search")
kernel_rate = fixed_work(1 << 32)
result["kernel_trials_per_s"] = kernel_rate
say("sc_grind, 2^32 nonces without a hit: %.2f G trials/s (%.2f .. %.2f); %.0f %% of the yardstick" %
    (kernel_rate["median"] / 1e9, kernel_rate["min"] / 1e9, kernel_rate["max"] / 1e9, 100 * kernel_rate["median"] / yardstick))
host = []
for _ in range(3):
    t, found = timed(lambda: grinding.grind_library_host(seeds[0], 63, 0, 1 << 23))
    host.append((1 << 23) / t)
host_rate = stats(host)
result["host_trials_per_s"] = host_rate
say("sc_grind_host, 2^23 nonces without a hit on one core: %.2f M trials/s (%.2f .. %.2f)" % (host_rate["median"] / 1e6, host_rate["min"] / 1e6, host_rate["max"] / 1e6))
result["search"] = {}
nonces_at = {}
for bits in (20, 24, 28):
    rates, seconds, trials = [], [], []
    for seed in seeds:
        t, nonce = timed(lambda: grinding.grind(seed, bits))
        assert nonce is not None and grinding.accepts(seed, nonce, bits)
        rates.append((nonce + 1) / t)
        seconds.append(t)
        trials.append(nonce + 1)
    nonces_at[bits] = [t - 1 for t in trials]
    r, s = stats(rates), stats(seconds)
    overall = sum(trials) / sum(seconds)
    result["search"][bits] = {"trials_per_s": r, "seconds": s, "sum_trials_over_sum_seconds": overall, "median_trials": stats(trials)["median"]}
    say("%2d bits, %d seeds: median %.3f G trials/s per call (%.3f .. %.3f), all trials / all time %.3f G trials/s; a call %.3f ms (%.3f .. %.3f); "
        "the host loop at its rate: %.1f ms for the median search, x %.0f" %
        (bits, len(seeds), r["median"] / 1e9, r["min"] / 1e9, r["max"] / 1e9, overall / 1e9, s["median"] * 1e3, s["min"] * 1e3, s["max"] * 1e3,
         stats(trials)["median"] / host_rate["median"] * 1e3, stats(trials)["median"] / host_rate["median"] / s["median"]))
t, nonce = timed(lambda: grinding.grind_library_host(seeds[0], 20))
assert nonce == nonces_at[20][0]
say("sc_grind_host on seed 0 at 20 bits: the same nonce (%d) in %.1f ms" % (nonce, t * 1e3))

say()
say("(c) the window (\"grind_window\"): 2^30 nonces without a hit, and the %d searches at 20 and 24 bits" % len(seeds))
result["window"] = {}
for log in range(14, 27, 2):
    sc.set_tuning("grind_window", 1 << log)
    rate = fixed_work(1 << 30)
    medians = {}
    for bits in (20, 24):
        ts = []
        for seed, want in zip(seeds, nonces_at[bits]):
            t, nonce = timed(lambda: grinding.grind(seed, bits))
            assert nonce == want
            ts.append(t)
        medians[bits] = stats(ts)
    result["window"][log] = {"trials_per_s": rate, "seconds_20_bits": medians[20], "seconds_24_bits": medians[24]}
    say("window 2^%-2d  %.3f G trials/s (%.3f .. %.3f)   20 bits: %.3f ms per search (%.3f .. %.3f)   24 bits: %.3f ms (%.3f .. %.3f)" %
        (log, rate["median"] / 1e9, rate["min"] / 1e9, rate["max"] / 1e9, medians[20]["median"] * 1e3, medians[20]["min"] * 1e3, medians[20]["max"] * 1e3,
         medians[24]["median"] * 1e3, medians[24]["min"] * 1e3, medians[24]["max"] * 1e3))
sc.set_tuning("grind_window", -1)
forms = {0: [], 1: []}
for _ in range(4):
    for unrolled in (0, 1):
        sc.set_tuning("grind_unrolled", unrolled)
        forms[unrolled].append(fixed_work(1 << 31, reps=1)["median"])
sc.set_tuning("grind_unrolled", 0)
result["forms"] = {"loop": stats(forms[0]), "unrolled": stats(forms[1])}
say("rounds 1 .. 22 as a loop: %.3f G trials/s (%.3f .. %.3f); unrolled: %.3f G trials/s (%.3f .. %.3f)  [2^31 nonces, alternating, 4 each]" %
    (stats(forms[0])["median"] / 1e9, min(forms[0]) / 1e9, max(forms[0]) / 1e9, stats(forms[1])["median"] / 1e9, min(forms[1]) / 1e9, max(forms[1]) / 1e9))

try:
    regs = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_regs.py"), "grind_window"], capture_output=True, text=True).stdout
except OSError:
    regs = ""
if regs.strip():
    with open(os.path.join(args.out, "kernel_regs.txt"), "w") as f:
        f.write(regs)
    say()
    say(regs.rstrip())

if not args.skip_proofs:
    say()
    say("(b) the proofs: FastRPSSS(num_colinearity_checks, grinding_bits)")
    result["proofs"] = {}
    for checks, bits in ((64, 0), (54, 20), (48, 32)):
        reps = args.reps if bits < 30 else max(2, args.reps // 2)
        scheme = fast_rpsss.FastRPSSS(checks, bits)
        sign, signature, sk = sign_times(scheme, reps)
        pk = scheme.rp.hash(sk)
        document = b"document %d" % reps
        verify = []
        for _ in range(reps + 1):
            t, ok = timed(lambda: scheme.verify(pk, document, signature))
            assert ok is True
            verify.append(t)
        batch = []
        documents = [b"member %d" % m for m in range(16)]
        try:
            for rep in range((reps if bits < 30 else 1) + 1):
                seeded(500 + rep)
                t, signatures = timed(lambda: scheme.sign_batch([sk] * 16, documents))
                batch.append(t / 16)
        finally:
            os.urandom = genuine
        assert scheme.verify_batch([pk] * 16, documents, signatures) == [True] * 16
        s, v, b = stats(sign), stats(verify[1:]), stats(batch[1:])
        result["proofs"]["%d,%d" % (checks, bits)] = {"signature_bytes": len(signature), "sha256": hashlib.sha256(signature).hexdigest(), "sign_s": s, "verify_s": v,
                                                      "sign_batch_16_per_member_s": b, "fri_rounds": scheme.stark.fri.num_rounds(), "randomizers": scheme.stark.num_randomizers}
        say("(%2d, %2d): signature %7d bytes   sign %9.2f ms (%.2f .. %.2f)   verify %8.2f ms (%.2f .. %.2f)   sign_batch of 16: %9.2f ms per member (%.2f .. %.2f)" %
            (checks, bits, len(signature), s["median"] * 1e3, s["min"] * 1e3, s["max"] * 1e3, v["median"] * 1e3, v["min"] * 1e3, v["max"] * 1e3,
             b["median"] * 1e3, b["min"] * 1e3, b["max"] * 1e3))
    if args.baseline_package:
        runs = {"this": [], "baseline": []}
        for _ in range(3):
            for name, package in (("baseline", args.baseline_package), ("this", args.package)):
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--package", package, "--default-sign-only", "--reps", str(args.reps)],
                                       capture_output=True, text=True, timeout=300)
                assert child.returncode == 0, child.stderr[-2000:]
                runs[name].append(json.loads(child.stdout.strip().splitlines()[-1]))
        same = len({r["sha256"] for rs in runs.values() for r in rs}) == 1
        mine, theirs = [t for r in runs["this"] for t in r["times"]], [t for r in runs["baseline"] for t in r["times"]]
        per_process = {name: [stats(r["times"])["median"] for r in rs] for name, rs in runs.items()}
        result["default_against_baseline"] = {"same_signature": same, "this_s": stats(mine), "baseline_s": stats(theirs), "medians_per_process_s": per_process}
        say("(64, 0) against the baseline package, 3 processes each, alternating, %d signatures per process: the same signature bytes: %s; "
            "sign %.2f ms (%.2f .. %.2f) here, %.2f ms (%.2f .. %.2f) there; medians per process %s here, %s there" %
            (args.reps, same, stats(mine)["median"] * 1e3, min(mine) * 1e3, max(mine) * 1e3, stats(theirs)["median"] * 1e3, min(theirs) * 1e3, max(theirs) * 1e3,
             ", ".join("%.2f" % (m * 1e3) for m in per_process["this"]), ", ".join("%.2f" % (m * 1e3) for m in per_process["baseline"])))
        assert same, "the default scheme's signature changed"

with open(os.path.join(args.out, "grind_timing.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
with open(os.path.join(args.out, "grind_timing.json"), "w") as f:
    json.dump(result, f, indent=1)

#!/usr/bin/env python3
"""The hash kernel alone, for rocprofv3 --kernel-trace --stats (dev tool): RescuePrime.hash_device over 2^20 inputs, --reps launches.

usage: rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/rpsss_kernel_stats.py [--log 20] [--reps 10]"""
import argparse, os, random, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
import starkcore as sc
import rescue_prime

ap = argparse.ArgumentParser()
ap.add_argument("--log", type=int, default=20)
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
sc.init(0)
rp = rescue_prime.RescuePrime()
n = 1 << args.log
vec = sc.DeviceVector.from_bytes(random.Random(3).randbytes(16 * n))
out, trace = sc.DeviceVector(n), sc.DeviceVector(2 * n * (rp.N + 1))
for _ in range(args.reps):
    sc._check(sc.lib().sc_rescue_prime_hash_dev(vec.ptr, n, rp._params, rp.N, out.ptr, None))
for _ in range(max(1, args.reps // 5)):
    sc._check(sc.lib().sc_rescue_prime_trace_dev(vec.ptr, n, rp._params, rp.N, trace.ptr, None))
sc.synchronize()
print("launched", args.reps, "hash and", max(1, args.reps // 5), "trace kernels over", n, "inputs")

#!/usr/bin/env python3
"""Pair leaves for FRI against the tutorial's three openings per colinearity test, on one MI355X (dev tool).

usage: pair_leaves_timing.py [--parts a,b,c,d] [--runs 3] [--limit 300] [--json OUT]

One process on one box.  Every comparison checks its two legs first, warms both up, then runs `runs` + `runs` repetitions ALTERNATING
and takes medians with ranges; the yardstick of every figure is the option-off leg of the same run.  Every part runs under a time limit
of its own (--limit seconds, SIGALRM: the process ends there).
(a) Fri.prove with pair_leaves off and on, on a resident codeword of a polynomial of degree < N / 4: 2^12 with s = 64 (the signature
    scheme's FRI shape), 2^16 and 2^20 with s = 40.  Checked first: both proofs verify; the proofs' path digests differ by exactly
    s * sum over the queried rounds of 2 log2(N_r).
(b) one round of the commit phase, enqueue to root: sc_fri_fold_pairs_commit_dev against sc_fri_fold_commit_dev at N = 2^16, 2^20,
    2^22.  Checked first: both write the same folded codeword.
(c) FastRPSSS without and with row_commitments: sign, verify and signature bytes, pair_leaves off and on.
(d) FastStark on workloads.synthetic_wide_instance (16 registers) at FRI 2^16, s = 40: proof bytes and prove, off and on."""
import argparse, ctypes, json, os, pickle, signal, sys, time
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
ap.add_argument("--parts", default="a,b,c,d")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--json", default=None)
args = ap.parse_args()
parts = args.parts.split(",")
sc.init(0)
assert os_urandom_is_genuine()
field = Field.main()


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


def digests(proof):
    """64-byte digests inside the lists (authentication paths) of a pickled proof"""
    return sum(sum(1 for d in o if type(d) is bytes and len(d) == 64) for o in pickle.loads(proof) if type(o) is list)


def fewer_digests(fri):
    """what pair leaves save in FRI's query phase: per test and queried round the paths of a and b (log2 N_r each) and of c
    (log2 N_r - 1) become one of log2 N_r - 1"""
    return fri.num_colinearity_tests * sum(2 * ((fri.domain_length >> r).bit_length() - 1) for r in range(fri.num_rounds() - 1))


result = {"runs": args.runs, "fri_prove": {}, "fold_commit": {}, "sign": {}, "stark": {}}

if "a" in parts:
    signal.alarm(args.limit)
    for log_n, s in ((12, 64), (16, 40), (20, 40)):
        n = 1 << log_n
        omega = field.primitive_nth_root(n)
        poly = sc.DeviceVector.from_bytes(synth.synth_packed(7, n // 4).tobytes())
        vec = sc.DeviceVector(n)
        sc._check(sc.lib().sc_coset_evaluate_dev(poly.ptr, n // 4, sc.fe_bytes(field.generator().value), sc.fe_bytes(omega.value), n, vec.ptr, None))
        provers = {"off": Fri(field.generator(), omega, n, 4, s), "on": Fri(field.generator(), omega, n, 4, s, pair_leaves=True)}

        def prove(fri):
            stream = ProofStream()
            fri.prove(sc.DeviceCodeword(vec, field), stream)          # (a fresh view: a DeviceCodeword keeps the trees it was asked for)
            return stream.serialize()
        proofs = {k: prove(f) for k, f in provers.items()}
        for k, f in provers.items():
            assert f.verify(ProofStream().deserialize(proofs[k]), []) is True, "a proof with the option %s does not verify" % k
        assert digests(proofs["off"]) - digests(proofs["on"]) == fewer_digests(provers["on"]), "digest count"
        got = alternate({k: timed(lambda f=f: prove(f)) for k, f in provers.items()}, args.runs)
        rec = {"prove": got, "proof_bytes": {k: len(v) for k, v in proofs.items()}, "path_digests": {k: digests(v) for k, v in proofs.items()}}
        result["fri_prove"]["2^%d_s%d" % (log_n, s)] = rec
        print("(a) Fri.prove 2^%d s = %d   off %s  on %s   bytes off %d  on %d   path digests off %d  on %d" % (
            log_n, s, show(got["off"]), show(got["on"]), len(proofs["off"]), len(proofs["on"]), rec["path_digests"]["off"], rec["path_digests"]["on"]), flush=True)
        del vec, poly
    signal.alarm(0)

if "b" in parts:
    signal.alarm(args.limit)
    lib = sc.lib()
    for log_n in (16, 20, 22):
        n = 1 << log_n
        omega = field.primitive_nth_root(n)
        source = sc.DeviceVector.from_bytes(synth.synth_packed(9, n).tobytes())
        outputs = {"off": sc.DeviceVector(n // 2), "on": sc.DeviceVector(n // 2)}
        constants = (sc.fe_bytes(0x1234567890ABCDEF1234567890ABCDEF), sc.fe_bytes(field.generator().value), sc.fe_bytes(omega.value))
        entries = {"off": lib.sc_fri_fold_commit_dev, "on": lib.sc_fri_fold_pairs_commit_dev}

        def round_trip(k):
            handle, root = ctypes.c_void_p(), ctypes.create_string_buffer(64)
            sc._check(entries[k](source.ptr, n, *constants, outputs[k].ptr, ctypes.byref(handle), None))
            sc._check(lib.sc_merkle_root(handle, root))               # enqueue to root
            sc._check(lib.sc_merkle_free(handle))
            return root.raw
        roots = {k: round_trip(k) for k in entries}
        assert outputs["off"].to_bytes() == outputs["on"].to_bytes() and roots["off"] != roots["on"], "the folded codewords"
        got = alternate({k: timed(lambda k=k: round_trip(k)) for k in entries}, args.runs)
        result["fold_commit"]["2^%d" % log_n] = got
        print("(b) fold + commit N = 2^%d, enqueue to root   sc_fri_fold_commit_dev %s   sc_fri_fold_pairs_commit_dev %s" % (log_n, show(got["off"]), show(got["on"])), flush=True)
        del source, outputs
    signal.alarm(0)

if "c" in parts:
    from fast_rpsss import FastRPSSS
    for rows in (False, True):
        signal.alarm(args.limit)
        schemes = {"off": FastRPSSS(row_commitments=rows), "on": FastRPSSS(row_commitments=rows, pair_leaves=True)}
        sk = schemes["off"].field.sample(b"the key of the timing tool")
        pk = schemes["off"].rp.hash(sk)
        signatures = {k: s.sign(sk, b"a document") for k, s in schemes.items()}
        for k, s in schemes.items():
            assert s.verify(pk, b"a document", signatures[k]) is True, "a signature with the option %s does not verify" % k
        assert digests(signatures["off"]) - digests(signatures["on"]) == fewer_digests(schemes["on"].stark.fri), "digest count"
        sign = alternate({k: timed(lambda s=s: s.sign(sk, b"a document")) for k, s in schemes.items()}, args.runs)
        verify = alternate({k: timed(lambda s=s, k=k: s.verify(pk, b"a document", signatures[k])) for k, s in schemes.items()}, args.runs, warmup=1)
        name = "row_commitments" if rows else "plain"
        result["sign"][name] = {"sign": sign, "verify": verify, "signature_bytes": {k: len(v) for k, v in signatures.items()},
                                "path_digests": {k: digests(v) for k, v in signatures.items()}}
        print("(c) FastRPSSS %-15s   sign off %s  on %s   verify off %s  on %s   bytes off %d  on %d" % (
            name, show(sign["off"]), show(sign["on"]), show(verify["off"]), show(verify["on"]), len(signatures["off"]), len(signatures["on"])), flush=True)
        del schemes
        signal.alarm(0)

if "d" in parts:
    signal.alarm(args.limit)
    checks = 40
    f, T, _, packed, air, boundary = workloads.synthetic_wide_instance(16, 16, checks)
    provers = {"off": FastStark(f, 4, checks, 2 * checks, 16, T), "on": FastStark(f, 4, checks, 2 * checks, 16, T, pair_leaves=True)}
    tz, tz_codeword, root = provers["off"].preprocess(device_resident=True)
    trace = DeviceTrace.from_packed(packed, f)
    proofs = {k: p.prove(trace, air, boundary, tz, tz_codeword) for k, p in provers.items()}
    for k, p in provers.items():
        assert p.verify(proofs[k], air, boundary, root) is True, "a proof with the option %s does not verify" % k
    assert digests(proofs["off"]) - digests(proofs["on"]) == fewer_digests(provers["on"].fri), "digest count"
    prove = alternate({k: timed(lambda p=p: p.prove(trace, air, boundary, tz, tz_codeword)) for k, p in provers.items()}, args.runs)
    result["stark"]["wide16_2^16"] = {"prove": prove, "proof_bytes": {k: len(v) for k, v in proofs.items()}, "path_digests": {k: digests(v) for k, v in proofs.items()}}
    print("(d) FastStark 16 registers FRI 2^16   prove off %s  on %s   bytes off %d  on %d" % (
        show(prove["off"]), show(prove["on"]), len(proofs["off"]), len(proofs["on"])), flush=True)
    signal.alarm(0)

if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)

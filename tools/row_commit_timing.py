#!/usr/bin/env python3
"""Row commitments against one tree per column, on one MI355X (dev tool).

usage: row_commit_timing.py [--parts a,b,c] [--runs 3] [--checks 40] [--json OUT]

One process on one box.  Every comparison checks its two sides first, warms both up, then runs `runs` + `runs` repetitions
ALTERNATING and takes medians; the yardstick of every time is the option-off leg of the same run.
(a) the tree alone: starkcore.RowTree.build (one tree over the rows) against Merkle.commit_batch (one tree per column, as one forest)
    on the same resident columns, w = 3 and 17 at N = 2^16 and 2^20, w = 3 at 2^24.  Checked first: the row tree's root and four
    opened rows with their paths against hashlib (the root up to 2^16), the forest's roots against Merkle.commit column by column.
(b) whole proofs: FastStark.prove, verify and len(proof) with row_commitments off and on -- workloads.synthetic_wide_instance (16
    registers) at FRI 2^16 and 2^20, workloads.synthetic_stark_instance at FRI 2^20; device-resident traces, the operating system's
    os.urandom.  Checked first: a proof of each kind verifies.
(c) signatures: FastRPSSS sign, verify and signature bytes, off and on."""
import argparse, json, os, sys, time
from hashlib import blake2b
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
sys.setrecursionlimit(10000)
import starkcore as sc
import synth
import workloads
from algebra import Field
from fast_stark import DeviceTrace, FastStark, os_urandom_is_genuine
from merkle import Merkle

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="a,b,c")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--checks", type=int, default=40)
ap.add_argument("--json", default=None)
args = ap.parse_args()
parts = args.parts.split(",")
sc.init(0)
assert os_urandom_is_genuine()


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


result = {"runs": args.runs, "tree": {}, "prove": {}, "sign": {}}

if "a" in parts:
    field = Field.main()
    for log_n, widths in ((16, (3, 17)), (20, (3, 17)), (24, (3,))):
        n = 1 << log_n
        for w in widths:
            packed = [synth.synth_packed(100 + c, n).tobytes() for c in range(w)]
            columns = [sc.DeviceCodeword(sc.DeviceVector.from_bytes(p), field) for p in packed]
            tree = sc.RowTree.build(columns)
            if log_n <= 16:
                level = [blake2b(b"".join(p[16 * i:16 * i + 16] for p in packed), person=Merkle.ROW_PERSON).digest() for i in range(n)]
                assert tree.root == Merkle.commit_(level), "row tree root"
            picks = [0, n - 1, n // 2 - 1, n // 2]
            rows, paths = tree.query(picks)
            for i, row, path in zip(picks, rows, paths):
                assert sc.pack(row) == b"".join(p[16 * i:16 * i + 16] for p in packed)
                assert Merkle.verify_(tree.root, i, path, blake2b(sc.pack(row), person=Merkle.ROW_PERSON).digest()), "opened row"
            fresh = lambda: [sc.DeviceCodeword(c.vec, field) for c in columns]          # (a DeviceCodeword keeps the tree it was asked for)
            assert Merkle.commit_batch(fresh()) == [Merkle.commit(c) for c in fresh()], "forest roots"
            tree.free()
            legs = {"per_column": timed(lambda: Merkle.commit_batch(fresh())), "rows": timed(lambda: sc.RowTree.build(columns).free())}
            got = alternate(legs, args.runs)
            result["tree"]["w%d_2^%d" % (w, log_n)] = got
            print("(a) tree alone  w = %2d  N = 2^%d   one tree per column %s   row tree %s" % (w, log_n, show(got["per_column"]), show(got["rows"])), flush=True)
            del columns, packed

if "b" in parts:
    shapes = [("wide16", 16, 16), ("wide16", 16, 20), ("stark2", 2, 20)]
    for name, registers, log_fri in shapes:
        if registers == 2:
            field, T, packed, air, boundary = workloads.synthetic_stark_instance(log_fri, args.checks)
        else:
            field, T, _, packed, air, boundary = workloads.synthetic_wide_instance(log_fri, registers, args.checks)
        provers = {"off": FastStark(field, 4, args.checks, 2 * args.checks, registers, T),
                   "on": FastStark(field, 4, args.checks, 2 * args.checks, registers, T, row_commitments=True)}
        tz, tz_codeword, root = provers["off"].preprocess(device_resident=True)
        trace = DeviceTrace.from_packed(packed, field)
        proofs = {k: p.prove(trace, air, boundary, tz, tz_codeword) for k, p in provers.items()}
        for k, p in provers.items():
            assert p.verify(proofs[k], air, boundary, root) is True, "a proof with the option %s does not verify" % k
        prove = alternate({k: timed(lambda p=p: p.prove(trace, air, boundary, tz, tz_codeword)) for k, p in provers.items()}, args.runs)
        verify = alternate({k: timed(lambda p=p, k=k: p.verify(proofs[k], air, boundary, root)) for k, p in provers.items()}, args.runs, warmup=1)
        rec = {"prove": prove, "verify": verify, "proof_bytes": {k: len(v) for k, v in proofs.items()}}
        result["prove"]["%s_2^%d" % (name, log_fri)] = rec
        print("(b) %s FRI 2^%d   prove off %s  on %s   verify off %s  on %s   bytes off %d  on %d" % (
            name, log_fri, show(prove["off"]), show(prove["on"]), show(verify["off"]), show(verify["on"]), len(proofs["off"]), len(proofs["on"])), flush=True)
        del trace, tz, tz_codeword, provers

if "c" in parts:
    from fast_rpsss import FastRPSSS
    schemes = {"off": FastRPSSS(), "on": FastRPSSS(row_commitments=True)}
    sk = schemes["off"].field.sample(b"the key of the timing tool")
    pk = schemes["off"].rp.hash(sk)
    signatures = {k: s.sign(sk, b"a document") for k, s in schemes.items()}
    for k, s in schemes.items():
        assert s.verify(pk, b"a document", signatures[k]) is True, "a signature with the option %s does not verify" % k
    sign = alternate({k: timed(lambda s=s: s.sign(sk, b"a document")) for k, s in schemes.items()}, args.runs)
    verify = alternate({k: timed(lambda s=s, k=k: s.verify(pk, b"a document", signatures[k])) for k, s in schemes.items()}, args.runs, warmup=1)
    result["sign"] = {"sign": sign, "verify": verify, "signature_bytes": {k: len(v) for k, v in signatures.items()}}
    print("(c) FastRPSSS   sign off %s  on %s   verify off %s  on %s   bytes off %d  on %d" % (
        show(sign["off"]), show(sign["on"]), show(verify["off"]), show(verify["on"]), len(signatures["off"]), len(signatures["on"])), flush=True)

if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)

#!/usr/bin/env python3
"""Rescue-Prime Merkle membership proofs on one MI355X (dev tool; method of tools/rescue_merkle_timing.py).

usage: membership_timing.py [--rounds 27] [--depth 20] [--runs 3] [--out-dir profiles/rescue_membership]

Everything in ONE process; both sides of every comparison are compared for equality first, then a warm-up of every leg and `runs` +
`runs` alternating repetitions, wall time from an idle stream to an idle stream.  Median with (min .. max).  A form is "faster" only
when it wins by more than the spread of the repetitions (max - min of either leg).

(a) sc_rescue_merkle_path_trace_dev, one lane per state register (split) against one lane per item (wide), at k = 1, 64, 4096, 65536,
    (m, capacity, d) = (4, 1, 1) and (8, 3, 2); beside it sc_rescue_merkle_verify_batch on the same paths (rows of one element) in both
    forms up to k = 4096: the walk the trace repeats.  The inputs are host arrays, so every call time includes staging them.
(b) the trace kernel against the same trace assembled from one sc_rescue_prime_trace_states_dev call per level: the first states put
    together, and each level's states, sibling and bit columns copied into place, by torch on the library stream; siblings and bits
    resident beforehand (which favours the loop).
(c) RescueMembership at (4, 1, 1), 64 colinearity checks: one `prove`, and `prove_batch` of 16."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
import torch
import starkcore as sc
import synth
from rescue_prime import RescuePrime
from rescue_merkle import RescueMerkle, set_split_max_nodes, INT32_MAX
from rescue_membership import RescueMembership

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=27)
ap.add_argument("--depth", type=int, default=20)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--counts", default="1,64,4096,65536")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--checks", type=int, default=64)
ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "rescue_membership"))
args = ap.parse_args()
sc.init(0)
lib = sc.lib()
SHAPES = ((4, 1, 1), (8, 3, 2))
ext = torch.cuda.ExternalStream(sc.library_stream())
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


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


def verdict(a, b, name_a, name_b):
    """which of two legs is faster by more than the spread of the repetitions; a tie otherwise"""
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    if abs(a["median_ms"] - b["median_ms"]) <= spread:
        return "tie", spread
    return (name_a if a["median_ms"] < b["median_ms"] else name_b), spread


def view(vec):
    return torch.as_tensor(vec, device="cuda")


def same(a, b):
    return bool(torch.equal(view(a), view(b)))


def inputs(m, d, k, depth):
    """k items of seeded canonical words: (leaves, indices, paths) as the entry takes them, and the indices as a list"""
    leaves = synth.synth_packed(7 + m, k * d).tobytes()
    paths = synth.synth_packed(70 + m, k * depth * d).tobytes()
    indices = [(0x9E3779B97F4A7C15 * (t + 1)) % (1 << depth) for t in range(k)]
    return leaves, (ctypes.c_uint64 * k)(*indices), paths, indices


def trace_call(rp, d, depth, k, leaves, idx, paths, out, key):
    def call():
        set_split_max_nodes(key)
        sc._check(lib.sc_rescue_merkle_path_trace_dev(leaves, idx, paths, k, depth, d, rp.m, rp.rate, rp._params, rp.N, out.ptr, None))
    return call


def level_loop(rp, d, depth, k, leaves, indices, paths, out):
    """the caller's loop over the existing entry: per level the first states put together, one sc_rescue_prime_trace_states_dev, the
    states and the side columns copied into place"""
    m, N = rp.m, rp.N
    C, W, T = N + 1, m + d + 1, depth * (N + 1) + 1
    sibs = sc.DeviceVector.from_bytes(paths)                      # [k][depth][d]
    leaf = sc.DeviceVector.from_bytes(leaves)                     # [k][d]
    bits = torch.tensor([[(i >> j) & 1 for i in indices] for j in range(depth)], dtype=torch.bool, device="cuda")
    states, level = sc.DeviceVector.zeros(m * k), sc.DeviceVector(m * k * C)
    sc.synchronize()
    whole, first = view(out).view(k, W, T, 2), view(states).view(m, k, 2)
    sib_all, leaf_all, level_all = view(sibs).view(k, depth, d, 2), view(leaf).view(k, d, 2), view(level).view(k, m, C, 2)
    with torch.cuda.stream(ext):
        first[2 * d, :, 0] = 1
    torch.cuda.synchronize()

    def call():
        with torch.cuda.stream(ext):
            whole[:, :, 0, :] = 0
            whole[:, :d, 0, :] = leaf_all
            for j in range(depth):
                lo, hi = 1 + j * C, 1 + (j + 1) * C
                reached, sibling, right = whole[:, :d, lo - 1, :], sib_all[:, j], bits[j][:, None, None]
                first[:d] = torch.where(right, sibling, reached).permute(1, 0, 2)
                first[d:2 * d] = torch.where(right, reached, sibling).permute(1, 0, 2)
                sc._check(lib.sc_rescue_prime_trace_states_dev(states.ptr, k, k, m, rp._params, N, level.ptr, None))
                whole[:, :m, lo:hi, :] = level_all
                whole[:, m:m + d, lo:hi, :] = sibling[:, :, None, :]
                whole[:, m + d, lo:hi, 0] = bits[j][:, None].to(torch.int64)
                whole[:, m + d, lo:hi, 1] = 0
    return call, (sibs, leaf, bits, states, level)


result = {"rounds": args.rounds, "depth": args.depth, "runs": args.runs, "trace": [], "loop": [], "proofs": {}}
depth = args.depth

# ---- (a) the two forms of the trace kernel, and the walk of verify_batch ---------------------------------------------------------------
say("(a) sc_rescue_merkle_path_trace_dev, depth %d, %d rounds: one lane per state register (split) against one lane per item (wide)" % (depth, args.rounds))
for m, capacity, d in SHAPES:
    rp = RescuePrime(m=m, capacity=capacity, rounds=args.rounds)
    W, T = m + d + 1, depth * (args.rounds + 1) + 1
    for k in [int(x) for x in args.counts.split(",")]:
        leaves, idx, paths, indices = inputs(m, d, k, depth)
        outs = {"split": sc.DeviceVector(k * W * T), "wide": sc.DeviceVector(k * W * T)}
        legs = {"split": trace_call(rp, d, depth, k, leaves, idx, paths, outs["split"], INT32_MAX),
                "wide": trace_call(rp, d, depth, k, leaves, idx, paths, outs["wide"], 0)}
        legs["split"](), legs["wide"]()
        sc.synchronize()
        assert same(outs["split"], outs["wide"]), "the two forms disagree"
        if k == 1:
            model = RescueMembership(RescueMerkle(rp, d), depth, 4, 2, 4)
            words = sc.unpack(leaves) , sc.unpack(paths)
            want = model.trace(words[0], indices[0], [words[1][j * d:(j + 1) * d] for j in range(depth)])
            assert sc.unpack(outs["wide"].to_bytes()) == [row[s].value for s in range(W) for row in want], "the kernel and the host model disagree"
        st = alternate({name: timed(call) for name, call in legs.items()}, args.runs)
        faster, spread = verdict(st["split"], st["wide"], "split", "wide")
        entry = {"m": m, "capacity": capacity, "d": d, "k": k, "split": st["split"], "wide": st["wide"], "spread_ms": spread, "faster": faster}
        if k <= 4096:
            roots_b, rows_b = synth.synth_packed(3, k * d).tobytes(), synth.synth_packed(4, k).tobytes()
            vouts = {"split": ctypes.create_string_buffer(k), "wide": ctypes.create_string_buffer(k)}

            def verify_leg(name, key):
                def call():
                    set_split_max_nodes(key)
                    sc._check(lib.sc_rescue_merkle_verify_batch(roots_b, idx, paths, rows_b, k, depth, 1, d, m, rp.rate, rp._params, rp.N, vouts[name]))
                return call
            vst = alternate({"split": timed(verify_leg("split", INT32_MAX)), "wide": timed(verify_leg("wide", 0))}, args.runs)
            entry["verify_split"], entry["verify_wide"] = vst["split"], vst["wide"]
        result["trace"].append(entry)
        say("m=%d c=%d d=%d k=%-5d  split %s   wide %s   spread %.3f ms   faster: %s" % (m, capacity, d, k, show(st["split"]), show(st["wide"]), spread, faster) +
            ("   | verify_batch split %s   wide %s" % (show(entry["verify_split"]), show(entry["verify_wide"])) if k <= 4096 else ""))
        del outs
set_split_max_nodes(-1)

# ---- (b) the kernel against a loop over the existing entry ----------------------------------------------------------------------------
say("(b) the trace kernel (default key) against one sc_rescue_prime_trace_states_dev per level with the rows put in place by torch")
for m, capacity, d in SHAPES[:1]:
    rp = RescuePrime(m=m, capacity=capacity, rounds=args.rounds)
    W, T = m + d + 1, depth * (args.rounds + 1) + 1
    for k in (1, 64, 4096):
        leaves, idx, paths, indices = inputs(m, d, k, depth)
        new_out, loop_out = sc.DeviceVector(k * W * T), sc.DeviceVector(k * W * T)
        new = trace_call(rp, d, depth, k, leaves, idx, paths, new_out, -1)
        loop, keep = level_loop(rp, d, depth, k, leaves, indices, paths, loop_out)
        new(), loop()
        sc.synchronize()
        assert same(new_out, loop_out), "the kernel and the loop disagree"
        st = alternate({"kernel": timed(new), "loop": timed(loop)}, args.runs)
        faster, spread = verdict(st["kernel"], st["loop"], "kernel", "loop")
        result["loop"].append({"m": m, "capacity": capacity, "d": d, "k": k, "kernel": st["kernel"], "loop": st["loop"], "spread_ms": spread, "faster": faster})
        say("m=%d c=%d d=%d k=%-5d  kernel %s   loop %s   loop / kernel x%.2f   spread %.3f ms   faster: %s" %
            (m, capacity, d, k, show(st["kernel"]), show(st["loop"]), st["loop"]["median_ms"] / st["kernel"]["median_ms"], spread, faster))
        del keep

# ---- (c) proofs ----------------------------------------------------------------------------------------------------------------------
m, capacity, d = SHAPES[0]
K = args.batch
say("(c) RescueMembership(m=%d, capacity=%d, d=%d), depth %d, %d rounds, %d colinearity checks: one proof and prove_batch of %d" % (m, capacity, d, depth, args.rounds, args.checks, K))
rp = RescuePrime(m=m, capacity=capacity, rounds=args.rounds)
tree = RescueMerkle(rp, d)
t0 = time.perf_counter()
scheme = RescueMembership(tree, depth, 4, args.checks, 2 * args.checks)
scheme.transition_constraints(), scheme._preprocess()
sc.synchronize()
setup_s = time.perf_counter() - t0
members = []
for t in range(K):
    leaf = synth.synth_ints(900 + t, d)
    path = [synth.synth_ints(1000 + 50 * t + j, d) for j in range(depth)]
    index = (0x9E3779B97F4A7C15 * (t + 1)) % (1 << depth)
    root = [row.value for row in scheme.trace(leaf, index, path)[-1][:d]]
    members.append((root, leaf, index, path))
proof = scheme.prove(*members[0])
t0 = time.perf_counter()
assert scheme.verify(members[0][0], members[0][1], proof) is True, "the proof does not verify"
verify_s = time.perf_counter() - t0
batch = scheme.prove_batch(*[[member[i] for member in members] for i in range(4)])
assert scheme.verify(members[K - 1][0], members[K - 1][1], batch[K - 1]) is True, "a proof of the batch does not verify"
st = alternate({"prove": timed(lambda: scheme.prove(*members[0])),
                "prove_batch": timed(lambda: scheme.prove_batch(*[[member[i] for member in members] for i in range(4)]))}, args.runs)
result["proofs"] = {"m": m, "capacity": capacity, "d": d, "K": K, "checks": args.checks, "trace_rows": scheme.T, "registers": scheme.W,
                    "fri_domain_length": scheme.stark.fri_domain_length, "proof_bytes": len(proof), "setup_s": setup_s, "verify_s": verify_s,
                    "prove": st["prove"], "prove_batch": st["prove_batch"], "per_proof_in_batch_ms": st["prove_batch"]["median_ms"] / K}
say("trace %d rows x %d registers, FRI domain %d, proof %d bytes; columns + constraints + preprocessing once %.2f s; host verify %.2f s" %
    (scheme.T, scheme.W, scheme.stark.fri_domain_length, len(proof), setup_s, verify_s))
say("one proof %s   prove_batch of %d %s   = %.3f ms per proof, x%.2f of a single one" %
    (show(st["prove"]), K, show(st["prove_batch"]), st["prove_batch"]["median_ms"] / K, st["prove"]["median_ms"] * K / st["prove_batch"]["median_ms"]))

os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "membership_timing.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
with open(os.path.join(args.out_dir, "membership_timing.json"), "w") as f:
    json.dump(result, f, indent=1)

#!/usr/bin/env python3
"""The Rescue-Prime Merkle tree on one MI355X (dev tool; method of tools/rescue_wide_timing.py).

usage: rescue_merkle_timing.py [--rounds 27] [--runs 3] [--out-dir profiles/rescue_merkle]

Everything in ONE process on resident operands; both sides of every comparison are compared for equality first, then a warm-up of
every leg and `runs` + `runs` alternating repetitions, wall time from an idle stream to an idle stream.  Median with (min .. max).

(a) sc_rescue_merkle_build_dev against what a caller can do without it: one sc_rescue_prime_sponge_dev per level on a message matrix
    put together in between -- sc_memcpy_dev of the rows into a matrix that already holds the padding rows, and per node level one
    strided torch copy (left and right children apart) on the library stream into a matrix that already holds its padding.  The
    buffers, the padding and the tensor views are made once, outside the timed region.  N = 2^10, 2^14, 2^18, 2^20 at
    (m, capacity, d) = (4, 1, 1) and (3, 1, 1), rows of 4 elements.
(b) the tuning key "rescue_tree_split_max_nodes": per level width w = 2^0 .. 2^18 a tree of 2 w leaves is built with the key at w (the
    level of w nodes one lane per state register) and at w / 2 (one lane per node); everything else in the two builds is the same
    launches, so the difference of the medians is that level's.  The default is the largest w at which the split form's median
    is below the wide form's.
(c) sc_rescue_merkle_verify_batch at k = 1, 64, 4096 and depth 20 in both forms, on paths opened from the tree of (a).
(d) beside every figure the arithmetic floor of its permutations: permutations * (144 m + 2 m^2) * rounds modular products over the
    8.2e11 products/s of DESIGN.md section 3.9."""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stark-anatomy_amd"))
import torch
import starkcore as sc
import synth
from rescue_prime import RescuePrime
from rescue_merkle import RescueMerkle, RescueTree, set_split_max_nodes, INT32_MAX

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=27)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "rescue_merkle"))
ap.add_argument("--log-sizes", default="10,14,18,20")
ap.add_argument("--sweep-max-log", type=int, default=18)
args = ap.parse_args()
sc.init(0)
lib = sc.lib()
PRODUCTS_PER_SECOND = 8.2e11
WIDTH = 4
SHAPES = ((4, 1, 1), (3, 1, 1))
SWEEP_SHAPES = SHAPES + ((8, 1, 1),)               # the widest state too: its split levels take eight lanes per node
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


def spread_ms(st):
    return st["max_ms"] - st["min_ms"]


def floor_ms(permutations, m, rounds):
    return 1e3 * permutations * (144 * m + 2 * m * m) * rounds / PRODUCTS_PER_SECOND


def tree_permutations(n, width, rate, d):
    return n * (width // rate + 1) + (n - 1) * (2 * d // rate + 1)


def view(vec):
    return torch.as_tensor(vec, device="cuda")


def build_call(tree, matrix, n, holder):
    """a build whose tree replaces the one in holder[0] (freed: frees never wait)"""
    def call():
        holder[0] = tree.build_device(matrix, n, WIDTH)
    return call


def level_loop(rp, d, n, matrix):
    """the caller's loop over the existing entries; returns (call, the vector that receives the root)"""
    m, rate, rounds = rp.m, rp.rate, rp.N
    leaf_blocks, node_blocks = WIDTH // rate + 1, 2 * d // rate + 1
    leaf_msg = sc.DeviceVector.zeros(leaf_blocks * rate * n)
    levels = [sc.DeviceVector(d * (n >> j)) for j in range(n.bit_length())]
    msgs, copies = [None], [None]
    sc.synchronize()
    with torch.cuda.stream(ext):
        view(leaf_msg).view(leaf_blocks * rate, n, 2)[WIDTH, :, 0] = 1
        for j in range(1, n.bit_length()):
            half = n >> j
            msg = sc.DeviceVector.zeros(node_blocks * rate * half)
            whole = view(msg).view(node_blocks * rate, half, 2)
            whole[2 * d, :, 0] = 1
            msgs.append(msg)
            # [child, e, k, limb] <- [e, k, child, limb]
            copies.append((whole[:2 * d].view(2, d, half, 2), view(levels[j - 1]).view(d, half, 2, 2).permute(2, 0, 1, 3)))
    torch.cuda.synchronize()

    def call():
        sc._check(lib.sc_memcpy_dev(leaf_msg.ptr, matrix.ptr, WIDTH * n, None))
        sc._check(lib.sc_rescue_prime_sponge_dev(leaf_msg.ptr, n, leaf_blocks, levels[0].ptr, n, d, n, m, rate, rp._params, rounds, None))
        with torch.cuda.stream(ext):
            for j in range(1, n.bit_length()):
                half = n >> j
                dst, src = copies[j]
                dst.copy_(src)
                sc._check(lib.sc_rescue_prime_sponge_dev(msgs[j].ptr, half, node_blocks, levels[j].ptr, half, d, half, m, rate, rp._params, rounds, None))
    return call, levels[-1], (leaf_msg, levels, msgs, copies)


result = {"rounds": args.rounds, "runs": args.runs, "products_per_second": PRODUCTS_PER_SECOND, "build": [], "sweep": {}, "verify": []}
set_split_max_nodes(-1)
deep = {}

# ---- (a) the build against the loop of existing entries -----------------------------------------------------------------------------
say("(a) sc_rescue_merkle_build_dev (default key) against one sc_rescue_prime_sponge_dev per level, rows of %d elements, %d rounds" % (WIDTH, args.rounds))
for m, capacity, d in SHAPES:
    rp = RescuePrime(m=m, capacity=capacity, rounds=args.rounds)
    tree = RescueMerkle(rp, d)
    for log_n in [int(x) for x in args.log_sizes.split(",")]:
        n = 1 << log_n
        matrix = sc.DeviceVector.from_bytes(synth.synth_packed(30 + m, WIDTH * n).tobytes())
        holder = [None]
        new = build_call(tree, matrix, n, holder)
        loop, loop_root, keep = level_loop(rp, d, n, matrix)
        new(), loop()
        assert holder[0].root() == sc.unpack(loop_root.to_bytes()), "the build and the loop disagree"
        words = sc.unpack(matrix.to_bytes(0, 8)) + sc.unpack(matrix.to_bytes(n, 8)) + sc.unpack(matrix.to_bytes(2 * n, 8)) + sc.unpack(matrix.to_bytes(3 * n, 8))
        corner = [[words[8 * j + i] for j in range(WIDTH)] for i in range(8)]               # the first eight rows: the leftmost node of level 3
        level3 = holder[0].level_device(3)
        assert [sc.unpack(level3.to_bytes(e * (n >> 3), 1))[0] for e in range(d)] == tree.commit(corner), "the build and the host model disagree"
        st = alternate({"build_dev": timed(new), "loop": timed(loop)}, args.runs)
        entry = {"m": m, "capacity": capacity, "d": d, "log_n": log_n, "build_dev": st["build_dev"], "loop": st["loop"],
                 "loop_over_build": st["loop"]["median_ms"] / st["build_dev"]["median_ms"],
                 "spread_ms": max(spread_ms(st["build_dev"]), spread_ms(st["loop"])),
                 "floor_ms": floor_ms(tree_permutations(n, WIDTH, rp.rate, d), m, args.rounds)}
        entry["faster_by_more_than_the_spread"] = st["loop"]["median_ms"] - st["build_dev"]["median_ms"] > entry["spread_ms"]
        result["build"].append(entry)
        say("m=%d c=%d d=%d N=2^%-2d  build_dev %s   loop %s   loop / build x%.2f   spread %.3f ms   floor %.3f ms   faster by more than the spread: %s" %
            (m, capacity, d, log_n, show(st["build_dev"]), show(st["loop"]), entry["loop_over_build"], entry["spread_ms"], entry["floor_ms"],
             entry["faster_by_more_than_the_spread"]))
        if log_n == 20:
            deep[(m, capacity, d)] = (holder[0], matrix)
        del keep

# ---- (b) the key's sweep -----------------------------------------------------------------------------------------------------------
say("(b) per level width w: a tree of 2 w leaves with the level of w nodes split (key = w) and wide (key = w / 2); the difference is that level's")
for m, capacity, d in SWEEP_SHAPES:
    rp = RescuePrime(m=m, capacity=capacity, rounds=args.rounds)
    tree = RescueMerkle(rp, d)
    rows, best, clear = [], 0, 0
    for log_w in range(args.sweep_max_log + 1):
        w = 1 << log_w
        n = 2 * w
        matrix = sc.DeviceVector.from_bytes(synth.synth_packed(50 + m, WIDTH * n).tobytes())
        holders = {"split": [None], "wide": [None]}

        def leg(name, key):
            inner = build_call(tree, matrix, n, holders[name])

            def call():
                set_split_max_nodes(key)
                inner()
            return call
        legs = {"split": leg("split", w), "wide": leg("wide", w // 2)}
        legs["split"](), legs["wide"]()
        a, b = holders["split"][0], holders["wide"][0]
        assert a.root() == b.root() and (w > 1 << 10 or a.level(1) == b.level(1)), "the two forms disagree"
        st = alternate({name: timed(call) for name, call in legs.items()}, args.runs)
        level_floor = floor_ms(w * (2 * d // rp.rate + 1), m, args.rounds)
        wins = st["split"]["median_ms"] < st["wide"]["median_ms"]
        tie = abs(st["split"]["median_ms"] - st["wide"]["median_ms"]) <= max(spread_ms(st["split"]), spread_ms(st["wide"]))     # inside the spread: goes to the wide form
        if wins:
            best = w
        if wins and not tie:
            clear = w
        rows.append({"log_w": log_w, "split": st["split"], "wide": st["wide"], "split_minus_wide_ms": st["split"]["median_ms"] - st["wide"]["median_ms"],
                     "level_floor_ms": level_floor, "split_wins": wins, "tie": tie})
        say("m=%d c=%d d=%d w=2^%-2d  split %s   wide %s   split - wide %+9.3f ms   level floor %.4f ms   %s" %
            (m, capacity, d, log_w, show(st["split"]), show(st["wide"]), rows[-1]["split_minus_wide_ms"], level_floor, "tie" if tie else "split" if wins else "wide"))
    result["sweep"]["m=%d,c=%d,d=%d" % (m, capacity, d)] = {"levels": rows, "largest_width_split_wins": best, "largest_width_split_wins_beyond_spread": clear}
    say("m=%d c=%d d=%d: the largest level width at which the split form's median is below the wide form's: %d; by more than the spread of the repetitions: %d" % (m, capacity, d, best, clear))
set_split_max_nodes(-1)

# ---- (c) path verification ---------------------------------------------------------------------------------------------------------
say("(c) sc_rescue_merkle_verify_batch, depth 20, in both forms")
for (m, capacity, d), (built, matrix) in deep.items():
    rp = RescuePrime(m=m, capacity=capacity, rounds=args.rounds)
    n = 1 << 20
    for k in (1, 64, 4096):
        indices = [(7919 * t + 13) % n for t in range(k)]
        paths = built.open_batch(indices)
        root = built.root()
        row_words = [[sc.unpack(matrix.to_bytes(j * n + i, 1))[0] for j in range(WIDTH)] for i in indices[:64]] if k <= 64 else None
        if row_words is None:                         # the rows of many items: whole columns once
            cols = [sc.unpack(matrix.to_bytes(j * n, n)) for j in range(WIDTH)]
            row_words = [[cols[j][i] for j in range(WIDTH)] for i in indices]
            del cols
        roots_b = sc.pack(root * k)
        paths_b = sc.pack([v for p in paths for s in p for v in s])
        rows_b = sc.pack([v for r in row_words for v in r])
        idx = (ctypes.c_uint64 * k)(*indices)
        outs = {"split": ctypes.create_string_buffer(k), "wide": ctypes.create_string_buffer(k)}

        def leg(name, key):
            def call():
                set_split_max_nodes(key)
                sc._check(lib.sc_rescue_merkle_verify_batch(roots_b, idx, paths_b, rows_b, k, 20, WIDTH, d, m, rp.rate, rp._params, rp.N, outs[name]))
            return call
        legs = {"split": leg("split", INT32_MAX), "wide": leg("wide", 0)}
        legs["split"](), legs["wide"]()
        assert outs["split"].raw == outs["wide"].raw == b"\x01" * k, "a path of the tree does not verify"
        st = alternate({name: timed(call) for name, call in legs.items()}, args.runs)
        perms = k * ((WIDTH // rp.rate + 1) + 20 * (2 * d // rp.rate + 1))
        entry = {"m": m, "capacity": capacity, "d": d, "k": k, "depth": 20, "split": st["split"], "wide": st["wide"],
                 "wide_over_split": st["wide"]["median_ms"] / st["split"]["median_ms"], "floor_ms": floor_ms(perms, m, args.rounds)}
        result["verify"].append(entry)
        say("m=%d c=%d d=%d k=%-4d  split %s   wide %s   wide / split x%.2f   floor %.4f ms" %
            (m, capacity, d, k, show(st["split"]), show(st["wide"]), entry["wide_over_split"], entry["floor_ms"]))
set_split_max_nodes(-1)


def readme(result):
    """the README beside the figures: the method, the tables, what the sweep says about the key's default, what was not measured"""
    out = ["# profiles/rescue_merkle", "",
           "Written by `tools/rescue_merkle_timing.py` together with `rescue_merkle_timing.txt` / `.json`: one run at %d rounds, rows of %d" % (result["rounds"], WIDTH),
           "elements, on one MI355X, with the tuning key `rescue_tree_split_max_nodes` at the library's default wherever a leg does not force it.",
           "Everything in one process on resident operands: both sides of every comparison are compared for equality first, then one",
           "warm-up of each leg and %d + %d alternating repetitions, wall time from an idle stream to an idle stream.  Medians.  All" % (result["runs"], result["runs"]),
           "figures are call times: no kernel times by rocprofv3, no hardware counters.  The floor of a figure is its permutations x",
           "(144 m + 2 m^2) x rounds modular products over %.1e products/s (DESIGN.md section 3.9)." % result["products_per_second"], "",
           "## (a) `sc_rescue_merkle_build_dev` against a loop of existing entries", "",
           "The loop is what a caller could do before: one `sc_rescue_prime_sponge_dev` per level on a message matrix put together in",
           "between -- `sc_memcpy_dev` of the rows into a matrix that already holds the padding rows, and per node level one strided torch",
           "copy on the library stream into a matrix that already holds its padding.  The loop's buffers, padding rows and tensor views are",
           "made once, outside the timed region, which favours the loop.  The roots are equal, and the leftmost node of level 3 equals the",
           "host model.", "",
           "| m, capacity, d | N | build_dev | loop | loop / build | spread of the repetitions | floor | faster by more than the spread |", "|---|---|---|---|---|---|---|---|"]
    for e in result["build"]:
        out.append("| %d, %d, %d | 2^%d | %.2f ms | %.2f ms | x%.2f | %.2f ms | %.2f ms | %s |" %
                   (e["m"], e["capacity"], e["d"], e["log_n"], e["build_dev"]["median_ms"], e["loop"]["median_ms"], e["loop_over_build"], e["spread_ms"], e["floor_ms"],
                    "yes" if e["faster_by_more_than_the_spread"] else "NO"))
    slower = [e for e in result["build"] if not e["faster_by_more_than_the_spread"]]
    out += ["", "The new build is faster than the loop at every shape by more than the spread of the repetitions." if not slower else
            "**The new build is NOT faster than the loop by more than the spread at: %s.**" % ", ".join("m = %d, N = 2^%d" % (e["m"], e["log_n"]) for e in slower), "",
            "## (b) the key's sweep", "",
            "Per level width w a tree of 2 w leaves is built with the key at w (the level of w nodes runs one lane per state register) and at",
            "w / 2 (one lane per node); every other launch of the two builds is the same, so the difference of the medians is that level's.",
            "Every width is in the .txt; here the narrow levels' gain and where it ends.", "",
            "| m, capacity, d | split - wide at w = 2^10 | at 2^15 | at 2^16 | at 2^17 | at 2^18 | largest w at which the split form's median is below the wide form's | ... by more than the spread |", "|---|---|---|---|---|---|---|---|"]
    largest = []
    for name, sweep in result["sweep"].items():
        by_log = {row["log_w"]: row for row in sweep["levels"]}
        cell = lambda log_w: "%+.3f ms%s" % (by_log[log_w]["split_minus_wide_ms"], " (tie)" if by_log[log_w]["tie"] else "") if log_w in by_log else "-"
        out.append("| %s | %s | %s | %s | %s | %s | %d | %d |" % (name.replace("m=", "").replace("c=", " ").replace("d=", " "), cell(10), cell(15), cell(16), cell(17), cell(18),
                                                          sweep["largest_width_split_wins"], sweep["largest_width_split_wins_beyond_spread"]))
        largest.append(sweep["largest_width_split_wins_beyond_spread"])
    out += ["", "A difference inside the spread of the repetitions (max - min of either leg) is a tie, and ties go to the wide form: on which side",
            "of zero such a difference falls changes from run to run.  The smallest entry of the last column, **%d**, is the largest level" % min(largest),
            "width at which the split form wins by more than the spread at every state width measured: the value the key's default is taken",
            "from (csrc/rescue_merkle.hip SPLIT_MAX_NODES_DEFAULT).  Widths above the sweep's last were not measured; they run wide.", "",
            "## (c) `sc_rescue_merkle_verify_batch`, depth 20, both forms", "",
            "Paths opened from the tree of 2^20 leaves of (a); all verdicts are 1 in both forms.", "",
            "| m, capacity, d | k | split | wide | wide / split | floor |", "|---|---|---|---|---|---|"]
    for e in result["verify"]:
        out.append("| %d, %d, %d | %d | %.2f ms | %.2f ms | x%.2f | %.4f ms |" % (e["m"], e["capacity"], e["d"], e["k"], e["split"]["median_ms"], e["wide"]["median_ms"],
                                                                              e["wide_over_split"], e["floor_ms"]))
    out += ["", "`kernel_regs.txt` beside this file is `tools/kernel_regs.py rescue_tree` on the cross-compiled code object (VGPRs, SGPRs, scratch and",
            "spills of every instantiation); it is not written by this tool.", "",
            "Not measured: digest lengths above 1, capacities above 1, rows of another width, state widths 5 to 7, level widths above the sweep's",
            "last, builds on several streams at once, `sc_rescue_merkle_open_batch`, kernel times and counters."]
    return "\n".join(out) + "\n"


os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "rescue_merkle_timing.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
with open(os.path.join(args.out_dir, "rescue_merkle_timing.json"), "w") as f:
    json.dump(result, f, indent=1)
with open(os.path.join(args.out_dir, "README.md"), "w") as f:
    f.write(readme(result))

"""The grid of NTT cases the GPU runs under every tuning of the planner (tests/test_gpu_ntt_grid.py), and the route to the planner's
view of it (tests/emu/kernel_cover.cpp: which kernel every launch takes, which cases the planner refuses), which
tests/test_ntt_grid_coverage.py uses to show that the grid reaches every pass kernel.

The tunings are tests/emu/plan_dump.cpp's, plus the launch-only knobs the planner does not see.  A case is a tuple whose first
field is its id (unique within its tuning); expected values never depend on the tuning."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "stark-anatomy_amd", "csrc")
HELPER_SRC = os.path.join(REPO, "tests", "emu", "kernel_cover.cpp")

# include/starkcore.h's defaults of every key a tuning below sets (core.h: Globals, ntt_plan.h: NttTuning)
DEFAULTS = dict(max_tile_log=-1, loge=2, max_col_log=-1, min_tiles_log=8, single_pass_max_log=11, max_digit_log=-1, direct_tw_max_log=22,
                tw_on_load=0, prune=1, loge_cols=3, fixed_shapes=1, wave_local=1, prio_balance=-1, xcd_remap=1)


def _tunings():
    t = [("default", {})]
    for key, vals in (("loge", (1, 3, 4)), ("max_tile_log", (6, 8, 11, 12)), ("max_col_log", (2, 6)), ("min_tiles_log", (0, 10)),
                      ("max_digit_log", (4, 9, 10)), ("single_pass_max_log", (3, 12)), ("prune", (0,)), ("tw_on_load", (1,)), ("loge_cols", (2,))):
        t += [(f"{key}={v}", {key: v}) for v in vals]
    # plan_dump.cpp's combinations: (tile, loge, single, min_tiles, max_col, digit)
    for c in ((4, 1, 2, 0, 2, 8), (6, 2, 3, 0, 2, 4), (12, 2, 11, 8, 4, 10)):
        t.append(("combo=" + ",".join(map(str, c)),
                  dict(zip(("max_tile_log", "loge", "single_pass_max_log", "min_tiles_log", "max_col_log", "max_digit_log"), c))))
    # launch-only knobs
    t += [("fixed_shapes=0", dict(fixed_shapes=0)), ("wave_local=0", dict(wave_local=0)), ("xcd_remap=0", dict(xcd_remap=0))]
    t += [(f"prio_balance={v}", dict(prio_balance=v)) for v in (0, 1, 2)]
    t += [(f"direct_tw_max_log={v}", dict(direct_tw_max_log=v)) for v in (0, 16)]
    return t


TUNINGS = _tunings()
TUNING = dict(TUNINGS)

# ---- sc_ntt_dev: lengths on both sides of every pass-count boundary of the tunings; 2^22 where the digit split changes
NTT_LOGS = (1, 2, 3, 5, 8, 11, 12, 13, 16, 17, 19, 20, 21)
NTT_BIG = ("default", "fixed_shapes=0", "max_digit_log=4", "max_digit_log=9", "max_digit_log=10", "single_pass_max_log=3",
           "single_pass_max_log=12", "combo=4,1,2,0,2,8", "combo=6,2,3,0,2,4", "combo=12,2,11,8,4,10")


def ntt_cases(tuning):
    """(id, logn, root index, inverse): root 0 = primitive_nth_root, 1 = another primitive root"""
    logs = NTT_LOGS + ((22,) if tuning in NTT_BIG else ())
    return [(f"ntt:2^{lg}:root{r}:{'inv' if inv else 'fwd'}", lg, r, inv) for lg in logs for r in (0, 1) for inv in (0, 1)]


# ---- sc_ntt_columns_dev: the fixed8 shapes (17: (9,3),(8,4); 18: (9,3)^2; 19: (10,2),(9,3); 20: (10,2)^2), 2^12, short columns
COLUMN_SHAPES = [(lg, c) for lg in (12, 17, 18, 19, 20) for c in (2, 3, 5)] + [(9, 70)]


def column_cases():
    """(id, logn, cols, inverse, in_place)"""
    return [(f"cols:2^{lg}x{c}:{'inv' if inv else 'fwd'}:{'inplace' if ip else 'outofplace'}", lg, c, inv, ip)
            for lg, c in COLUMN_SHAPES for inv in (0, 1) for ip in (0, 1)]


# ---- sc_coset_evaluate(_columns)_dev: m = n (full), n/2 (zero padding), (n>>5)+1 (pruned first pass), n-5 (odd limit)
COSET_SHAPES = [(12, 3), (17, 3), (19, 2)]


def coset_ms(logn):
    n = 1 << logn
    return (n, n // 2, (n >> 5) + 1, n - 5)


def coset_cases():
    """(id, logn, cols, m, columns_entry): the columns entry reads column c at c * m (the plan's column input stride)"""
    return [(f"coset:2^{lg}x{c}:m={m}:{'columns' if ce else 'single'}", lg, c if ce else 1, m, ce)
            for lg, c in COSET_SHAPES for m in coset_ms(lg) for ce in (1, 0)]


# ---- sc_ntt_batch_dev / sc_ntt_batch_ex_dev / sc_ntt_rows_t_ld_dev
BATCH_SHAPES = [(1, 0), (1, 14), (2, 7), (3, 12), (4, 4), (5, 10), (6, 1), (7, 13), (8, 8), (9, 2), (9, 13), (10, 6), (11, 11), (12, 3),
                (13, 9), (14, 0), (15, 6), (16, 4), (17, 1), (18, 2), (20, 0), (20, 1)]
OUTER_SHAPES = [(3, 5), (6, 4), (8, 2), (9, 3), (10, 6), (12, 4), (13, 1)]
CHUNK_SHAPES = [(3, 4), (6, 6), (9, 5), (12, 2), (16, 1)]
ROWS_LD_SHAPES = [(4, 3, 1), (9, 4, 2), (12, 2, 4), (16, 0, 8)]        # (loglen, logbatch, chunks)


def batch_cases():
    """(id, kind, loglen, logbatch): plain batched transforms, kind 0 [len][batch] columns, kind 1 [batch][len] rows -> [len][batch]"""
    return [(f"batch{k}:2^{ll}x2^{lb}", k, ll, lb) for ll, lb in BATCH_SHAPES for k in (0, 1)]


def outer_cases():
    """(id, loglen, logbatch, col_base, order, ninv): kind 0 with the outer twiddle w_order^(r * (col_base + c)) [* order^-1]"""
    out = []
    for ll, lb in OUTER_SHAPES:
        b, nb = 1 << lb, 1 << (ll + lb)
        for base, order in ((0, nb), (0, 2 * nb), (3 * b, 4 * nb)):
            for ninv in (0, 1):
                out.append((f"outer:2^{ll}x2^{lb}:base={base}:order={order}:ninv={ninv}", ll, lb, base, order, ninv))
    return out


def chunk_cases():
    """(id, loglen, logbatch, chunks): kind 1 reading [chunks][batch][len / chunks]"""
    return [(f"chunks:2^{ll}x2^{lb}:chunks={c}", ll, lb, c) for ll, lb in CHUNK_SHAPES for c in (2, 4, 8) if c <= (1 << ll)]


def rows_ld_cases():
    """(id, loglen, logbatch, chunks, out_ld, col0): kind 1 into columns [col0, col0 + batch) of a [len][out_ld] output"""
    return [(f"rows_ld:2^{ll}x2^{lb}:chunks={c}:ld={3 << lb}", ll, lb, c, 3 << lb, 1 << lb) for ll, lb, c in ROWS_LD_SHAPES]


# ---- the sharded transform's stages (tests/test_gpu_sharded.py: _simulate, fused): (log2n, world, blocks, defer, diag_in_place,
# log_n1; 0 = the library's split).  The column stage with the rank's own block written into its receive buffer is the only route to
# the second-destination (ALT) instantiations of the four-element kernels; 2^20 on one rank gives 2^8 / 2^9-point columns in batches
# of 2^12 / 2^11, the (8,4) and (9,3) tiles.
SHARDED = [(16, 4, 2, True, True, 0), (10, 2, 1, False, False, 0), (12, 2, 1, True, True, 0), (14, 4, 1, True, True, 0),
           (18, 2, 1, True, True, 0), (20, 8, 2, True, True, 0), (20, 1, 1, True, True, 0), (20, 1, 1, True, True, 9)]


def sharded_cases():
    return [(f"sharded:2^{lg}:world={w}:blocks={b}:{'defer' if d else 'nodefer'}:{'diag' if dg else 'nodiag'}:n1=2^{l1 or 'default'}",
             lg, w, b, d, dg, l1) for lg, w, b, d, dg, l1 in SHARDED]


def _sharded_plans(case):
    """the batched calls (kernel_cover 'batch' directives, without their id) of one sharded transform, forward and inverse:
    fourstep.hip fourstep_cols / fourstep_rows / fourstep_rows_finish for the first and the last rank"""
    _, lg, world, blocks, defer, diag, log1 = case
    log1 = log1 or ((lg + 1) // 2 if lg <= 16 else 8)      # sc_fourstep_create_ex's default split
    lw = world.bit_length() - 1
    out = []
    for dirn, (lr, lc) in enumerate(((log1, lg - log1), (lg - log1, log1))):
        rw, cw = 1 << (lr - lw), 1 << (lc - lw)
        for rank in (0, world - 1):
            dl, dn = (rank * rw, rw) if diag else (0, 0)
            out.append(f"0 {lr} {lc - lw} 1 {dirn} 0 0 0 {dl} {dn} 0 4")
        K = blocks if rw % blocks == 0 else 1
        rk = rw // K
        split = defer and K > 1
        out.append(f"1 {lc} {rk.bit_length() - 1} 0 0 {lw} {rw * cw} {rw} 0 0 0 {1 if split else 4}")
        if split:
            out.append(f"1 {lc} {rw.bit_length() - 1} 0 0 0 0 0 0 0 1 2")
    return out


NOLIMIT = (1 << 64) - 1


def helper_input(tuning):
    """kernel_cover's directives for every case of one tuning; the ids are the cases' ids (sharded: id/stage number)"""
    lines = ["tune " + tuning + "".join(f" {k}={v}" for k, v in TUNING[tuning].items())]
    for cid, lg, _, inv in ntt_cases(tuning):
        lines.append(f"ntt {cid} {lg} 1 {NOLIMIT} 0 {inv} 0")
    for cid, lg, c, inv, _ in column_cases():
        lines.append(f"ntt {cid} {lg} {c} {NOLIMIT} 0 {inv} 0")
    for cid, lg, c, m, ce in coset_cases():
        lines.append(f"ntt {cid} {lg} {c} {m} 1 0 {m if ce else 0}")
    for cid, k, ll, lb in batch_cases():
        lines.append(f"batch {cid} {k} {ll} {lb} 0 0 0 0 0 0 0 0 4")
    for cid, ll, lb, _, _, ninv in outer_cases():
        lines.append(f"batch {cid} 0 {ll} {lb} 1 {ninv} 0 0 0 0 0 0 4")
    for cid, ll, lb, c in chunk_cases():
        lines.append(f"batch {cid} 1 {ll} {lb} 0 0 {c.bit_length() - 1} 0 0 0 0 0 4")
    for cid, ll, lb, c, ld, _ in rows_ld_cases():
        lines.append(f"batch {cid} 1 {ll} {lb} 0 0 {c.bit_length() - 1} 0 {ld} 0 0 0 4")
    for case in sharded_cases():
        lines += [f"batch {case[0]}/{i} {s}" for i, s in enumerate(_sharded_plans(case))]
    return lines


def build_helper(outdir):
    exe = os.path.join(outdir, "kernel_cover")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe, HELPER_SRC])
    return exe


def run_helper(exe, lines):
    return subprocess.run([exe], input="\n".join(lines) + "\n", check=True, stdout=subprocess.PIPE, text=True).stdout


def plan_grid(exe, tunings=None):
    """{tuning: {case id: [kernel@prio, ...] or None (the planner refuses the case)}}"""
    out = {}
    for name in tunings or TUNING:
        res = {}
        for line in run_helper(exe, helper_input(name)).splitlines():
            cid, *ks = line.split()
            res[cid] = None if ks == ["unsupported"] else ks
        out[name] = res
    return out

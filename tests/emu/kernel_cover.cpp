// Which pass kernel every launch of a case of the GPU test grid (tests/ntt_grid.py) takes: the library's planner (csrc/ntt_plan.h)
// plans each case as core.hip / fourstep.hip call it, and csrc's pass_kernel / pass_prio_balance -- the functions launch_pass and
// run_plan use -- pick the instantiation and the priority schedule.  tests/test_ntt_grid_coverage.py builds it and checks that
// the grid reaches every kernel; tests/test_gpu_ntt_grid.py asks it which cases the planner refuses.
//
// stdin, one directive per line:
//   tune <name> key=value ...          the tuning of the following cases (sc_set_tuning keys; unknown keys are launch-only)
//   ntt <id> <logn> <cols> <in_limit> <coset> <inverse> <col_stride_in>
//   batch <id> <kind> <loglen> <logbatch> <outer> <outer_ninv> <chunks_log> <chunk_stride> <out_ld> <diag_lo> <diag_n> <pass_lo> <pass_hi>
//   nofit                              the smallest sc_ntt_columns_dev over the tunings so far whose plan has an eight-element shape
//                                      that the launch keeps off its kernel because the lane offsets could reach 4 GiB
// stdout: "<id> unsupported", or "<id>" followed by one "<kernel>@p<prio_balance>" per launched pass, where <kernel> is
// fixed4<LR,LC,TRACE,ALT>, fixed8<LR,LC>, generic<LOGE>, or generic<3>:nofit for a fixed8 shape that fixed_offsets_fit refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "ntt_plan.h"

using namespace sc;

namespace {

const int NUM_CUS = 256;        // MI355X; only the automatic prio_balance rule reads it
Fe sentinel[16][2];             // distinct non-null pointers for the tables and buffers (never dereferenced)
Fe* S(int i) { return sentinel[i]; }

struct Tune {
    NttTuning t;
    int fixed_shapes = 1, prio_balance = -1;
};

bool set_key(Tune& tu, const std::string& k, int v) {
    NttTuning& t = tu.t;
    if (k == "max_tile_log") t.max_tile_log = v;
    else if (k == "loge") t.loge = v;
    else if (k == "max_col_log") t.max_col_log = v;
    else if (k == "min_tiles_log") t.min_tiles_log = v;
    else if (k == "single_pass_max_log") t.single_pass_max_log = v;
    else if (k == "max_digit_log") t.max_digit_log = v;
    else if (k == "direct_tw_max_log") t.direct_tw_max_log = v;
    else if (k == "tw_on_load") t.tw_on_load = v;
    else if (k == "prune") t.prune = v;
    else if (k == "loge_cols") t.loge_cols = v;
    else if (k == "fixed_shapes") tu.fixed_shapes = v;
    else if (k == "prio_balance") tu.prio_balance = v;
    else return false;          // xcd_remap, wave_local: no say in the plan or the kernel
    return true;
}

std::string kernels(const NttPlanDesc& d, const Tune& tu, int pass_lo = 0, int pass_hi = 4) {
    std::string s;
    for (int i = pass_lo; i < d.npasses && i < pass_hi; ++i) {
        NttPassDesc pd = d.pass[i];
        pd.p.prio_balance = pass_prio_balance(pd, tu.prio_balance, NUM_CUS);
        pd.p.trace = nullptr;
        const PassKernel k = pass_kernel(pd, tu.fixed_shapes != 0);
        char b[64];
        if (k.kind == PK_FIXED4) snprintf(b, sizeof b, " fixed4<%d,%d,%d,%d>", pd.p.logR, pd.p.logC, k.trace ? 1 : 0, k.alt ? 1 : 0);
        else if (k.kind == PK_FIXED8) snprintf(b, sizeof b, " fixed8<%d,%d>", pd.p.logR, pd.p.logC);
        else snprintf(b, sizeof b, " generic<%d>%s", pd.loge,
                      tu.fixed_shapes && pd.loge == 3 && !pd.p.blk_enable && fixed8_shape(pd.p.logR, pd.p.logC) && !fixed_offsets_fit(pd.p) ? ":nofit" : "");
        s += b;
        s += "@p" + std::to_string(pd.p.prio_balance);
    }
    return s;
}

// core.hip ntt_device: plan, then replan with the direct inter-pass tables no larger than 2^direct_tw_max_log entries
bool plan_ntt_call(NttPlanDesc& d, const Tune& tu, int logn, uint32_t cols, uint64_t in_limit, bool coset, bool inverse, uint64_t csi) {
    const int m = plan_num_passes(logn, tu.t);
    NttTables tb;
    tb.mt = S(0); tb.mt_log = logn < 12 ? logn : 12; tb.tl = S(1); tb.th = S(2);
    tb.th_scaled = (inverse && m > 1) ? S(3) : nullptr;
    NttIo io;
    io.in = S(4); io.out = S(5); io.work = m > 1 ? S(6) : nullptr;
    io.in_limit = in_limit; io.cols = cols; io.col_stride_in = csi;
    if (coset) { io.ol = S(7); io.oh = S(8); }
    if (inverse && m == 1) { io.scale_last = true; io.scale = Fe{1, 0}; }
    if (!plan_ntt(d, logn, tb, io, tu.t)) return false;
    if (d.npasses > 1) {
        bool any = false;
        for (int i = 0; i + 1 < d.npasses; ++i) {
            const DirectTable t = direct_table(d, i, inverse);
            if (t.logR + t.logB <= tu.t.direct_tw_max_log) { tb.twd[i] = S(9 + i); any = true; }
        }
        if (any && !plan_ntt(d, logn, tb, io, tu.t)) return false;
    }
    return true;
}

// fourstep.hip batch_call / plan_batched_direct
bool plan_batch_call(NttPlanDesc& d, const Tune& tu, int kind, int loglen, int logbatch, bool outer, bool outer_ninv, int chunks_log,
                     uint64_t chunk_stride, uint64_t out_ld, uint32_t diag_lo, uint32_t diag_n) {
    NttTables tb;
    tb.mt = S(0); tb.mt_log = loglen < 12 ? loglen : 12; tb.tl = S(1); tb.th = S(2);
    BatchExtras ex;
    ex.chunks_log = chunks_log;
    ex.chunk_stride = chunk_stride;
    ex.out_ld = out_ld;
    if (diag_n) { ex.diag_out = S(13); ex.diag_lo = diag_lo; ex.diag_n = diag_n; }
    if (outer) {
        ex.outer_tl = S(14);
        ex.outer_th = outer_ninv ? S(15) : S(14);
        if (tu.t.direct_tw_max_log > 0 && loglen + logbatch <= tu.t.direct_tw_max_log) ex.outer_twd = S(12);
    }
    const BatchKind bk = kind == 0 ? BATCH_COLS : BATCH_ROWS_T;
    if (!plan_batched(d, bk, loglen, logbatch, tb, S(4), S(6), S(5), tu.t, ex)) return false;
    if (d.npasses != 2) return true;
    const DirectTable t = direct_table(d, 0, false);
    if (t.logR + t.logB > tu.t.direct_tw_max_log) return true;
    ex.inner_twd = S(11);
    return plan_batched(d, bk, loglen, logbatch, tb, S(4), S(6), S(5), tu.t, ex);
}

}  // namespace

int main() {
    std::vector<std::pair<std::string, Tune>> seen;
    Tune tu;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what, id;
        in >> what;
        if (what == "tune") {
            tu = Tune();
            std::string name, kv;
            in >> name;
            while (in >> kv) {
                const size_t eq = kv.find('=');
                set_key(tu, kv.substr(0, eq), atoi(kv.c_str() + eq + 1));
            }
            seen.push_back({name, tu});
        } else if (what == "ntt") {
            int logn, coset, inverse;
            uint64_t cols, limit, csi;
            in >> id >> logn >> cols >> limit >> coset >> inverse >> csi;
            NttPlanDesc d;
            const bool ok = plan_ntt_call(d, tu, logn, (uint32_t)cols, limit, coset != 0, inverse != 0, csi);
            printf("%s%s\n", id.c_str(), ok ? kernels(d, tu).c_str() : " unsupported");
        } else if (what == "batch") {
            int kind, loglen, logbatch, outer, ninv, chunks_log, pass_lo, pass_hi;
            uint64_t chunk_stride, out_ld;
            uint32_t diag_lo, diag_n;
            in >> id >> kind >> loglen >> logbatch >> outer >> ninv >> chunks_log >> chunk_stride >> out_ld >> diag_lo >> diag_n >> pass_lo >> pass_hi;
            NttPlanDesc d;
            const bool ok = plan_batch_call(d, tu, kind, loglen, logbatch, outer != 0, ninv != 0, chunks_log, chunk_stride, out_ld, diag_lo, diag_n);
            printf("%s%s\n", id.c_str(), ok ? kernels(d, tu, pass_lo, pass_hi).c_str() : " unsupported");
        } else if (what == "nofit") {
            // columns of every power-of-two count, forward and inverse, full, zero-padded and pruned inputs: the fewest elements
            double best = 0;
            std::string where = "none";
            for (size_t ti = 0; ti < seen.size(); ++ti)
                for (int logn = 1; logn <= 32; ++logn)
                    for (int lc = 0; lc <= 16; ++lc)
                        for (int inv = 0; inv < 2; ++inv)
                            for (int li = 0; li < 3; ++li) {
                                const uint64_t n = 1ull << logn, lim = li == 0 ? ~0ull : li == 1 ? n / 2 : (n >> 5) + 1;
                                NttPlanDesc d;
                                if (!plan_ntt_call(d, seen[ti].second, logn, 1u << lc, lim, li == 2, inv != 0, 0)) continue;
                                if (kernels(d, seen[ti].second).find(":nofit") == std::string::npos) continue;
                                const double elems = (double)n * (double)(1u << lc);
                                if (best == 0 || elems < best) {
                                    best = elems;
                                    where = seen[ti].first + " logn=" + std::to_string(logn) + " cols=" + std::to_string(1u << lc) +
                                            " inverse=" + std::to_string(inv) + " limit=" + std::to_string(li);
                                }
                            }
            printf("nofit %s elements=%.0f\n", where.c_str(), best);
        }
    }
    return 0;
}

// Canonical dump of the NTT planner's output (csrc/ntt_plan.h) over a fixed grid of transforms, tunings and extras.
// tests/test_ntt_plans.py builds it against the tree's csrc/ and compares each case's SHA-256 with tests/golden/ntt_plans.json,
// which tests/golden/make_ntt_plans.py writes by building the same file against another csrc/ (-I picks the planner).
// Output: one "case <tuning> <logn>" line per tuning and length, followed by the dump of every plan of that case (plan_ntt of 2^logn,
// both kinds of plan_batched of length 2^logn up to 2^20); fields are printed by name and pointers as the name of the sentinel
// buffer they point at, so neither struct padding nor addresses enter the dump.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "ntt_plan.h"

using namespace sc;

namespace {

enum Sentinel { S_IN, S_WORK, S_OUT, S_MT, S_TL, S_TH, S_THS, S_TWD0, S_TWD1, S_TWD2, S_TWD3, S_OL, S_OH, S_OTL, S_OTH, S_OTWD,
                S_ITWD, S_DIAG, S_BLK0, S_COUNT = S_BLK0 + 32 };
const char* const NAMES[S_BLK0] = {"in", "work", "out", "mt", "tl", "th", "th_scaled", "twd0", "twd1", "twd2", "twd3", "ol", "oh",
                                   "outer_tl", "outer_th", "outer_twd", "inner_twd", "diag_out"};
Fe sentinel[S_COUNT][2];

Fe* S(int i) { return sentinel[i]; }

std::string name(const void* p) {
    if (!p) return "null";
    for (int i = 0; i < S_COUNT; ++i)
        if (p == (const void*)sentinel[i]) return i < S_BLK0 ? NAMES[i] : "blk" + std::to_string(i - S_BLK0);
    return "?";
}

std::string out;
void put(const char* k, uint64_t v) { out += ' '; out += k; out += '='; out += std::to_string(v); }
void put(const char* k, int v) { out += ' '; out += k; out += '='; out += std::to_string(v); }
void put(const char* k, uint32_t v) { put(k, (uint64_t)v); }
void put(const char* k, const void* p) { out += ' '; out += k; out += '='; out += name(p); }
void put(const char* k, Fe v) { out += ' '; out += k; out += '='; out += std::to_string(v.lo) + ':' + std::to_string(v.hi); }

void dump(bool ok, const NttPlanDesc& d, const std::string& what) {
    out += what;
    if (!ok) { out += " unsupported\n"; return; }
    put("logn", d.logn); put("npasses", d.npasses);
    for (int i = 0; i < 4; ++i) put("digit", d.digits[i]);
    out += '\n';
    for (int i = 0; i < d.npasses; ++i) {
        const NttPassDesc& pd = d.pass[i];
        const PassParams& p = pd.p;
        out += " pass"; put("loge", pd.loge); put("ntiles", pd.ntiles); put("cols", pd.cols); put("threads", pd.threads); put("lds_bytes", pd.lds_bytes);
        put("in", p.in); put("out", p.out); put("logR", p.logR); put("logC", p.logC); put("lo_log", p.lo_log); put("mid_log", p.mid_log);
        put("in_hi", p.in_hi); put("in_mid", p.in_mid); put("in_lo", p.in_lo); put("in_rs", p.in_rs); put("in_cs", p.in_cs);
        put("in_split", p.in_split); put("in_rs_hi", p.in_rs_hi);
        put("out_hi", p.out_hi); put("out_mid", p.out_mid); put("out_lo", p.out_lo); put("out_rs", p.out_rs); put("out_cs", p.out_cs);
        put("rfast_load", p.rfast_load); put("mt", p.mt); put("mt_shift", p.mt_shift);
        put("tw_enable", p.tw_enable); put("tw_col_shift", p.tw_col_shift); put("tw_scale", p.tw_scale);
        put("tw_col_base", p.tw_col_base); put("tw_row_k", p.tw_row_k); put("tw_row_mid", p.tw_row_mid); put("tl", p.tl); put("th", p.th);
        put("twd", p.twd); put("twd_stride", p.twd_stride); put("twd_in", p.twd_in); put("twd_in_mask", p.twd_in_mask);
        put("scale_enable", p.scale_enable); put("scale", p.scale); put("in_limit", p.in_limit); put("coset_enable", p.coset_enable);
        put("ol", p.ol); put("oh", p.oh); put("prune_log", p.prune_log); put("prio_balance", p.prio_balance);
        put("blk_enable", p.blk_enable); put("blk_log", p.blk_log); put("blk_row_k", p.blk_row_k); put("blk_row_mid", p.blk_row_mid);
        for (int h = 0; h < SC_MAX_BLOCKS; ++h) put("out_blk", (const void*)p.out_blk[h]);
        put("col_enable", p.col_enable); put("col_tiles_log", p.col_tiles_log); put("col_stride", p.col_stride); put("col_stride_in", p.col_stride_in);
        put("trace", (const void*)p.trace);
        out += '\n';
    }
}

struct Tuning { const char* name; NttTuning t; };

std::vector<Tuning> tunings() {
    std::vector<Tuning> v;
    auto add = [&](std::string nm, NttTuning t) { v.push_back({strdup(nm.c_str()), t}); };
    add("default", NttTuning());
    auto key = [&](const char* k, int NttTuning::*f, std::initializer_list<int> vals) {
        for (int x : vals) { NttTuning t; t.*f = x; add(std::string(k) + "=" + std::to_string(x), t); }
    };
    key("loge", &NttTuning::loge, {1, 3, 4});
    key("max_tile_log", &NttTuning::max_tile_log, {6, 8, 11, 12});
    key("max_col_log", &NttTuning::max_col_log, {2, 6});
    key("min_tiles_log", &NttTuning::min_tiles_log, {0, 10});
    key("max_digit_log", &NttTuning::max_digit_log, {4, 9, 10});
    key("single_pass_max_log", &NttTuning::single_pass_max_log, {3, 12});
    key("prune", &NttTuning::prune, {0});
    key("tw_on_load", &NttTuning::tw_on_load, {1});
    key("loge_cols", &NttTuning::loge_cols, {2});
    // combinations the emulator tests use to force many-pass plans at small sizes: (tile, loge, single, min_tiles, max_col, digit)
    const int combos[][6] = {{4, 1, 2, 0, 2, 8}, {6, 2, 3, 0, 2, 4}, {12, 2, 11, 8, 4, 10}};
    for (const auto& c : combos) {
        NttTuning t;
        t.max_tile_log = c[0]; t.loge = c[1]; t.single_pass_max_log = c[2]; t.min_tiles_log = c[3]; t.max_col_log = c[4]; t.max_digit_log = c[5];
        add("combo=" + std::to_string(c[0]) + "," + std::to_string(c[1]) + "," + std::to_string(c[2]) + "," + std::to_string(c[3]) + "," +
            std::to_string(c[4]) + "," + std::to_string(c[5]), t);
    }
    return v;
}

void case_ntt(const NttTuning& tu, int logn) {
    const uint64_t n = 1ull << logn;
    const uint32_t cols_list[] = {1, 2, 64, 4096, 65536};
    const uint64_t limits[] = {~0ull, n / 2, (n >> 5) + 1};
    for (uint32_t cols : cols_list)
        for (int li = 0; li < 3; ++li)
            for (int scaled = 0; scaled < 2; ++scaled)
                for (int direct = 0; direct < 2; ++direct)
                    for (int csi = 0; csi < (cols > 1 ? 2 : 1); ++csi) {
                        NttTables tb;
                        tb.mt = S(S_MT); tb.mt_log = logn < 12 ? logn : 12; tb.tl = S(S_TL); tb.th = S(S_TH);
                        if (scaled) tb.th_scaled = S(S_THS);
                        if (direct) for (int i = 0; i < 4; ++i) tb.twd[i] = S(S_TWD0 + i);
                        NttIo io;
                        io.in = S(S_IN); io.work = S(S_WORK); io.out = S(S_OUT);
                        io.in_limit = limits[li];
                        if (li == 2) { io.ol = S(S_OL); io.oh = S(S_OH); }
                        io.scale_last = scaled != 0;
                        io.scale = Fe{12345, 678};
                        io.cols = cols;
                        if (csi) io.col_stride_in = n / 2 + 3;
                        NttPlanDesc d;
                        const bool ok = plan_ntt(d, logn, tb, io, tu);
                        dump(ok, d, "ntt cols=" + std::to_string(cols) + " limit=" + std::to_string(li) + " scaled=" + std::to_string(scaled) +
                                    " direct=" + std::to_string(direct) + " csi=" + std::to_string(csi));
                    }
}

void case_batched(const NttTuning& tu, BatchKind kind, int loglen) {
    const uint64_t len = 1ull << loglen;
    NttTables tb;
    tb.mt = S(S_MT); tb.mt_log = loglen < 12 ? loglen : 12; tb.tl = S(S_TL); tb.th = S(S_TH);
    static Fe* blk[32];
    for (int h = 0; h < 32; ++h) blk[h] = S(S_BLK0 + h);
    for (int logbatch = 0; logbatch <= 14; ++logbatch) {
        const uint64_t batch = 1ull << logbatch;
        std::vector<std::pair<std::string, BatchExtras>> xs;
        BatchExtras plain;
        xs.push_back({"plain", plain});
        BatchExtras x = plain; x.inner_twd = S(S_ITWD); xs.push_back({"inner", x});
        if (kind == BATCH_COLS) {
            BatchExtras o = plain; o.outer_tl = S(S_OTL); o.outer_th = S(S_OTH); o.outer_col_base = 3 * batch;
            xs.push_back({"outer", o});
            x = o; x.outer_twd = S(S_OTWD); xs.push_back({"outer_twd", x});
            x.inner_twd = S(S_ITWD); xs.push_back({"outer_twd_inner", x});
            const uint32_t q = (uint32_t)(len >> 2 ? len >> 2 : 1);
            x = plain; x.diag_out = S(S_DIAG); x.diag_lo = q; x.diag_n = q; xs.push_back({"diag", x});
            x.diag_lo = 1; xs.push_back({"diag_unaligned", x});
            x = o; x.outer_twd = S(S_OTWD); x.inner_twd = S(S_ITWD); x.block_out = blk; x.block_rows = (uint32_t)(len >> 3 ? len >> 3 : 1);
            xs.push_back({"block", x});
            x.block_rows = (uint32_t)(len >> 5 ? len >> 5 : 1); xs.push_back({"block_many", x});
            x.block_rows = 3; xs.push_back({"block_odd", x});
        } else {
            for (int cl = 1; cl <= 3; ++cl)
                for (int stride = 0; stride < 2; ++stride) {
                    x = plain; x.chunks_log = cl; x.chunk_stride = stride ? (len >> cl) * batch * 4 : 0;
                    xs.push_back({"chunks=" + std::to_string(cl) + (stride ? " stride" : ""), x});
                }
            x = plain; x.chunks_log = 1; x.inner_twd = S(S_ITWD); xs.push_back({"chunks=1 inner", x});
            x = plain; x.out_ld = batch * 4; xs.push_back({"out_ld", x});
            x.chunks_log = 2; x.chunk_stride = (len >> 2) * batch * 8; x.inner_twd = S(S_ITWD); xs.push_back({"out_ld chunks=2 stride inner", x});
        }
        for (const auto& e : xs) {
            NttPlanDesc d;
            const bool ok = plan_batched(d, kind, loglen, logbatch, tb, S(S_IN), S(S_WORK), S(S_OUT), tu, e.second);
            dump(ok, d, std::string(kind == BATCH_COLS ? "batch_cols" : "batch_rows_t") + " logbatch=" + std::to_string(logbatch) + " " + e.first);
        }
    }
}

void emit(const std::string& name) {
    fputs("case ", stdout);
    fputs(name.c_str(), stdout);
    fputc('\n', stdout);
    fwrite(out.data(), 1, out.size(), stdout);
    out.clear();
}

}  // namespace

int main() {
    static char buf[1 << 20];
    setvbuf(stdout, buf, _IOFBF, sizeof buf);
    for (const Tuning& t : tunings())
        for (int logn = 1; logn <= 32; ++logn) {
            case_ntt(t.t, logn);
            if (logn <= 20) { case_batched(t.t, BATCH_COLS, logn); case_batched(t.t, BATCH_ROWS_T, logn); }
            emit(std::string(t.name) + " " + std::to_string(logn));
        }
    return 0;
}

// CPU side of the top-limb field corrections (csrc/field.cuh: fe_add_fast / fe_sub_fast / mont_mul_fast) and of the FAST rounds of
// the eight-element tile kernels (csrc/ntt_tile.cuh): the portable twins of the device forms against the exact forms, and one tile
// of a planned pass through the FAST and the exact round bodies.  Test infrastructure (built by tests/test_fast_fixups_emu.py).
#include "ntt_emu.cpp"

// op 0: a + b, 1: a - b (a, b canonical); 2: mont_mul(a, b) (a any 128-bit value, b canonical).
// out: fast result, exact result (2 limbs each); returns the flag of the fast form.
extern "C" int fast_field_one(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    const Fe x{a[0], a[1]}, y{b[0], b[1]};
    rare_t rare = 0;
    Fe f, e;
    if (op == 0) { f = fe_add_fast(x, y, rare); e = fe_add_c(x, y); }
    else if (op == 1) { f = fe_sub_fast(x, y, rare); e = fe_sub_c(x, y); }
    else { f = mont_mul_fast(x, y, rare); e = mont_mul_c(x, y); }
    out[0] = f.lo; out[1] = f.hi; out[2] = e.lo; out[3] = e.hi;
    return rare != 0;
}

// every pair (a[i], b[j]): counts[0] = pairs, [1] = flagged, [2] = unflagged and different from the exact result (must be 0),
// [3] = flagged and different (the results the redo exists for)
extern "C" void fast_field_pairs(int op, const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb, uint64_t* counts) {
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (uint64_t i = 0; i < na; ++i)
        for (uint64_t j = 0; j < nb; ++j) {
            uint64_t out[4];
            const int flag = fast_field_one(op, a + 2 * i, b + 2 * j, out);
            const bool same = out[0] == out[2] && out[1] == out[3];
            ++counts[0];
            counts[1] += flag;
            counts[2] += !flag && !same;
            counts[3] += flag && !same;
        }
}

template <int GLR, int GLC, bool FAST, int ROUND = 0>
static void run_tile_rounds(const NttPassDesc& pd, uint32_t tile, Fe* lds, const Fe* tw, rare_t& rare) {
    using FR = FixedRounds<3, GLR, GLC, ROUND>;
    for (uint32_t tid = 0; tid < pd.threads; ++tid) ntt_round<3, FR::S, GLR, GLC, FAST>(pd.p, FR::SH, ROUND == 0, tile, tid, lds, tw, &rare);
    if constexpr (ROUND + 1 < FR::NR) run_tile_rounds<GLR, GLC, FAST, ROUND + 1>(pd, tile, lds, tw, rare);
}

template <bool FAST>
static bool run_tile(const NttPassDesc& pd, uint32_t tile, rare_t& rare) {
    const PassParams& P = pd.p;
    std::vector<Fe> lds(pd.lds_bytes / sizeof(Fe));
    Fe* tw = lds.data() + ((size_t)1 << (P.logR + P.logC));
    for (uint32_t tid = 0; tid < pd.threads; ++tid) tile_twiddles_to_lds(P, P.logR, tid, pd.threads, tw);
#define RUN_TILE(LR, LC) if (P.logR == LR && P.logC == LC) { run_tile_rounds<LR, LC, FAST>(pd, tile, lds.data(), tw, rare); return true; }
    SC_FIXED8_SHAPES(RUN_TILE)
#undef RUN_TILE
    return false;
}

// Tile 0 of pass `pass` of the forward transform of `cols` columns of length 2^logn, as the library plans it (direct four-step table at the
// store): `in` is that pass's input buffer [cols][n]; out_fast / out_exact ([cols][n], zeroed by the caller) receive the tile's outputs
// from the FAST and from the exact rounds.  Returns logR * 100 + logC of the pass (negative: not an eight-element pass);
// *rare_out = the FAST rounds' flag.
extern "C" int fast_tile(int logn, int cols, int pass, const uint64_t* in, uint64_t* out_fast, uint64_t* out_exact, const uint64_t* root, uint64_t* rare_out) {
    const uint64_t n = 1ull << logn;
    const Fe r_m = to_mont(Fe{root[0], root[1]});
    NttTuning tu;
    const RootTables rt(r_m, logn);
    NttTables tb = rt.tb;
    std::vector<Fe> work(n * cols);
    NttIo io;
    io.in = (const Fe*)in; io.work = work.data(); io.out = (Fe*)out_exact;
    io.cols = (uint32_t)cols;
    NttPlanDesc d;
    if (!plan_ntt(d, logn, tb, io, tu)) return -1;
    std::vector<Fe> twd[4];
    for (int i = 0; i + 1 < d.npasses; ++i) {
        fill_direct(twd[i], d, i, false, rt);
        tb.twd[i] = twd[i].data();
    }
    if (!plan_ntt(d, logn, tb, io, tu)) return -1;
    if (pass >= d.npasses) return -2;
    if (d.pass[pass].loge != 3) return -4 - d.pass[pass].loge;
    if (!fast_pass_ok(d.pass[pass].p)) return -3;
    NttPassDesc pd = d.pass[pass];
    pd.p.in = (const Fe*)in;
    rare_t rare = 0, none = 0;
    pd.p.out = (Fe*)out_fast;
    if (!run_tile<true>(pd, 0, rare)) return -3;
    pd.p.out = (Fe*)out_exact;
    if (!run_tile<false>(pd, 0, none)) return -3;
    *rare_out = rare;
    return pd.p.logR * 100 + pd.p.logC;
}

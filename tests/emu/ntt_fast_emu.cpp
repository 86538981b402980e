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

// ---- whole passes, single tiles and single rounds of a planned column transform through the FAST and the exact round bodies, with
// the flag kept per wave and per round (tests/fast_fixups_cases.py builds inputs that flag chosen tiles with these).

// grid index -> tile of the eight-element kernels' launch (core.hip: fixed8_tile and launch_pass's remap condition): keep in step
static uint32_t grid_tile(const NttPassDesc& pd, uint32_t index, int xcd_remap) {
    const PassParams& P = pd.p;
    const bool remap = xcd_remap && pd.ntiles >= 16 && (pd.ntiles & 7u) == 0;
    uint32_t wg = index, colbits = 0;
    if (P.col_enable) { colbits = (wg >> P.col_tiles_log) << P.col_tiles_log; wg -= colbits; }
    uint32_t tile = wg;
    if (remap) tile = (wg & 7u) * (pd.ntiles >> 3) + (wg >> 3);
    return tile | colbits;
}

// the plan of emu_ntt_columns (direct four-step tables at the store, th * n^-1 for an inverse) with its tables kept alive; the
// passes' in / out pointers are set per call
struct FxPlan {
    int logn, cols;
    uint64_t n;
    RootTables* rt = nullptr;
    std::vector<Fe> twd[4];
    NttPlanDesc d;
    bool fast[4] = {false, false, false, false};          // launch_pass: the pass takes ntt_pass_kernel_fixed8, then the redo of marked tiles
    bool fixed8[4] = {false, false, false, false};
    bool ok = false;
    FxPlan(int logn_, int cols_, const uint64_t* root, int inverse) : logn(logn_), cols(cols_), n(1ull << logn_) {
        Fe r_m = to_mont(Fe{root[0], root[1]});
        Fe scale_m = fe_mont_one();
        if (inverse) {
            r_m = mont_pow(r_m, n - 1);
            scale_m = mont_inv(to_mont(Fe{n, 0}));
        }
        NttTuning tu;
        const int m = plan_num_passes(logn, tu);
        rt = new RootTables(r_m, logn, scale_m);
        NttTables tb = rt->tb;
        tb.th_scaled = (inverse && m > 1) ? rt->ths.data() : nullptr;
        // three distinct buffers, as sc_ntt_columns_dev has them out of place (never dereferenced here: only pass_in_place looks)
        Fe* const base = reinterpret_cast<Fe*>((uintptr_t)1 << 40);
        NttIo io;
        io.in = base; io.work = base + 2 * n * cols; io.out = base + 4 * n * cols;
        io.cols = (uint32_t)cols;
        io.scale_last = inverse && m == 1;
        io.scale = scale_m;
        if (!plan_ntt(d, logn, tb, io, tu)) return;
        if (d.npasses > 1) {
            for (int i = 0; i + 1 < d.npasses; ++i) {
                fill_direct(twd[i], d, i, tb.th_scaled != nullptr, *rt);
                tb.twd[i] = twd[i].data();
            }
            if (!plan_ntt(d, logn, tb, io, tu)) return;
        }
        for (int i = 0; i < d.npasses; ++i) {
            fixed8[i] = pass_kernel(d.pass[i], true).kind == PK_FIXED8;
            fast[i] = fixed8[i] && fast_pass_ok(d.pass[i].p) && !pass_in_place(d.pass[i]);
        }
        ok = true;
    }
    ~FxPlan() { delete rt; }
    NttPassDesc pass(int i, const uint64_t* in, uint64_t* out) const {
        NttPassDesc pd = d.pass[i];
        pd.p.in = (const Fe*)in;
        pd.p.out = (Fe*)out;
        return pd;
    }
};

extern "C" void* fx_open(int logn, int cols, const uint64_t* root, int inverse) {
    FxPlan* h = new FxPlan(logn, cols, root, inverse);
    if (!h->ok) { delete h; return nullptr; }
    return h;
}
extern "C" void fx_close(void* h) { delete (FxPlan*)h; }
// info[0] = passes; per pass i, info[1 + 8 i ..]: logR, logC, loge, tiles per column, threads, rounds, eight-element kernel, FAST
extern "C" void fx_info(void* hv, int* info) {
    const FxPlan& h = *(FxPlan*)hv;
    info[0] = h.d.npasses;
    for (int i = 0; i < h.d.npasses; ++i) {
        const NttPassDesc& pd = h.d.pass[i];
        int* o = info + 1 + 8 * i;
        o[0] = pd.p.logR; o[1] = pd.p.logC; o[2] = pd.loge; o[3] = (int)pd.ntiles; o[4] = (int)pd.threads;
        o[5] = (pd.p.logR + pd.loge - 1) / pd.loge; o[6] = h.fixed8[i]; o[7] = h.fast[i];
    }
}
extern "C" uint32_t fx_grid_tile(void* hv, int pass, uint32_t index, int xcd_remap) { return grid_tile(((FxPlan*)hv)->d.pass[pass], index, xcd_remap); }

// rounds [r0, r1) of one tile, one lane at a time; word: bits 0-7 = the waves (tid >> 6) with a flagged lane, bits 8-15 = 1 + the first
// round that flagged (0: none).  The last round stores to P.out.
template <int GLR, int GLC, bool FAST, int ROUND = 0>
static void fx_rounds(const NttPassDesc& pd, uint32_t tile, Fe* lds, const Fe* tw, int r0, int r1, uint32_t& word) {
    using FR = FixedRounds<3, GLR, GLC, ROUND>;
    if (ROUND >= r0 && ROUND < r1) {
        for (uint32_t tid = 0; tid < pd.threads; ++tid) {
            rare_t rare = 0;
            ntt_round<3, FR::S, GLR, GLC, FAST>(pd.p, FR::SH, ROUND == 0, tile, tid, lds, tw, &rare);
            if (rare) {
                word |= 1u << (tid >> 6);
                if (!(word >> 8)) word |= (uint32_t)(ROUND + 1) << 8;
            }
        }
    }
    if constexpr (ROUND + 1 < FR::NR) fx_rounds<GLR, GLC, FAST, ROUND + 1>(pd, tile, lds, tw, r0, r1, word);
}
template <bool FAST>
static bool fx_tile_run(const NttPassDesc& pd, uint32_t tile, Fe* lds, int r0, int r1, uint32_t& word) {
    const PassParams& P = pd.p;
    Fe* tw = lds + ((size_t)1 << (P.logR + P.logC));
#define FX_TILE(LR, LC) if (P.logR == LR && P.logC == LC) { fx_rounds<LR, LC, FAST>(pd, tile, lds, tw, r0, r1, word); return true; }
    SC_FIXED8_SHAPES(FX_TILE)
#undef FX_TILE
    return false;
}
static std::vector<Fe> fx_lds(const NttPassDesc& pd) {
    std::vector<Fe> lds(pd.lds_bytes / sizeof(Fe));
    Fe* tw = lds.data() + ((size_t)1 << (pd.p.logR + pd.p.logC));
    for (uint32_t tid = 0; tid < pd.threads; ++tid) tile_twiddles_to_lds(pd.p, pd.p.logR, tid, pd.threads, tw);
    return lds;
}

// Every tile of pass `pass`: `in` is the pass's input [cols][n]; out_exact / out_fast ([cols][n], either may be null) get the outputs of
// the exact and of the FAST rounds; words[grid index] (null or one per workgroup, grid as launch_pass lays it out under xcd_remap) as
// fx_rounds builds them.  Returns 1 where the pass is one the library runs FAST, 0 where it runs exact only (out_fast and words are
// then left alone), negative on error.
extern "C" int fx_pass(void* hv, int pass, int xcd_remap, const uint64_t* in, uint64_t* out_fast, uint64_t* out_exact, uint32_t* words) {
    const FxPlan& h = *(FxPlan*)hv;
    if (pass < 0 || pass >= h.d.npasses) return -2;
    if (out_exact) {
        const NttPassDesc pd = h.pass(pass, in, out_exact);
        NttPlanDesc one = h.d;
        one.pass[pass] = pd;
        if (run_plan(one, pass, pass + 1) < 0) return -3;
    }
    if (!h.fast[pass]) return 0;
    if (out_fast) {
        const NttPassDesc pd = h.pass(pass, in, out_fast);
        std::vector<Fe> lds = fx_lds(pd);
        for (uint32_t wg = 0; wg < pd.ntiles * pd.cols; ++wg) {
            uint32_t word = 0;
            if (!fx_tile_run<true>(pd, grid_tile(pd, wg, xcd_remap), lds.data(), 0, 16, word)) return -3;
            if (words) words[wg] = word;
        }
    }
    return 1;
}

// Rounds [r0, r1) of one tile of an eight-element pass, FAST or exact.  r0 = 0 reads the tile's slice of `in` ([cols][n]); r0 >= 1 starts
// from `state`, the tile's LDS image (2^12 elements) at the input of round r0.  A run that ends before the last round leaves the LDS image
// at the input of round r1 in `state`; one that includes it stores the tile's outputs into `out` ([cols][n], the rest untouched).
// *word as fx_rounds builds it.  Returns the pass's number of rounds.
extern "C" int fx_tile(void* hv, int pass, uint32_t tile, int r0, int r1, int fast, const uint64_t* in, uint64_t* state, uint64_t* out, uint32_t* word) {
    const FxPlan& h = *(FxPlan*)hv;
    if (pass < 0 || pass >= h.d.npasses || !h.fixed8[pass]) return -2;
    const NttPassDesc pd = h.pass(pass, in, out);
    if (tile >= pd.ntiles * pd.cols) return -2;
    const int nr = (pd.p.logR + 2) / 3;
    if (r0 < 0 || r0 >= r1 || r1 > nr || (r0 == 0 && !in) || ((r0 > 0 || r1 < nr) && !state) || (r1 == nr && !out)) return -2;
    std::vector<Fe> lds = fx_lds(pd);
    const size_t tile_elems = (size_t)1 << (pd.p.logR + pd.p.logC);
    if (r0 > 0) memcpy(lds.data(), state, tile_elems * sizeof(Fe));
    uint32_t w = 0;
    const bool ran = fast ? fx_tile_run<true>(pd, tile, lds.data(), r0, r1, w) : fx_tile_run<false>(pd, tile, lds.data(), r0, r1, w);
    if (!ran) return -3;
    if (r1 < nr) memcpy(state, lds.data(), tile_elems * sizeof(Fe));
    if (word) *word = w;
    return nr;
}

// Where the lanes of a tile take their elements from in round `round`, by the kernels' own Round: pos[tid * 8 + i] = the index of
// x[i] of thread tid -- in the pass's input [cols][n] for round 0, in the tile's LDS image for a later round.
template <int GLR, int GLC, int ROUND = 0>
static void fx_map_rounds(const NttPassDesc& pd, uint32_t tile, int round, uint64_t* pos) {
    using FR = FixedRounds<3, GLR, GLC, ROUND>;
    if (ROUND == round) {
        for (uint32_t tid = 0; tid < pd.threads; ++tid) {
            Round<3, FR::S, GLR, GLC> R;
            R.setup(pd.p, ROUND == 0, tile, tid);
            for (int i = 0; i < 8; ++i)
                pos[tid * 8 + i] = ROUND == 0 ? R.col_off_in + R.in_index(pd.p, i, FR::SH) : lds_index(R.row(i, FR::SH), R.cc[i >> FR::S], GLC);
        }
        return;
    }
    if constexpr (ROUND + 1 < FR::NR) fx_map_rounds<GLR, GLC, ROUND + 1>(pd, tile, round, pos);
}
extern "C" int fx_tile_map(void* hv, int pass, uint32_t tile, int round, uint64_t* pos) {
    const FxPlan& h = *(FxPlan*)hv;
    if (pass < 0 || pass >= h.d.npasses || !h.fixed8[pass]) return -2;
    const NttPassDesc pd = h.pass(pass, nullptr, nullptr);
    if (tile >= pd.ntiles * pd.cols || round < 0 || round >= (pd.p.logR + 2) / 3) return -2;
#define FX_MAP(LR, LC) if (pd.p.logR == LR && pd.p.logC == LC) { fx_map_rounds<LR, LC>(pd, tile, round, pos); return 0; }
    SC_FIXED8_SHAPES(FX_MAP)
#undef FX_MAP
    return -3;
}

// The store side of a tile: pos[tid * 8 + i] = where thread tid stores its element i in the pass's output [cols][n] (found by storing
// numbered elements through scatter_global into `scratch`, [cols][n], all zero before and after), twd[tid * 8 + i] = the direct-table
// entry that element is multiplied by (Montgomery form; only where the return value has bit 0), scale = P.scale (bit 1), and
// twimg = the tile's LDS twiddle image (2^(logR-1) entries).  Returns bit 0: direct table at the store, bit 1: final scale,
// bit 2: a two-level four-step twiddle at the store (no table; twd is left alone).
template <int GLR, int GLC>
static void fx_store_map(const NttPassDesc& pd, uint32_t tile, Fe* scratch, uint64_t count, uint64_t* pos, Fe* twd) {
    using FR = FixedRounds<3, GLR, GLC, (GLR + 2) / 3 - 1>;
    static_assert(FR::SH == 0, "last round");
    NttPassDesc plain = pd;
    plain.p.tw_enable = 0; plain.p.scale_enable = 0; plain.p.out = scratch;
    for (uint32_t tid = 0; tid < pd.threads; ++tid) {
        Round<3, FR::S, GLR, GLC> R;
        R.setup(pd.p, false, tile, tid);
        Fe x[8];
        for (int i = 0; i < 8; ++i) x[i] = Fe{(uint64_t)tid * 8 + i + 1, 0};
        R.scatter_global(plain.p, x);
        if (pd.p.tw_enable && pd.p.twd) R.load_twd(pd.p, twd + tid * 8);
    }
    for (uint64_t j = 0; j < count; ++j)
        if (scratch[j].lo) { pos[scratch[j].lo - 1] = j; scratch[j] = fe_zero(); }
}
extern "C" int fx_tile_store(void* hv, int pass, uint32_t tile, uint64_t* scratch, uint64_t* pos, uint64_t* twd, uint64_t* scale, uint64_t* twimg) {
    const FxPlan& h = *(FxPlan*)hv;
    if (pass < 0 || pass >= h.d.npasses || !h.fixed8[pass]) return -2;
    const NttPassDesc pd = h.pass(pass, nullptr, nullptr);
    if (tile >= pd.ntiles * pd.cols) return -2;
    tile_twiddles_to_lds(pd.p, pd.p.logR, 0, 1, (Fe*)twimg);
    scale[0] = pd.p.scale.lo; scale[1] = pd.p.scale.hi;
    const int kind = (pd.p.tw_enable && pd.p.twd ? 1 : 0) | (pd.p.scale_enable ? 2 : 0) | (pd.p.tw_enable && !pd.p.twd ? 4 : 0);
#define FX_STORE(LR, LC) if (pd.p.logR == LR && pd.p.logC == LC) { fx_store_map<LR, LC>(pd, tile, (Fe*)scratch, h.n * h.cols, pos, (Fe*)twd); return kind; }
    SC_FIXED8_SHAPES(FX_STORE)
#undef FX_STORE
    return -3;
}

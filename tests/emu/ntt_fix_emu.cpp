// CPU side of the self-repairing top-limb field corrections (csrc/field.cuh: fe_add_fix / fe_sub_fix / mont_mul_fix) and of the
// ARITH_FIX rounds of the eight-element tile kernels (csrc/ntt_tile.cuh): the portable twins against the exact forms -- no flag, no
// pair left out -- and single tiles of a planned pass through the ARITH_FIX and the exact round bodies.  Everything of
// ntt_fast_emu.cpp is in here too (the fx_* plan handles are shared).  Test infrastructure (built by tests/test_inline_repair_emu.py).
#include "ntt_fast_emu.cpp"

// op 0: a + b, 1: a - b (a, b canonical); 2: mont_mul(a, b) (a any 128-bit value, b canonical).
// out: self-repairing result, exact result (2 limbs each); returns the flag the fast twin raises on the same operands.
extern "C" int fix_field_one(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    const Fe x{a[0], a[1]}, y{b[0], b[1]};
    rare_t rare = 0;
    Fe f, e;
    if (op == 0) { f = fe_add_fix(x, y); e = fe_add_c(x, y); (void)fe_add_fast(x, y, rare); }
    else if (op == 1) { f = fe_sub_fix(x, y); e = fe_sub_c(x, y); (void)fe_sub_fast(x, y, rare); }
    else { f = mont_mul_fix(x, y); e = mont_mul_c(x, y); (void)mont_mul_fast(x, y, rare); }
    out[0] = f.lo; out[1] = f.hi; out[2] = e.lo; out[3] = e.hi;
    return rare != 0;
}

static void fix_count(int op, const uint64_t* a, const uint64_t* b, uint64_t* counts) {
    uint64_t out[4];
    const int flag = fix_field_one(op, a, b, out);
    const bool same = out[0] == out[2] && out[1] == out[3];
    ++counts[0];
    counts[1] += !same;
    counts[2] += flag;
}
// counts[0] = pairs, [1] = results that differ from the exact form (must be 0), [2] = pairs on which the fast twin flags (the
// repairs taken).  crossed = 1: every pair (a[i], b[j]); 0: the pairs (a[i], b[i]), na == nb.
extern "C" void fix_field_pairs(int op, int crossed, const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb, uint64_t* counts) {
    counts[0] = counts[1] = counts[2] = 0;
    if (crossed) {
        for (uint64_t i = 0; i < na; ++i)
            for (uint64_t j = 0; j < nb; ++j) fix_count(op, a + 2 * i, b + 2 * j, counts);
    } else {
        for (uint64_t i = 0; i < na && i < nb; ++i) fix_count(op, a + 2 * i, b + 2 * i, counts);
    }
}

// the paired dispatchers (portable: one member after the other) on (a, b) in slot 0 and (c, d) in slot 1; op 0: mont_mul2_fix
// (out: r0, r1), op 1: fe_addsub2_fix (out: s0, d0, s1, d1)
extern "C" void fix_field_two(int op, const uint64_t* a, const uint64_t* b, const uint64_t* c, const uint64_t* d, uint64_t* out) {
    const Fe x{a[0], a[1]}, y{b[0], b[1]}, z{c[0], c[1]}, w{d[0], d[1]};
    Fe r[4] = {fe_zero(), fe_zero(), fe_zero(), fe_zero()};
    if (op == 0) mont_mul2_fix(x, y, z, w, r[0], r[1]);
    else fe_addsub2_fix(x, y, z, w, r[0], r[1], r[2], r[3]);
    for (int k = 0; k < 4; ++k) { out[2 * k] = r[k].lo; out[2 * k + 1] = r[k].hi; }
}

template <int GLR, int GLC, int ARITH, int ROUND = 0>
static void fix_rounds(const NttPassDesc& pd, uint32_t tile, Fe* lds, const Fe* tw, rare_t& rare) {
    using FR = FixedRounds<3, GLR, GLC, ROUND>;
    for (uint32_t tid = 0; tid < pd.threads; ++tid) ntt_round<3, FR::S, GLR, GLC, ARITH>(pd.p, FR::SH, ROUND == 0, tile, tid, lds, tw, &rare);
    if constexpr (ROUND + 1 < FR::NR) fix_rounds<GLR, GLC, ARITH, ROUND + 1>(pd, tile, lds, tw, rare);
}
template <int ARITH>
static bool fix_tile_run(const NttPassDesc& pd, uint32_t tile, rare_t& rare) {
    std::vector<Fe> lds = fx_lds(pd);
    Fe* tw = lds.data() + ((size_t)1 << (pd.p.logR + pd.p.logC));
#define FIX_TILE(LR, LC) if (pd.p.logR == LR && pd.p.logC == LC) { fix_rounds<LR, LC, ARITH>(pd, tile, lds.data(), tw, rare); return true; }
    SC_FIXED8_SHAPES(FIX_TILE)
#undef FIX_TILE
    return false;
}

// Tile `tile` of pass `pass` of an fx_open plan, all rounds: `in` is the pass's input [cols][n]; out_fix / out_exact ([cols][n], zeroed
// by the caller) receive the tile's outputs from the ARITH_FIX and from the exact rounds.  *fast_flag = whether the ARITH_FAST rounds
// flag on this tile (their output goes nowhere), *fix_rare = what the ARITH_FIX rounds left in their (unused) accumulator: 0.
// Returns logR * 100 + logC.
extern "C" int fix_tile(void* hv, int pass, uint32_t tile, const uint64_t* in, uint64_t* out_fix, uint64_t* out_exact, uint64_t* scratch,
                        uint64_t* fast_flag, uint64_t* fix_rare) {
    const FxPlan& h = *(FxPlan*)hv;
    if (pass < 0 || pass >= h.d.npasses || !h.fixed8[pass] || !fast_pass_ok(h.d.pass[pass].p)) return -2;
    if (tile >= h.d.pass[pass].ntiles * h.d.pass[pass].cols) return -2;
    rare_t rare_fix = 0, rare_fast = 0, none = 0;
    if (!fix_tile_run<ARITH_FIX>(h.pass(pass, in, out_fix), tile, rare_fix)) return -3;
    if (!fix_tile_run<ARITH_EXACT>(h.pass(pass, in, out_exact), tile, none)) return -3;
    if (!fix_tile_run<ARITH_FAST>(h.pass(pass, in, scratch), tile, rare_fast)) return -3;
    *fast_flag = rare_fast;
    *fix_rare = rare_fix;
    return h.d.pass[pass].p.logR * 100 + h.d.pass[pass].p.logC;
}

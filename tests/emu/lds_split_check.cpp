// The eight-element kernels' LDS addressing (csrc/ntt_tile.cuh, Round::lds_index_split: lane index ^ compile-time swizzle bits +
// compile-time offset) against the per-element form (lds_index(row(i, sh), cc[g], logC)) that the generic and the emulated paths
// use: every shape of SC_FIXED8_SHAPES, every round, both splits of the thread index in the first round, every thread, every element.
// Also: the host forms of scatter_lds_split / gather_lds_split move the same elements as scatter_lds / gather_lds, and the
// compile-time parts stay inside what one ds_read_b128 / ds_write_b128 can address (a 16-bit byte offset).
// Prints one line per shape and round; exit status 0 when everything agrees.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../stark-anatomy_amd/csrc/ntt_plan.h"

using namespace sc;

static int failures = 0;

template <int GLR, int GLC, int ROUND>
static void check_round() {
    using FR = FixedRounds<3, GLR, GLC, ROUND>;
    using Rd = Round<3, FR::S, GLR, GLC>;
    static_assert(Rd::SPLIT_ADDR, "eight-element geometry-specialised round");
    constexpr int SH = FR::SH, E = 8;
    const uint32_t threads = 1u << (GLR + GLC - 3), elems = 1u << (GLR + GLC);
    for (int rfast = 0; rfast <= (ROUND == 0 ? 1 : 0); ++rfast) {
        PassParams P;
        memset(&P, 0, sizeof P);
        P.logR = GLR; P.logC = GLC; P.rfast_load = rfast;
        std::vector<int> seen(elems, 0);
        std::vector<Fe> tile_a(elems), tile_b(elems);
        uint32_t bad = 0, distinct_low = 0, max_off = 0;
        for (uint32_t tid = 0; tid < threads; ++tid) {
            Rd R;
            R.setup(P, ROUND == 0, 0, tid);
            const uint32_t lane = R.lds_lane(SH);
            Fe x[E], y[E];
            uint32_t lows = 0;
            for (int i = 0; i < E; ++i) {
                const uint32_t want = lds_index(R.row(i, SH), R.cc[i >> FR::S], GLC);
                const uint32_t got = rfast ? Rd::template lds_index_split<true>(lane, i, SH) : Rd::template lds_index_split<false>(lane, i, SH);
                const uint32_t low = rfast ? Rd::template lds_low<true>(i, SH) : Rd::template lds_low<false>(i, SH);
                const uint32_t off = rfast ? Rd::template lds_off<true>(i, SH) : Rd::template lds_off<false>(i, SH);
                bad += want != got || want >= elems;
                if (want < elems) seen[want]++;
                lows |= 1u << low;
                if (off > max_off) max_off = off;
                x[i] = Fe{(uint64_t)tid * E + i, 0x5a5au + tid};
            }
            distinct_low = __builtin_popcount(lows);
            R.scatter_lds(SH, x, tile_a.data());
            if (rfast) R.template scatter_lds_split<true>(SH, x, tile_b.data()); else R.template scatter_lds_split<false>(SH, x, tile_b.data());
            if (rfast) R.template gather_lds_split<true>(SH, y, tile_a.data()); else R.template gather_lds_split<false>(SH, y, tile_a.data());
            for (int i = 0; i < E; ++i) bad += y[i].lo != x[i].lo || y[i].hi != x[i].hi;
        }
        for (uint32_t e = 0; e < elems; ++e) bad += seen[e] != 1 || tile_a[e].lo != tile_b[e].lo || tile_a[e].hi != tile_b[e].hi;
        // the largest compile-time byte offset plus a lane address stays inside the tile, and is a legal DS offset
        const bool fits = ((uint64_t)max_off << 4) < 65536;
        printf("fixed8<%d,%d> round %d (S %d, sh %d) rfast %d: %u mismatches, %u lane bases, max offset %u bytes%s\n", GLR, GLC, ROUND, FR::S, SH, rfast,
               bad, distinct_low, max_off << 4, fits ? "" : " (does not fit 16 bits)");
        failures += bad != 0 || !fits;
    }
    if constexpr (ROUND + 1 < FR::NR) check_round<GLR, GLC, ROUND + 1>();
}

int main() {
#define SC_CHECK(LR, LC) check_round<LR, LC, 0>();
    SC_FIXED8_SHAPES(SC_CHECK)
#undef SC_CHECK
    return failures ? 1 : 0;
}

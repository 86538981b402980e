// CPU walk of the column kernels: the SAME per-thread bodies the HIP kernels run (csrc/columns.cuh), compiled by g++ with the portable
// field arithmetic and called once per (workgroup, thread) of the grid the library would launch.  Test infrastructure (built by
// tests/test_columns_emu.py).
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../stark-anatomy_amd/csrc/columns.cuh"

using namespace sc;

extern "C" {

// pointwise_div_cols_kernel over its whole grid: (position blocks) x (column chunks), 256 threads each
void emu_div_cols(const void* a, uint64_t ld_a, const void* b, uint64_t ld_b, void* out, uint64_t ld_out, uint64_t n, uint64_t cols, uint32_t chunk, uint32_t* zero) {
    const DivCols D{(const Fe*)a, ld_a, (const Fe*)b, ld_b, (Fe*)out, ld_out, n, cols, chunk, zero};
    const uint32_t gx = div_cols_grid_x(n), gy = (uint32_t)((cols + chunk - 1) / chunk);
    for (uint32_t y = 0; y < gy; ++y)
        for (uint32_t x = 0; x < gx; ++x)
            for (uint32_t t = 0; t < COLS_WG; ++t) div_cols_thread<DIV_COLS_K>(D, x, y, t, gx);
}

// columns_verdict_kernel: 64 lanes, then lane 0's merge; rem may be null (the pointwise form)
void emu_verdict(const uint32_t* zero, const long long* rem, uint64_t cols, uint64_t words[4]) {
    long long firsts[64];
    uint64_t counts[64];
    for (uint32_t lane = 0; lane < 64; ++lane) verdict_lane(zero, rem, cols, lane, &firsts[lane], &counts[lane]);
    verdict_words(zero, rem, firsts, counts, words);
}

// combine_cols_kernel: one thread per element of [0, n_out) of every column (the last workgroup's spare threads write nothing);
// srcs / lds / ns / shifts: the term table; weights: canonical [cols][nterms], converted like the entry does
void emu_combine_cols(const void* const* srcs, const uint64_t* lds, const uint64_t* ns, const uint64_t* shifts, uint32_t nterms, const void* weights, uint64_t cols,
                      void* out, uint64_t n_out, uint64_t ld_out) {
    std::vector<CombineTerm> terms(nterms);
    for (uint32_t t = 0; t < nterms; ++t) terms[t] = CombineTerm{(const Fe*)srcs[t], lds[t], ns[t], shifts[t]};
    std::vector<Fe> w(cols * nterms);
    for (uint64_t k = 0; k < cols * nterms; ++k) w[k] = to_mont(((const Fe*)weights)[k]);
    const uint64_t gx = (n_out + COLS_WG - 1) / COLS_WG;
    for (uint64_t c = 0; c < cols; ++c)
        for (uint64_t x = 0; x < gx; ++x)
            for (uint32_t t = 0; t < COLS_WG; ++t) {
                const uint64_t i = x * COLS_WG + t;
                if (i < n_out) ((Fe*)out)[c * ld_out + i] = combine_cols_elem(terms.data(), nterms, w.data(), c, i);
            }
}

// unscale_cols_kernel: grid (position blocks) x (columns); the wave's report is the highest of its lanes' (here: every lane's)
void emu_unscale_cols(const void* full, uint64_t order, void* out, uint64_t ld_out, const uint64_t* n_out, uint64_t cols, const void* base, long long* rem) {
    // the two-level table of `base` (canonical), Montgomery form: lo[j] = base^j, j < 4096; hi[j] = base^(4096 j)
    const Fe b_m = to_mont(*(const Fe*)base);
    std::vector<Fe> lo(4096), hi((order >> 12) + 1);
    for (uint64_t j = 0; j < 4096; ++j) lo[j] = mont_pow(b_m, j);
    for (uint64_t j = 0; j < hi.size(); ++j) hi[j] = mont_pow(b_m, 4096 * j);
    const UnscaleCols U{(const Fe*)full, order, (Fe*)out, ld_out, n_out, lo.data(), hi.data(), rem};
    const uint64_t gx = (order + COLS_WG - 1) / COLS_WG;
    for (uint64_t c = 0; c < cols; ++c)
        for (uint64_t x = 0; x < gx; ++x)
            for (uint32_t t = 0; t < COLS_WG; ++t) {
                const long long r = unscale_cols_thread(U, c, x * COLS_WG + t);
                if (r >= 0) cols_word_max(rem + c, r);
            }
}
}

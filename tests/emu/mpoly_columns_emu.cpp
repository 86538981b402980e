// CPU walk of mpoly_eval_columns_kernel: the plan the library builds (csrc/mpoly_plan.h) and the SAME per-thread body the HIP kernel
// runs (csrc/columns.cuh), compiled by g++ with the portable field arithmetic and called once per (workgroup, thread) of the grids the
// entry would launch.  Test infrastructure (built by tests/test_mpoly_columns_emu.py).
#include <cstdint>
#include <vector>
#include "../../stark-anatomy_amd/csrc/mpoly_plan.h"

using namespace sc;

extern "C" {

// sc_mpoly_eval_columns_dev on host memory.  rows: pairs (member, constraint) per launch -- COLS_GRID_ROWS in the library, lower here so
// that small cases go through several launches.  Per constraint: products[c] / flat[c] = products per point of the plan / of the
// term-by-term evaluation, horner[c] = the Horner variable.  0: done; 1: a bad argument; 2: turned variables over a count that is no
// power of two (nothing is written then)
int emu_mpoly_eval_columns(const void* vals, uint64_t nvars, uint64_t n, uint64_t members, const uint64_t* var_base, const uint64_t* var_ld, const uint32_t* var_src,
                           const uint64_t* var_rot, uint64_t ncons, const uint64_t* nterms, const uint8_t* exps, const void* coefs, void* out, uint64_t ld_out,
                           uint32_t rows, uint64_t* products, uint64_t* flat, uint32_t* horner) {
    MpolyPlan P;
    if (mpoly_plan_build((uint32_t)nvars, ncons, nterms, exps, (const Fe*)coefs, P)) return 1;
    std::vector<MpolyVar> vars;
    const char* what = nullptr;
    if (const int bad = mpoly_vars_resolve((uint32_t)nvars, n, var_base, var_ld, var_src, var_rot, P.used, vars, &what)) return bad;
    for (uint64_t c = 0; c < ncons; ++c) {
        products[c] = P.products[c];
        flat[c] = P.products_flat[c];
        horner[c] = P.cons[c].h;
    }
    const uint64_t pairs = members * ncons;
    const uint32_t gx = (uint32_t)((n + COLS_WG - 1) / COLS_WG);
    for (uint64_t pair0 = 0; pair0 < pairs; pair0 += rows) {
        const uint32_t gy = (uint32_t)(pairs - pair0 < rows ? pairs - pair0 : rows);
        const MpolyCols D{(const Fe*)vals, vars.data(), P.cons.data(), P.coef.data(), P.drop.data(), P.exps.data(), P.nvw, (uint32_t)ncons, n, (Fe*)out, ld_out, (uint32_t)pair0};
        for (uint32_t y = 0; y < gy; ++y)
            for (uint32_t x = 0; x < gx; ++x)
                for (uint32_t t = 0; t < COLS_WG; ++t) mpoly_cols_thread(D, x, y, t);
    }
    return 0;
}

// scale_cols_kernel over its grid: (position blocks) x (columns); base: the factor, canonical
void emu_scale_cols(const void* in, uint64_t ld_in, void* out, uint64_t ld_out, uint64_t n, uint64_t cols, const void* base) {
    // the two-level table of `base`, Montgomery form: lo[j] = base^j, j < 4096; hi[j] = base^(4096 j)
    const Fe b_m = to_mont(*(const Fe*)base);
    std::vector<Fe> lo(4096), hi((n >> 12) + 1);
    for (uint64_t j = 0; j < 4096; ++j) lo[j] = mont_pow(b_m, j);
    for (uint64_t j = 0; j < hi.size(); ++j) hi[j] = mont_pow(b_m, 4096 * j);
    const uint64_t gx = (n + COLS_WG - 1) / COLS_WG;
    for (uint64_t c = 0; c < cols; ++c)
        for (uint64_t x = 0; x < gx; ++x)
            for (uint32_t t = 0; t < COLS_WG; ++t) scale_cols_thread((const Fe*)in, ld_in, (Fe*)out, ld_out, n, lo.data(), hi.data(), c, x * COLS_WG + t);
}
}

// CPU walk of sc_stark_combination_batch: the checks and tables the library's entry builds (csrc/combination_plan.h, csrc/mpoly_plan.h)
// and the SAME per-thread bodies the HIP kernels run (csrc/combination.cuh, csrc/columns.cuh), compiled by g++ with the portable field
// arithmetic and called once per (workgroup, thread) of the grids the entry launches, chunk by chunk.  Test infrastructure: a shared
// object for tests/test_combination_emu.py, and with -DCOMBINATION_EMU_MAIN a stand-alone program (for sanitizer builds) that reads
// one call from a file and prints what the walk wrote.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../stark-anatomy_amd/csrc/combination_plan.h"

using namespace sc;

extern "C" {

// The entry on host memory.  stage_bytes: the staging buffer's size (g.verify_stage_bytes in the library).  points_out (optional):
// the point matrix, [1 + 2 w][n] residues; *chunks_out: chunks walked.  0: done; 1: a bad argument (nothing is written then)
int emu_stark_combination_batch(const sc_combination_t* shared, const void* rows, uint64_t n, uint8_t* verdicts_out, uint64_t stage_bytes, void* points_out,
                                uint64_t* chunks_out) {
    if (n == 0) return 0;
    if (!shared || !rows || !verdicts_out) return 1;
    const sc_combination_t& c = *shared;
    CombTables T;
    if (combination_prepare(c, rows, n, T)) return 1;
    if (chunks_out) *chunks_out = 0;
    if (T.undecided) {
        memset(verdicts_out, CB_UNDECIDED, n);
        return 0;
    }
    const uint32_t w = (uint32_t)c.registers, ncons = (uint32_t)c.ncons, nvars = 1 + 2 * w;
    const uint64_t stride = comb_row_bytes(w);
    const uint64_t fit = combination_chunk_rows(stage_bytes, w), per = n < fit ? n : fit;
    std::vector<Fe> staged((per * stride + 15) / 16), vals((size_t)(nvars + ncons) * per);
    std::vector<uint8_t> verdicts(per);
    const std::vector<MpolyVar> vars = combination_vars(w, per);
    Fe* tq = vals.data() + (size_t)nvars * per;
    for (uint64_t i = 0; i < n; i += per) {
        const uint64_t count = n - i < per ? n - i : per;
        memcpy(staged.data(), (const uint8_t*)rows + i * stride, count * stride);
        const CombShared S{(const uint8_t*)staged.data(), count, w, ncons, T.generator_m, T.omega_m, c.domain_length - 1, c.step, (const CombPoly*)c.polys,
                           (const Fe*)c.pool, T.weights_m.data(), T.member_bad.data(), T.shifts.data(), vals.data(), per, tq, verdicts.data()};
        const uint32_t gx = (uint32_t)((count + COLS_WG - 1) / COLS_WG);
        for (uint32_t y = 0; y < nvars; ++y)
            for (uint32_t x = 0; x < gx; ++x)
                for (uint32_t t = 0; t < COLS_WG; ++t) combination_point_thread(S, x, y, t);
        if (ncons) {
            const MpolyCols D{vals.data(), vars.data(), T.plan.cons.data(), T.plan.coef.data(), T.plan.drop.data(), T.plan.exps.data(), T.plan.nvw, ncons, count, tq, per, 0};
            for (uint32_t y = 0; y < ncons; ++y)
                for (uint32_t x = 0; x < gx; ++x)
                    for (uint32_t t = 0; t < COLS_WG; ++t) mpoly_cols_thread(D, x, y, t);
        }
        for (uint32_t x = 0; x < gx; ++x)
            for (uint32_t t = 0; t < COLS_WG; ++t) combination_sum_thread(S, x, t);
        memcpy(verdicts_out + i, verdicts.data(), count);
        if (points_out)
            for (uint32_t y = 0; y < nvars; ++y) memcpy((Fe*)points_out + (size_t)y * n + i, vals.data() + (size_t)y * per, count * sizeof(Fe));
        if (chunks_out) ++*chunks_out;
    }
    return 0;
}

// products per point of the plan of constraint k (what stage 2 spends), -1 for a bad argument
long long emu_combination_products(const sc_combination_t* shared, uint64_t k) {
    MpolyPlan P;
    if (mpoly_plan_build(1 + 2 * (uint32_t)shared->registers, shared->ncons, shared->nterms, shared->exps, (const Fe*)shared->coefs, P)) return -1;
    return k < P.products.size() ? (long long)P.products[k] : -1;
}
}

#if defined(COMBINATION_EMU_MAIN)
// <program> <call file>: the file is 16 u64 words {w, ncons, domain_length, step, members, n, stage_bytes, terms, pool_len, generator[2],
// omega[2], 0, 0, 0}, then coefs[terms], weights[members][1 + 2 ncons + 2 w], pool[pool_len] (16 bytes each), nterms[ncons],
// transition_shifts[ncons], boundary_shifts[w], polys[members][w][4] (u64 each), the rows, the exponent bytes.  Prints the status, the
// chunks, the verdicts and the point matrix as hexadecimal lines.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<Fe> file;
    Fe block[256];
    size_t got, bytes = 0;
    while ((got = fread(block, 1, sizeof(block), f)) > 0) {
        file.resize((bytes + got + 15) / 16);
        memcpy((uint8_t*)file.data() + bytes, block, got);
        bytes += got;
    }
    fclose(f);
    if (bytes < 128) return 2;
    const uint64_t* h = (const uint64_t*)file.data();
    const uint64_t w = h[0], ncons = h[1], members = h[4], n = h[5], stage_bytes = h[6], terms = h[7], pool_len = h[8], nw = 1 + 2 * ncons + 2 * w;
    const Fe* fe = file.data() + 8;
    const uint64_t* words = (const uint64_t*)(fe + terms + members * nw + pool_len);
    const uint64_t nwords = 2 * ncons + w + 4 * members * w, stride = comb_row_bytes((uint32_t)w);
    const uint8_t* rows = (const uint8_t*)(words + nwords + (nwords & 1));        // (the rows start on a 16-byte boundary)
    const size_t need = (size_t)(rows - (const uint8_t*)file.data()) + n * stride + terms * (1 + 2 * w);
    if (w == 0 || w > 127 || bytes < need) return 2;
    const sc_combination_t c{w, ncons, words, rows + n * stride, fe, {h[9], h[10]}, {h[11], h[12]}, h[2], h[3], words + ncons, words + 2 * ncons, members,
                             fe + terms, words + 2 * ncons + w, fe + terms + members * nw, pool_len};
    std::vector<uint8_t> verdicts(n, 0xEE);
    std::vector<Fe> points((size_t)(1 + 2 * w) * n, Fe{0, 0});
    uint64_t chunks = 0;
    const int rc = emu_stark_combination_batch(&c, rows, n, verdicts.data(), stage_bytes, points.data(), &chunks);
    printf("%d\n%llu\n", rc, (unsigned long long)chunks);
    for (uint8_t v : verdicts) printf("%02x", v);
    printf("\n");
    for (const Fe& v : points) printf("%016llx%016llx", (unsigned long long)v.hi, (unsigned long long)v.lo);
    printf("\n");
    return 0;
}
#endif

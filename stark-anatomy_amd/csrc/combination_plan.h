// combination_plan.h -- the host side of sc_stark_combination_batch (csrc/combination.cuh): the argument checks and the tables the
// three stages read.  Host code, shared by the library's entry (csrc/columns.hip) and the CPU walk of the kernels
// (tests/emu/combination_emu.cpp), like mpoly_plan.h.
#pragma once
#include <cstring>
#include <vector>
#include "../../include/starkcore.h"
#include "combination.cuh"

namespace sc {

struct CombTables {
    MpolyPlan plan;                      // of the AIR over nvars = 1 + 2 w variables
    std::vector<Fe> weights_m;           // [members][1 + 2 ncons + 2 w], Montgomery form
    std::vector<uint8_t> member_bad;     // [members]
    std::vector<uint64_t> shifts;        // [ncons + w]
    Fe generator_m, omega_m;
    bool undecided = false;              // generator or omega is not below p: every row is undecided
};

// nullptr, or what is wrong with the call (SC_ERR_BAD_ARG; nothing of T is then to be used).  n > 0.
inline const char* combination_prepare(const sc_combination_t& c, const void* rows, uint64_t n, CombTables& T) {
    const uint64_t w = c.registers, ncons = c.ncons;
    if (w == 0 || w > 127) return "between 1 and 127 registers (1 + 2 w <= 255 variables)";
    if (c.domain_length == 0 || (c.domain_length & (c.domain_length - 1))) return "the domain length is no power of two";
    if (c.step == 0) return "step is zero";
    if (!rows || !c.boundary_shifts || !c.weights || !c.polys || c.members == 0) return "null argument";
    if (ncons && (!c.nterms || !c.transition_shifts)) return "null argument";
    if (ncons > 0xFFFFull) return "more than 65 535 constraints";
    if (c.pool_len && !c.pool) return "null argument";
    uint64_t total = 0;
    for (uint64_t k = 0; k < ncons; ++k) total += c.nterms[k];
    if (total && (!c.exps || !c.coefs)) return "null argument";
    const uint32_t nvars = 1 + 2 * (uint32_t)w;
    const uint64_t stride = comb_row_bytes((uint32_t)w);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t head[2];                            // member, index (the caller's buffer need not be aligned)
        memcpy(head, (const uint8_t*)rows + i * stride, sizeof(head));
        if (head[0] >= c.members) return "combination row: member outside the table";
        if (head[1] >= c.domain_length) return "combination row: index outside the domain";
    }
    const CombPoly* polys = (const CombPoly*)c.polys;
    for (uint64_t k = 0; k < 2 * c.members * w; ++k)
        if (polys[k].off > c.pool_len || polys[k].len > c.pool_len - polys[k].off) return "a coefficient list outside the pool";
    if (const char* what = mpoly_plan_build(nvars, ncons, c.nterms, c.exps, (const Fe*)c.coefs, T.plan)) return what;
    // bad[i]: coefficients of pool[0 .. i) that are not below p
    const Fe* pool = (const Fe*)c.pool;
    std::vector<uint64_t> bad(c.pool_len + 1, 0);
    for (uint64_t i = 0; i < c.pool_len; ++i) bad[i + 1] = bad[i] + (fe_ge_p(pool[i]) ? 1 : 0);
    const uint64_t nw = 1 + 2 * ncons + 2 * w;
    const Fe* weights = (const Fe*)c.weights;
    T.weights_m.resize(c.members * nw);
    T.member_bad.assign(c.members, 0);
    for (uint64_t m = 0; m < c.members; ++m) {
        for (uint64_t k = 0; k < nw; ++k) {
            if (fe_ge_p(weights[m * nw + k])) T.member_bad[m] = 1;
            T.weights_m[m * nw + k] = to_mont(weights[m * nw + k]);
        }
        for (uint64_t k = 2 * m * w; k < 2 * (m + 1) * w; ++k)
            if (bad[polys[k].off + polys[k].len] != bad[polys[k].off]) T.member_bad[m] = 1;
    }
    T.shifts.assign(c.transition_shifts, c.transition_shifts + ncons);
    T.shifts.insert(T.shifts.end(), c.boundary_shifts, c.boundary_shifts + w);
    const Fe g{c.generator[0], c.generator[1]}, o{c.omega[0], c.omega[1]};
    T.undecided = fe_ge_p(g) || fe_ge_p(o);
    T.generator_m = to_mont(g);
    T.omega_m = to_mont(o);
    return nullptr;
}

// the variables of stage 2: variable j is row j of the point matrix [1 + 2 w][ldv], the same for the one member
inline std::vector<MpolyVar> combination_vars(uint32_t w, uint64_t ldv) {
    std::vector<MpolyVar> vars(1 + 2 * w);
    for (uint32_t j = 0; j < vars.size(); ++j) vars[j] = MpolyVar{j * ldv, 0, 0};
    return vars;
}

// rows of one chunk: what the staging buffer of `cap` bytes holds as [rows, 256-aligned][verdicts, 256-aligned]; at least 1
// (cap >= 16 KiB and a row is at most 64 + 32 * 127 bytes)
inline uint64_t combination_chunk_rows(uint64_t cap, uint32_t w) {
    const uint64_t per = comb_row_bytes(w) + 1;
    const uint64_t rows = cap > 512 ? (cap - 512) / per : 0;
    return rows ? rows : 1;
}

}  // namespace sc

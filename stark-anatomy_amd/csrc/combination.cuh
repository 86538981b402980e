// combination.cuh -- the third check of the batched verifier (FastStark.verify_batch): the nonlinear combination recomputed at every
// opened point (code/fast_stark.py:236-284) as rows, beside the Merkle and colinearity rows of merkle_verify.cuh.
//
// One call describes one AIR on one FRI domain (CombShared), the proofs it opens points of (members: their Fiat-Shamir weights and
// the coefficient lists of their boundary zerofiers and interpolants) and the opened points (rows).  A chunk of rows is three launches:
//   1  combination_point_kernel   vals[1 + 2w][rows]: x = generator * omega^index, then per register the trace value at `index` and at
//                                 the successor, each  quotient * zerofier(x) + interpolant(x)  -- one lane per (row, variable), so a
//                                 wide trace does not lengthen one lane's chain: pow (<= 2 log2 N products) + the two Horner walks + 2
//   2  mpoly_eval_columns_kernel  the AIR at every point under the plan of mpoly_plan.h (members = 1, n = rows): tq[ncons][rows]
//   3  combination_sum_kernel     one lane per row: the zerofier leaf inverted (143 products), the transition quotients, x^shift (the
//                                 power is kept while consecutive terms share a shift), the weighted sum, the comparison
// Arithmetic is exact on canonical residues, so a verdict is a fact about integers mod p.  Host-and-device code like columns.cuh:
// the lane bodies are SC_HD functions of (row, variable), walked thread by thread by tests/emu/combination_emu.cpp.
#pragma once
#include "mpoly_plan.h"   // columns.cuh (COLS_WG), field.cuh

namespace sc {

enum : uint8_t { CB_REJECT = 0, CB_ACCEPT = 1, CB_UNDECIDED = 2 };

struct CombRowHead {        // 64 bytes, then w boundary-quotient leaves at `index` and w at the successor (16 bytes each)
    uint64_t member, index;
    Fe claimed, randomizer, zerofier;
};
static_assert(sizeof(CombRowHead) == 64, "row layout");
SC_HD uint64_t comb_row_bytes(uint32_t w) { return sizeof(CombRowHead) + 32ull * w; }

struct CombPoly {           // a coefficient list: pool[off .. off + len), lowest degree first; len 0: the zero polynomial
    uint64_t off, len;
};

struct CombShared {         // device pointers (the emulation: host pointers) and what all rows share
    const uint8_t* rows;    // [n] rows of comb_row_bytes(w)
    uint64_t n;
    uint32_t w, ncons;
    Fe generator_m, omega_m;             // Montgomery form
    uint64_t mask, step;                 // domain_length - 1
    const CombPoly* polys;               // [members][w][2]: zerofier, interpolant
    const Fe* pool;                      // canonical
    const Fe* weights_m;                 // [members][1 + 2 ncons + 2 w], Montgomery form
    const uint8_t* member_bad;           // [members]: a weight or a coefficient of the member is not below p
    const uint64_t* shifts;              // [ncons + w]: transition, then boundary
    Fe* vals; uint64_t ldv;              // [1 + 2 w][ldv], ldv >= n
    const Fe* tq;                        // [ncons][ldv]: the AIR's values (stage 2)
    uint8_t* verdicts;                   // [n]
};

SC_HD const CombRowHead& comb_row(const CombShared& S, uint64_t i) { return *(const CombRowHead*)(S.rows + i * comb_row_bytes(S.w)); }
SC_HD const Fe* comb_leaves(const CombShared& S, uint64_t i) { return (const Fe*)(S.rows + i * comb_row_bytes(S.w) + sizeof(CombRowHead)); }

// p(x) for a canonical coefficient list and x in Montgomery form; canonical
SC_HD Fe comb_horner(const Fe* pool, CombPoly p, Fe x_m) {
    if (p.len == 0) return fe_zero();
    const Fe* c = pool + p.off;
    Fe acc = c[p.len - 1];
    for (uint64_t k = p.len - 1; k-- > 0;) acc = fe_add(mont_mul(acc, x_m), c[k]);
    return acc;
}

// stage 1, lane (row i, variable y): y = 0: x; 1 + s: register s at `index`; 1 + w + s: register s at the successor.
// A leaf that is not below p gives 0 (stage 3 leaves such a row undecided).
SC_HD Fe combination_point_value(const CombShared& S, uint64_t i, uint32_t y) {
    const CombRowHead& r = comb_row(S, i);
    const bool next = y > S.w;
    const uint64_t at = next ? (r.index + S.step) & S.mask : r.index;
    const Fe x_m = mont_mul(S.generator_m, mont_pow(S.omega_m, at));
    if (y == 0) return from_mont(x_m);
    const uint32_t s = next ? y - 1 - S.w : y - 1;
    const Fe leaf = comb_leaves(S, i)[next ? S.w + s : s];
    if (fe_ge_p(leaf)) return fe_zero();
    const CombPoly* p = S.polys + 2 * (r.member * S.w + s);
    const Fe z = comb_horner(S.pool, p[0], x_m);
    return fe_add(mont_mul(to_mont(leaf), z), comb_horner(S.pool, p[1], x_m));
}

// stage 3, lane (row i)
SC_HD uint8_t combination_sum_row(const CombShared& S, uint64_t i) {
    const CombRowHead& r = comb_row(S, i);
    const Fe* leaves = comb_leaves(S, i);
    bool bad = S.member_bad[r.member] != 0 || fe_ge_p(r.claimed) || fe_ge_p(r.randomizer) || fe_ge_p(r.zerofier) || fe_is_zero(r.zerofier);
    for (uint32_t s = 0; s < 2 * S.w; ++s) bad |= fe_ge_p(leaves[s]);
    if (bad) return CB_UNDECIDED;
    const Fe* wt = S.weights_m + r.member * (1ull + 2ull * S.ncons + 2ull * S.w);
    const Fe x_m = to_mont(S.vals[i]);
    const Fe zinv_m = mont_inv(to_mont(r.zerofier));
    Fe total = mont_mul(r.randomizer, wt[0]);
    uint64_t shift = 0;
    Fe xs_m = fe_mont_one();                       // x^shift
    for (uint32_t t = 0; t < S.ncons + S.w; ++t) {
        const Fe q = t < S.ncons ? mont_mul(S.tq[(uint64_t)t * S.ldv + i], zinv_m) : leaves[t - S.ncons];
        if (S.shifts[t] != shift) {
            shift = S.shifts[t];
            xs_m = mont_pow(x_m, shift);
        }
        total = fe_add(total, mont_mul(q, wt[1 + 2 * t]));
        total = fe_add(total, mont_mul(mont_mul(q, xs_m), wt[2 + 2 * t]));
    }
    return fe_eq(total, r.claimed) ? CB_ACCEPT : CB_REJECT;
}

// the lanes of the two launches: grid (row blocks) x (1 + 2 w variables), and (row blocks)
SC_HD void combination_point_thread(const CombShared& S, uint32_t wg_x, uint32_t wg_y, uint32_t tid) {
    const uint64_t i = (uint64_t)wg_x * COLS_WG + tid;
    if (i < S.n) S.vals[(uint64_t)wg_y * S.ldv + i] = combination_point_value(S, i, wg_y);
}
SC_HD void combination_sum_thread(const CombShared& S, uint32_t wg_x, uint32_t tid) {
    const uint64_t i = (uint64_t)wg_x * COLS_WG + tid;
    if (i < S.n) S.verdicts[i] = combination_sum_row(S, i);
}

}  // namespace sc

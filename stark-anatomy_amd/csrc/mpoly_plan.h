// mpoly_plan.h -- the evaluation plan of mpoly_eval_columns_kernel (csrc/columns.cuh): host code, shared by the library's entry
// (csrc/columns.hip) and the CPU walk of the kernel (tests/emu/mpoly_columns_emu.cpp).
//
// A constraint  sum_t coef_t * prod_j v_j^e_tj  is evaluated as a Horner walk in ONE variable h -- the used variable with the largest
// maximum exponent, the lowest index on a tie -- over the terms sorted (stably) by e_th, descending:
//     acc <- acc * v_h^drop_t               drop_t = e_h of the term before - e_h of this one (0 for the first term)
//     acc <- acc + coef_t * prod_{j != h} v_j^e_tj
// and after the last term  acc <- acc * v_h^tail, tail = e_h of the last term:  max e_h + sum_t sum_{j != h} e_tj  products per point
// (`products`) instead of the sum of all exponents (`products_flat`: what mpoly_eval_kernel spends).
//
// No value is ever converted.  mont_mul(x, y) = x y / R (R = 2^128), so a product with a canonical value takes one factor R out of
// the running product.  Term t meets exactly  s_t = sum_{j != h} e_tj  such products before it joins the accumulator and e_th more
// afterwards, so its coefficient is stored as  coef_t * R^(s_t + e_th):  every summand of the accumulator then carries the same power
// of R at every step, and what is left after the tail is the canonical result -- the same residue mpoly_eval_kernel writes, the
// arithmetic being exact.
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>
#include "columns.cuh"   // MpolyCons, MpolyVar, MPOLY_NO_VAR

namespace sc {

struct MpolyPlan {
    uint32_t nvw = 0;                    // 32-bit words of exponent bytes per term: (nvars + 3) / 4
    std::vector<MpolyCons> cons;
    std::vector<Fe> coef;                // [terms] coef_t * R^(s_t + e_th)
    std::vector<uint32_t> drop;          // [terms]
    std::vector<uint32_t> exps;          // [terms][nvw]: byte j of a term's words = e_tj, the Horner variable's byte 0
    std::vector<uint64_t> products, products_flat;       // per constraint
    std::vector<uint8_t> used;           // [nvars]: some term of some constraint has a non-zero exponent there
};

// exps: the constraints' [nterms_c][nvars] exponent bytes one after the other, coefs: their canonical coefficients likewise.
// nullptr, or what is wrong (nothing of P is then to be used)
inline const char* mpoly_plan_build(uint32_t nvars, uint64_t ncons, const uint64_t* nterms, const uint8_t* exps, const Fe* coefs, MpolyPlan& P) {
    uint64_t total = 0;
    for (uint64_t c = 0; c < ncons; ++c) total += nterms[c];
    if (total > 0x7FFFFFFFull) return "too many terms";
    P = MpolyPlan();
    P.nvw = (nvars + 3) / 4;
    P.used.assign(nvars, 0);
    P.coef.reserve(total);
    P.drop.reserve(total);
    P.exps.reserve(total * P.nvw);
    const Fe r_m{R2_LO, R2_HI};                      // R in Montgomery form
    uint64_t first = 0;
    for (uint64_t c = 0; c < ncons; ++c) {
        const uint64_t nt = nterms[c];
        const uint8_t* e = exps + first * nvars;
        std::vector<uint32_t> top(nvars, 0);
        for (uint64_t t = 0; t < nt; ++t)
            for (uint32_t j = 0; j < nvars; ++j) top[j] = std::max<uint32_t>(top[j], e[t * nvars + j]);
        uint32_t h = MPOLY_NO_VAR;
        for (uint32_t j = 0; j < nvars; ++j) {
            if (top[j]) P.used[j] = 1;
            if (top[j] && (h == MPOLY_NO_VAR || top[j] > top[h])) h = j;
        }
        auto eh = [&](uint64_t t) -> uint32_t { return h == MPOLY_NO_VAR ? 0u : e[t * nvars + h]; };
        std::vector<uint64_t> order(nt);
        std::iota(order.begin(), order.end(), 0ull);
        std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return eh(a) > eh(b); });
        uint64_t products = nt ? eh(order[0]) : 0, flat = 0;
        for (uint64_t k = 0; k < nt; ++k) {
            const uint64_t t = order[k];
            const Fe coef = coefs[first + t];
            if (fe_ge_p(coef)) return "coefficient is not a canonical residue";
            uint64_t others = 0;
            for (uint32_t w = 0; w < P.nvw; ++w) {
                uint32_t word = 0;
                for (uint32_t b = 0; b < 4 && 4 * w + b < nvars; ++b) {
                    const uint32_t j = 4 * w + b;
                    if (j == h) continue;
                    word |= (uint32_t)e[t * nvars + j] << (8 * b);
                    others += e[t * nvars + j];
                }
                P.exps.push_back(word);
            }
            P.coef.push_back(mont_mul(coef, mont_pow(r_m, others + eh(t))));
            P.drop.push_back(k ? eh(order[k - 1]) - eh(t) : 0u);
            products += others;
            flat += others + eh(t);
        }
        P.cons.push_back(MpolyCons{h, (uint32_t)first, (uint32_t)nt, nt ? eh(order[nt - 1]) : 0u});
        P.products.push_back(products);
        P.products_flat.push_back(flat);
        first += nt;
    }
    return nullptr;
}

// The variables as the kernel reads them.  var_src / var_rot (both or neither) mean what they mean in sc_mpoly_eval_rot_dev:
// var_src[j] == j with var_rot[j] == 0 for a variable stored in its own place (var_base[j], var_ld[j]), another stored variable's
// index for one read off that variable var_rot[j] places on, MPOLY_NO_VAR for one that no term may use.
// 0: fine; 1: a bad argument; 2: turned variables over a count that is no power of two
inline int mpoly_vars_resolve(uint32_t nvars, uint64_t n, const uint64_t* var_base, const uint64_t* var_ld, const uint32_t* var_src, const uint64_t* var_rot,
                              const std::vector<uint8_t>& used, std::vector<MpolyVar>& out, const char** what) {
    out.assign(nvars, MpolyVar{0, 0, 0});
    bool turned = false;
    for (uint32_t j = 0; j < nvars; ++j) {
        if (!var_src) {
            out[j] = MpolyVar{var_base[j], var_ld[j], 0};
            continue;
        }
        const uint32_t s = var_src[j];
        if (s == MPOLY_NO_VAR) {
            if (used[j]) { *what = "a term uses a variable that is marked absent"; return 1; }
            continue;
        }
        if (s >= nvars || var_src[s] != s || var_rot[s] != 0 || (s == j && var_rot[j] != 0)) {
            *what = "a turned variable must point at one stored in its own place";
            return 1;
        }
        if (s != j) turned = true;
        out[j] = MpolyVar{var_base[s], var_ld[s], s != j ? var_rot[j] : 0};
    }
    if (turned) {
        if (n & (n - 1)) { *what = "turned variables need a power-of-two domain"; return 2; }
        for (uint32_t j = 0; j < nvars; ++j) out[j].rot &= n - 1;
    }
    return 0;
}

}  // namespace sc

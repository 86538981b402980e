// columns.cuh -- pointwise steps over a MATRIX of polynomial columns (column c at element c * ld): the division, the short-divisor
// evaluation, the unscale / store / exactness step of the coset division, the weighted combination of shifted terms and the one
// verdict of a whole batch of deferred checks (ntt.py: coset_divide_columns_device, combine_columns_device).
//
// Host-and-device code like rescue_prime.cuh and merkle_forest.cuh: every per-thread body is an SC_HD function of (workgroup,
// thread, grid shape), so g++ walks the same indexing thread by thread in tests/emu/columns_emu.cpp and hipcc wraps the bodies in
// the kernels of csrc/columns.hip.  Arithmetic is exact on canonical residues: every result is the single-column kernels' own
// (pointwise_div_kernel, short_poly_coset_kernel, scale_pow_kernel, axpy_shift_kernel of core.hip), element for element.
#pragma once
#include "ntt_tile.cuh"   // field.cuh, pow2level

namespace sc {

constexpr uint32_t COLS_WG = 256;         // threads per workgroup of every kernel here
constexpr int DIV_COLS_K = 16;            // positions per thread of the division (pointwise_div_kernel's K)

// flag |= bits / word = max(word, v): atomics on the device, plain updates in the one-thread-at-a-time walk of the emulation
SC_HD void cols_flag_or(uint32_t* word, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(word, bits);
#else
    *word |= bits;
#endif
}
SC_HD void cols_word_max(long long* word, long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(word, v);
#else
    if (v > *word) *word = v;
#endif
}

// ---- out[c][i] = a[c][i] / b[c][i], c < cols, i < n.  ld_b == 0: ONE divisor row for every column.
// Grid (position blocks) x (column chunks): thread t of the position grid owns the K positions t + k * nthreads (strided, so a wave's
// loads are consecutive), workgroup row y the columns [y * chunk, (y + 1) * chunk).  Montgomery's trick turns the K inversions into
// one (about 190 products) plus 3 (K - 1) products; with a shared divisor the K inverses stay in registers and every column of the
// chunk costs one product per element, so the inversion is paid once per chunk.  With a divisor per column there is nothing to
// share: pointwise_div_kernel's scheme, column after column.  zero[c] |= 1 where column c met a zero divisor (a shared divisor
// marks every column of the chunk, and every chunk sees it).  `out` may be `a` (each element is read by the thread that writes it).
struct DivCols {
    const Fe* a; uint64_t ld_a;
    const Fe* b; uint64_t ld_b;
    Fe* out; uint64_t ld_out;
    uint64_t n, cols;
    uint32_t chunk;
    uint32_t* zero;          // [cols]
};
// batch inversion of the K divisor values of thread t in row `b`: pre[k] <- (b_k)^-1 in Montgomery form; false: one of them is zero
template <int K>
SC_HD bool div_cols_invert(const Fe* b, uint64_t n, uint64_t t, uint64_t nthreads, Fe (&pre)[K]) {
    Fe bm[K];
    Fe acc = fe_mont_one();
    bool zero = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t i = t + (uint64_t)k * nthreads;
        const Fe v = (i < n) ? b[i] : fe_one();
        zero |= fe_is_zero(v);
        bm[k] = to_mont(v);
        pre[k] = acc;                  // product of bm[0..k)
        acc = mont_mul(acc, bm[k]);
    }
    Fe inv = mont_inv(acc);
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
        pre[k] = mont_mul(inv, pre[k]);
        inv = mont_mul(inv, bm[k]);
    }
    return !zero;
}
template <int K>
SC_HD void div_cols_thread(const DivCols& D, uint32_t wg_x, uint32_t wg_y, uint32_t tid, uint32_t grid_x) {
    const uint64_t nthreads = (uint64_t)grid_x * COLS_WG;
    const uint64_t t = (uint64_t)wg_x * COLS_WG + tid;
    if (t >= D.n) return;                                  // (no position at all: the padding of the last workgroup)
    const uint64_t c0 = (uint64_t)wg_y * D.chunk;
    const uint64_t c1 = c0 + D.chunk < D.cols ? c0 + D.chunk : D.cols;
    Fe inv[K];
    const bool shared = D.ld_b == 0;
    bool ok = shared ? div_cols_invert<K>(D.b, D.n, t, nthreads, inv) : true;
    for (uint64_t c = c0; c < c1; ++c) {
        if (!shared) ok = div_cols_invert<K>(D.b + c * D.ld_b, D.n, t, nthreads, inv);
        if (!ok) cols_flag_or(D.zero + c, 1u);
        const Fe* a = D.a + c * D.ld_a;
        Fe* out = D.out + c * D.ld_out;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint64_t i = t + (uint64_t)k * nthreads;
            if (i < D.n) out[i] = mont_mul(a[i], inv[k]);
        }
    }
}
SC_HD uint32_t div_cols_grid_x(uint64_t n) { return (uint32_t)(((n + DIV_COLS_K - 1) / DIV_COLS_K + COLS_WG - 1) / COLS_WG); }

// ---- out[c][i] = b_c(offset * root^i), i < order, for SHORT divisors of nb coefficients (canonical; column c at b + c * ld_b):
// short_poly_coset_kernel's Horner at every point, for `cols` divisors in one launch (grid: position blocks x columns)
SC_HD void short_poly_cols_thread(const Fe* b, uint64_t ld_b, uint32_t nb, Fe off_m, const Fe* tl, const Fe* th, Fe* out, uint64_t order, uint64_t c, uint64_t i) {
    if (i >= order) return;
    const Fe* bc = b + c * ld_b;
    const Fe x_m = mont_mul(off_m, pow2level(tl, th, i));
    Fe acc = bc[nb - 1];
    for (uint32_t k = nb - 1; k-- > 0;) acc = fe_add(mont_mul(acc, x_m), bc[k]);
    out[c * order + i] = acc;
}

// ---- the end of the coset division for a whole matrix: coefficient i of column c of the interpolant `full` [cols][order] is
// unscaled by offset^-i (lo / hi: the two-level power table of offset^-1) and stored where i < n_out[c]; above the quotient it
// must vanish -- a factor offset^-i does not change that, so those are only tested.  Returns the index, counted from n_out[c], of
// a non-zero coefficient above the quotient, -1 otherwise: the kernel reports the highest of a wave with cols_word_max(rem + c).
struct UnscaleCols {
    const Fe* full; uint64_t order;
    Fe* out; uint64_t ld_out;
    const uint64_t* n_out;   // [cols], device memory
    const Fe* lo; const Fe* hi;
    long long* rem;          // [cols], preset to -1
};
SC_HD long long unscale_cols_thread(const UnscaleCols& U, uint64_t c, uint64_t i) {
    if (i >= U.order) return -1;
    const uint64_t keep = U.n_out[c];
    const Fe v = U.full[c * U.order + i];
    if (i < keep) {
        U.out[c * U.ld_out + i] = mont_mul(v, pow2level(U.lo, U.hi, i));
        return -1;
    }
    return fe_is_zero(v) ? -1 : (long long)(i - keep);
}

// ---- out[c][i] = sum_t w[c][t] * src_t[c][i - shift_t] over the terms with shift_t <= i < shift_t + n_t, i < n_out: the nonlinear
// combination of code/fast_stark.py:130-145 (a chain of axpy_shift_kernel launches over a zeroed accumulator) as ONE pass that
// writes every element once.  One thread per output element; the term index is the same in every lane, so the table and the
// weights (device memory, weights in Montgomery form, [cols][nterms]) are read with scalar loads.
struct CombineTerm {         // (the layout of sc_combine_term_t)
    const Fe* src; uint64_t ld, n, shift;
};
SC_HD Fe combine_cols_elem(const CombineTerm* terms, uint32_t nterms, const Fe* w_m, uint64_t c, uint64_t i) {
    Fe acc = fe_zero();
    const Fe* w = w_m + c * nterms;
    for (uint32_t t = 0; t < nterms; ++t) {
        const CombineTerm T = terms[t];
        const uint64_t j = i - T.shift;                    // (wraps below the shift: then j >= n)
        if (i >= T.shift && j < T.n) acc = fe_add(acc, mont_mul(T.src[c * T.ld + j], w[t]));
    }
    return acc;
}

// ---- ONE verdict for the checks of `cols` columns: lane l of one wave looks at the columns l, l + 64, ... (verdict_lane), then
// the 64 partial results are merged into the words of one pinned slot (verdict_words):
//   words[0], words[1]  zero-divisor flag and remainder index of the LOWEST failing column -- (0, -1) if none failed: what
//                       sc_later_wait returns for a single division      words[2]  that column, -1 if none      words[3]  failing columns
// rem == nullptr: a pointwise division (no remainder to speak of).
SC_HD void verdict_lane(const uint32_t* zero, const long long* rem, uint64_t cols, uint32_t lane, long long* first, uint64_t* count) {
    long long f = -1;
    uint64_t n = 0;
    for (uint64_t c = lane; c < cols; c += 64) {
        if (zero[c] != 0 || (rem && rem[c] >= 0)) {
            if (f < 0) f = (long long)c;
            ++n;
        }
    }
    *first = f;
    *count = n;
}
SC_HD void verdict_words(const uint32_t* zero, const long long* rem, const long long* firsts, const uint64_t* counts, uint64_t words[4]) {
    long long f = -1;
    uint64_t n = 0;
    for (int l = 0; l < 64; ++l) {
        if (firsts[l] >= 0 && (f < 0 || firsts[l] < f)) f = firsts[l];
        n += counts[l];
    }
    words[0] = f >= 0 ? (uint64_t)zero[f] : 0ull;
    words[1] = (uint64_t)((f >= 0 && rem) ? rem[f] : -1ll);
    words[2] = (uint64_t)f;
    words[3] = n;
}

// ---- out[(m * ncons + c) * ld_out + i] = constraint c at point i of member m: multivariate polynomials evaluated pointwise on the
// values of `members` point sets, every member and every constraint in one launch (mpoly_eval_kernel takes one of each).  Grid
// (point blocks) x (pairs (m, c), `pair0` on in a launch that is not the first): the pair, and with it every table entry a lane
// reads, is the same in all lanes of a workgroup, so the tables come in through scalar loads and the loops over terms, variables and
// exponents are scalar control flow.  The plan (csrc/mpoly_plan.h) is a Horner walk in the constraint's variable of highest
// exponent: v_h is loaded once, and a term costs the products of its other variables only.  Values are read in canonical form and
// never converted: the powers of R that the Montgomery products take out are in the plan's coefficients.  No value is modified.
constexpr uint32_t MPOLY_NO_VAR = 0xFFFFFFFFu;       // MpolyCons::h of a constraint that uses no variable (the value of SC_MPOLY_ABSENT)
struct MpolyCons {           // one constraint
    uint32_t h;              // the Horner variable, MPOLY_NO_VAR: none
    uint32_t first, nterms;  // its terms: [first, first + nterms) of coef / drop / exps
    uint32_t tail;           // e_h of its last term
};
struct MpolyVar {            // a variable's value at point i of member m: element base + m * ld + ((i + rot) mod n) of `vals`
    uint64_t base, ld, rot;  // (rot != 0 only with n a power of two)
};
struct MpolyCols {
    const Fe* vals;
    const MpolyVar* vars;    // [nvars]
    const MpolyCons* cons;   // [ncons]
    const Fe* coef;          // [terms] coef_t * R^(products the term goes through)
    const uint32_t* drop;    // [terms] products with v_h before the term is added
    const uint32_t* exps;    // [terms][nvw]: byte j = e_tj, the Horner variable's byte 0
    uint32_t nvw, ncons;
    uint64_t n;
    Fe* out; uint64_t ld_out;
    uint32_t pair0;
};
SC_HD Fe mpoly_cols_value(const MpolyCols& D, uint32_t j, uint64_t m, uint64_t i) {
    const MpolyVar V = D.vars[j];
    return D.vals[V.base + m * V.ld + (V.rot ? ((i + V.rot) & (D.n - 1)) : i)];
}
SC_HD void mpoly_cols_thread(const MpolyCols& D, uint32_t wg_x, uint32_t wg_y, uint32_t tid) {
    const uint64_t i = (uint64_t)wg_x * COLS_WG + tid;
    if (i >= D.n) return;
    const uint32_t pair = D.pair0 + wg_y;
    const uint32_t m = pair / D.ncons;
    const MpolyCons C = D.cons[pair - m * D.ncons];
    const Fe vh = C.h != MPOLY_NO_VAR ? mpoly_cols_value(D, C.h, m, i) : fe_zero();
    Fe acc = fe_zero();
    for (uint32_t t = C.first; t < C.first + C.nterms; ++t) {
        for (uint32_t k = D.drop[t]; k; --k) acc = mont_mul(acc, vh);
        Fe p = D.coef[t];
        const uint32_t* e = D.exps + (uint64_t)t * D.nvw;
        for (uint32_t w = 0; w < D.nvw; ++w) {
            uint32_t word = e[w];
            for (uint32_t j = 4 * w; word; ++j, word >>= 8) {
                uint32_t k = word & 255u;
                if (!k) continue;
                const Fe v = mpoly_cols_value(D, j, m, i);
                for (; k; --k) p = mont_mul(p, v);
            }
        }
        acc = fe_add(acc, p);
    }
    for (uint32_t k = C.tail; k; --k) acc = mont_mul(acc, vh);
    D.out[(uint64_t)pair * D.ld_out + i] = acc;
}
// ---- out[c][i] = in[c][i] * factor^i, i < n, c < cols (lo / hi: the two-level power table of `factor`): scale_pow_kernel -- Polynomial.scale
// -- for the rows of a matrix, grid (position blocks) x (columns).  `out` may be `in` (with the same stride).
SC_HD void scale_cols_thread(const Fe* in, uint64_t ld_in, Fe* out, uint64_t ld_out, uint64_t n, const Fe* lo, const Fe* hi, uint64_t c, uint64_t i) {
    if (i < n) out[c * ld_out + i] = mont_mul(in[c * ld_in + i], pow2level(lo, hi, i));
}

// ---- the randomized trace matrix of a batch of proofs (code/fast_stark.py:79-81 for every member at once): column c = m * registers
// + s of `out` (at element c * ld_out) is the trace column at element c * ld_trace of `trace`, rows elements, then `extra` randomizer
// values: element rows + r is Field.sample (fe_sample_bytes) of the `width` bytes at draws + m * draws_stride + (r * registers + s) *
// width -- the reference's draw order, row by row, register by register.  Grid (position blocks) x (columns, `col0` on in a launch
// that is not the first); one thread per output element.  rows == 0: nothing is read from `trace` (it may be null), and with
// registers == 1 the call samples one polynomial of `extra` coefficients per member.
struct RandomizedCols {
    const Fe* trace; uint64_t rows, ld_trace;
    uint64_t registers;
    const uint8_t* draws; uint64_t draws_stride;
    uint64_t extra; uint32_t width;
    Fe* out; uint64_t ld_out;
    uint64_t col0;
};
SC_HD void randomized_cols_thread(const RandomizedCols& D, uint32_t wg_x, uint32_t wg_y, uint32_t tid) {
    const uint64_t i = (uint64_t)wg_x * COLS_WG + tid;
    if (i >= D.rows + D.extra) return;
    const uint64_t c = D.col0 + wg_y;
    Fe v;
    if (i < D.rows) {
        v = D.trace[c * D.ld_trace + i];
    } else {
        const uint64_t m = c / D.registers, s = c - m * D.registers, r = i - D.rows;
        v = fe_sample_bytes(D.draws + m * D.draws_stride + (r * D.registers + s) * D.width, D.width);
    }
    D.out[c * D.ld_out + i] = v;
}

// rows of a grid (pairs of mpoly_eval_columns_kernel, columns of scale_cols_kernel) per launch: gridDim.y takes 65 535
constexpr uint32_t COLS_GRID_ROWS = 65535;

}  // namespace sc

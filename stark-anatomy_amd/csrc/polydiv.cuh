// Division with remainder on the device: Polynomial.divide (code/univariate.py:80-97) for a of na and b of nb coefficients,
// b[nb-1] != 0, m = na - nb + 1 (model: tests/emu/poly_divide_model.py).
//
// The reference subtracts a multiple of the divisor per quotient coefficient.  Quotient and remainder are unique, so the device
// takes the reversal route instead: with rev(f)(y) = y^deg f(1/y), a = q b + r becomes rev(a) = rev(q) rev(b) mod y^m, hence
//   1. h = rev(b)^-1 mod y^m        Newton doubling h <- h (2 - G h) from h_0 = 1 / b[nb-1] (pt_newton_kernel, polytree.cuh);
//   2. rev(q) = rev(a)[0..m) h mod y^m;
//   3. r = (a - q b) mod (x^n3 - 1), first nb - 1 entries, n3 >= nb a power of two: deg r < nb - 1 < n3, so the cyclic residue
//      IS r -- q and a are folded to n3 entries and the product runs at the divisor's size whatever the numerator's.
// The arithmetic is in the transforms between these kernels; the kernels are elementwise, one 16-byte element per lane (one
// 128-bit load and store), lanes along a column (unit stride, descending for the reversed loads), the column on grid.y: column
// c of a matrix lies at element c * ld.  One column is the same launch with grid.y = 1.
#pragma once
#include "field.cuh"

namespace sc {

#define PD_INDEX() ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x)

// dst[c][t] = src[c][top - t], t < count (count <= top + 1): the first `count` coefficients of the reversed polynomial whose
// highest coefficient is src[c][top].  rev(b) and rev(a) going in (the transform zero-extends behind `count`), q = rev(rev(q)) going out.
__global__ void __launch_bounds__(256) pd_rev_kernel(const Fe* __restrict__ src, uint64_t ld_src, uint64_t top, uint64_t count, Fe* __restrict__ dst, uint64_t ld_dst) {
    const uint64_t t = PD_INDEX();
    if (t < count) dst[blockIdx.y * ld_dst + t] = src[blockIdx.y * ld_src + top - t];
}

// frequency domain: v[c][i] = k * v[c][i] * tab[i], one table row for every column   (c_m2 = k * R^2: undoes both Montgomery factors)
__global__ void __launch_bounds__(256) pd_mul_tab_kernel(Fe* __restrict__ v, uint64_t ld, const Fe* __restrict__ tab, uint64_t n, Fe c_m2) {
    const uint64_t i = PD_INDEX();
    if (i >= n) return;
    Fe* at = v + blockIdx.y * ld + i;
    *at = mont_mul(mont_mul(*at, tab[i]), c_m2);
}

// revq[c][0..m) = rev(q_c)  ->  fold[c][j] = sum of q_c[i] over i = j, j + n3, ... < m, for j < min(m, n3): q mod (x^n3 - 1).  With
// q != nullptr the quotient is stored on the way, q[c][i] = revq[c][m - 1 - i]: every i < m is visited exactly once.
__global__ void __launch_bounds__(256) pd_fold_rev_kernel(const Fe* __restrict__ revq, uint64_t ld_rev, uint64_t m, uint64_t n3, Fe* __restrict__ fold, uint64_t ld_fold,
                                                          Fe* __restrict__ q, uint64_t ld_q) {
    const uint64_t j = PD_INDEX();
    if (j >= n3 || j >= m) return;
    const Fe* src = revq + blockIdx.y * ld_rev;
    Fe acc{0, 0};
    for (uint64_t i = j; i < m; i += n3) {
        const Fe v = src[m - 1 - i];
        if (q) q[blockIdx.y * ld_q + i] = v;
        acc = fe_add(acc, v);
    }
    fold[blockIdx.y * ld_fold + j] = acc;
}

// r[c][j] = (sum of a_c[i] over i = j, j + n3, ... < na) - prod[c][j], j < nr: the numerator folded to n3 entries less the cyclic
// product q b, of which only the remainder's nr = nb - 1 entries are formed
__global__ void __launch_bounds__(256) pd_remainder_kernel(const Fe* __restrict__ a, uint64_t ld_a, uint64_t na, const Fe* __restrict__ prod, uint64_t ld_prod, uint64_t n3,
                                                           Fe* __restrict__ r, uint64_t ld_r, uint64_t nr) {
    const uint64_t j = PD_INDEX();
    if (j >= nr) return;
    const Fe* src = a + blockIdx.y * ld_a;
    Fe acc{0, 0};
    for (uint64_t i = j; i < na; i += n3) acc = fe_add(acc, src[i]);
    r[blockIdx.y * ld_r + j] = fe_sub(acc, prod[blockIdx.y * ld_prod + j]);
}

}  // namespace sc

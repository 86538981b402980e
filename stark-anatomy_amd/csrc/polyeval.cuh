// Values of polynomials resident in HBM at a list of points, DIRECTLY: Polynomial.evaluate / evaluate_domain (code/univariate.py:99-105)
// as m * k * cols modular products, no tree, no transform (model: tests/emu/poly_evaluate_model.py).  This is the route for few
// points against many coefficients, where the subproduct tree would first reduce the polynomial modulo a zerofier at the
// polynomial's own size; sc_polytree_evaluate_columns_dev stays the route for k ~ m.
//
//   out[c * ld_out + j] = sum_i coeffs[c * ld_in + i] * points[j]^i,    i < m, j < k, c < cols
//
// The coefficients of a column are cut into CHUNKS of 2^chunk_log coefficients; one workgroup computes, for one chunk, one column and
// a few points, the chunk's own value  partial = sum_i chunk[i] * x^i.  Two forms of that kernel, by the number of points:
//   * coefficients across lanes (pe_coeffs_across_kernel, few points; one point must be efficient): thread t of the PE_T threads walks
//     coefficients t, t + T, t + 2T, ... of the chunk by Horner in x^T -- every step one coalesced 16-byte load per lane, read once for
//     the G <= 4 points the workgroup serves -- and the workgroup folds its T accumulators a_t into sum_t a_t x^t by a tree through LDS
//     whose level h is a_t += x^h * a_(t+h): the powers x^(2^b) are the squarings that lead to x^T anyway, so the factor x^t costs
//     log2 T products per thread instead of a power per thread;
//   * points across lanes (pe_points_across_kernel, many points): one thread per point, one wave per workgroup, the chunk's
//     coefficients are the same address in every lane (wave-uniform loads), Horner per thread -- as PE_WAYS independent chains in
//     x^4 over the coefficients 4 i + r, folded at the end, so that a thread has as many products in flight as the other form.
// A launch of either form covers every chunk (grid.x), a range of points (grid.y) and a range of columns (grid.z).  With ONE chunk the
// partial IS the value and goes straight to `out`; with more, the partials go to a temporary [cols][k][chunks] and a second, small
// launch (pe_combine_kernel) forms  out = sum_chunks partial[chunk] * (x^(2^chunk_log))^chunk  -- again a polynomial value, now in
// y = x^(2^chunk_log) with `chunks` coefficients, by one wave per output with the same Horner-in-y^64 and the same tree.  No workgroup
// waits for another, there are no tickets and no atomics on field elements (the choice of merkle_forest.cuh): every output is a fixed
// sequence of exact modular operations, so the results do not depend on the chunk length, on the form or on the schedule.
//
// Arithmetic: field.cuh.  Data is canonical in HBM, LDS and registers; only the powers of the points are Montgomery forms
// (to_mont on load), so acc * x^T is ONE mont_mul with a canonical result and nothing is converted on store.
#pragma once
#include "field.cuh"

namespace sc {

constexpr int PE_LOG_T = 8;
constexpr int PE_T = 1 << PE_LOG_T;      // threads of a coefficients-across-lanes workgroup = the Horner stride
constexpr int PE_LOG_W = 6;
constexpr int PE_W = 1 << PE_LOG_W;      // points of a points-across-lanes workgroup, lanes of a combine: one wave
constexpr int PE_WAYS = 4;               // independent Horner chains of a points-across-lanes thread

// G accumulators times G Montgomery factors (mont_mul2 where there are two)
template <int G>
SC_HD void pe_mul(Fe (&acc)[G], const Fe (&f)[G]) {
    if constexpr (G == 1) {
        acc[0] = mont_mul(acc[0], f[0]);
    } else {
#pragma unroll
        for (int g = 0; g < G; g += 2) mont_mul2(acc[g], f[g], acc[g + 1], f[g + 1], acc[g], acc[g + 1]);
    }
}

// Coefficients across lanes.  grid = (chunks, groups of G points, columns); the workgroup serves points j0 + G * blockIdx.y + g, g < G
// (indices >= k repeat the last point and are not stored), column c0 + blockIdx.z, chunk blockIdx.x.
// dst[c * dst_col + j * dst_point + chunk]: the partials' temporary, or `out` itself when there is one chunk (dst_col = ld_out, dst_point = 1).
template <int G>
__global__ void __launch_bounds__(PE_T) pe_coeffs_across_kernel(const Fe* __restrict__ coeffs, uint64_t m, uint64_t ld_in, const Fe* __restrict__ points, uint64_t k, uint64_t j0,
                                                                 uint64_t c0, int chunk_log, Fe* __restrict__ dst, uint64_t dst_col, uint64_t dst_point) {
    __shared__ Fe pw[G][PE_LOG_T];        // x_g^(2^b) as Montgomery forms
    __shared__ Fe red[G][PE_T];
    const uint32_t t = threadIdx.x;
    const uint64_t chunk = blockIdx.x, c = c0 + blockIdx.z, jg = j0 + (uint64_t)blockIdx.y * G;
    const uint64_t base = chunk << chunk_log;
    const uint64_t rest = m - base, full = 1ull << chunk_log;
    const uint64_t len = rest < full ? rest : full;                    // the last chunk may be partial
    const Fe* __restrict__ src = coeffs + c * ld_in + base;
    Fe xT[G], acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint64_t j = jg + g < k ? jg + g : k - 1;
        Fe v = to_mont(points[j]);
#pragma unroll
        for (int b = 0; b < PE_LOG_T; ++b) {
            if (t == 0) pw[g][b] = v;
            v = mont_mul(v, v);
        }
        xT[g] = v;                                                     // x^T
        acc[g] = Fe{0, 0};
    }
    // thread t: coefficients t + s T, s = steps - 1 .. 0; only the top step can lie past the chunk's end (the per-thread tail)
    const uint64_t steps = (len + PE_T - 1) >> PE_LOG_T;
    const uint64_t top = t + (steps - 1) * PE_T;
    if (top < len) {
        const Fe a = src[top];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = a;
    }
    for (uint64_t s = steps - 1; s-- > 0;) {
        const Fe a = src[t + s * PE_T];
        pe_mul<G>(acc, xT);
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = fe_add(acc[g], a);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) red[g][t] = acc[g];
    __syncthreads();
    // sum_t a_t x^t: level h folds a_(t+h) x^h into a_t
#pragma unroll
    for (int b = PE_LOG_T - 1; b >= 0; --b) {
        const uint32_t h = 1u << b;
        if (t < h) {
#pragma unroll
            for (int g = 0; g < G; ++g) red[g][t] = fe_add(red[g][t], mont_mul(red[g][t + h], pw[g][b]));
        }
        __syncthreads();
    }
    if (t < G && jg + t < k) dst[c * dst_col + (jg + t) * dst_point + chunk] = red[t][0];
}

// Points across lanes.  grid = (chunks, waves of points, columns); lane l serves point j0 + PE_W * blockIdx.y + l < j1 (lanes past j1
// repeat the last point and are not stored).  The chunk's coefficients are read at wave-uniform addresses.
__global__ void __launch_bounds__(PE_W) pe_points_across_kernel(const Fe* __restrict__ coeffs, uint64_t m, uint64_t ld_in, const Fe* __restrict__ points, uint64_t j0, uint64_t j1,
                                                                 uint64_t c0, int chunk_log, Fe* __restrict__ dst, uint64_t dst_col, uint64_t dst_point) {
    const uint64_t chunk = blockIdx.x, c = c0 + blockIdx.z, j = j0 + (uint64_t)blockIdx.y * PE_W + threadIdx.x;
    const uint64_t base = chunk << chunk_log;
    const uint64_t rest = m - base, full = 1ull << chunk_log;
    const uint64_t len = rest < full ? rest : full;
    const Fe* __restrict__ src = coeffs + c * ld_in + base;
    const bool live = j < j1;
    const Fe x = to_mont(points[live ? j : j1 - 1]);
    const Fe x2 = mont_mul(x, x), x4 = mont_mul(x2, x2);
    const Fe y[PE_WAYS] = {x4, x4, x4, x4};
    // PE_WAYS independent Horner chains in x^4 over the coefficients 4 i + r (two mont_mul2 in flight instead of one dependent
    // product); only the top group can lie past the chunk's end
    const uint64_t groups = (len + PE_WAYS - 1) / PE_WAYS;
    const uint64_t top = (groups - 1) * PE_WAYS;
    Fe acc[PE_WAYS];
#pragma unroll
    for (int r = 0; r < PE_WAYS; ++r) acc[r] = top + r < len ? src[top + r] : Fe{0, 0};
    for (uint64_t i = groups - 1; i-- > 0;) {
        pe_mul<PE_WAYS>(acc, y);
#pragma unroll
        for (int r = 0; r < PE_WAYS; ++r) acc[r] = fe_add(acc[r], src[i * PE_WAYS + r]);
    }
    Fe v = acc[PE_WAYS - 1];                                           // a_0 + x (a_1 + x (a_2 + x a_3))
#pragma unroll
    for (int r = PE_WAYS - 2; r >= 0; --r) v = fe_add(mont_mul(v, x), acc[r]);
    if (live) dst[c * dst_col + j * dst_point + chunk] = v;
}

// out[c * ld_out + j] = sum_chunk partial[(c * k + j) * chunks + chunk] * y^chunk, y = points[j]^(2^chunk_log): one wave per output
// o = c * k + j (four per workgroup, outputs o0 + 4 * blockIdx.x + wave; o >= total repeats the last one and is not stored), lane l
// walks chunks l, l + 64, ... by Horner in y^64, then the tree of pe_coeffs_across_kernel over the wave's 64 accumulators.
__global__ void __launch_bounds__(4 * PE_W) pe_combine_kernel(const Fe* __restrict__ partial, uint64_t chunks, int chunk_log, const Fe* __restrict__ points, uint64_t k, uint64_t total,
                                                               uint64_t o0, Fe* __restrict__ out, uint64_t ld_out) {
    __shared__ Fe pw[4][PE_LOG_W];
    __shared__ Fe red[4 * PE_W];
    const uint32_t t = threadIdx.x, lane = t & (PE_W - 1), w = t >> PE_LOG_W;
    const uint64_t o = o0 + (uint64_t)blockIdx.x * 4 + w;
    const bool live = o < total;
    const uint64_t oo = live ? o : total - 1;
    const uint64_t c = oo / k, j = oo - c * k;
    Fe v = to_mont(points[j]);
    for (int s = 0; s < chunk_log; ++s) v = mont_mul(v, v);           // y
#pragma unroll
    for (int b = 0; b < PE_LOG_W; ++b) {
        if (lane == 0) pw[w][b] = v;
        v = mont_mul(v, v);
    }
    const Fe y64 = v;
    const Fe* __restrict__ src = partial + oo * chunks;
    const uint64_t steps = (chunks + PE_W - 1) >> PE_LOG_W;
    const uint64_t top = lane + (steps - 1) * PE_W;
    Fe acc = top < chunks ? src[top] : Fe{0, 0};
    for (uint64_t s = steps - 1; s-- > 0;) acc = fe_add(mont_mul(acc, y64), src[lane + s * PE_W]);
    red[t] = acc;
    __syncthreads();
#pragma unroll
    for (int b = PE_LOG_W - 1; b >= 0; --b) {
        const uint32_t h = 1u << b;
        if (lane < h) red[t] = fe_add(red[t], mont_mul(red[t + h], pw[w][b]));
        __syncthreads();
    }
    if (lane == 0 && live) out[c * ld_out + j] = red[t];
}

// m == 0: out[c * ld_out + j] = 0, j < k, c < cols (total = k * cols; nothing between the columns is written)
__global__ void __launch_bounds__(256) pe_zero_kernel(Fe* __restrict__ out, uint64_t ld_out, uint64_t k, uint64_t total, uint64_t o0) {
    const uint64_t o = o0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    const uint64_t c = o / k, j = o - c * k;
    out[c * ld_out + j] = Fe{0, 0};
}

}  // namespace sc

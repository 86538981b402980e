// Products, powers and products of many polynomials on the device: Polynomial.__mul__ (code/univariate.py:48-57) and
// Polynomial.__xor__ (code/univariate.py:140-150) for operands resident in HBM (model: tests/emu/poly_multiply_model.py).
//
// A result of `len` coefficients is computed at the smallest power of two n >= len (at least 2): zero-extending forward transforms,
// one pointwise step in the frequency domain, one inverse transform, the first `len` values stored.  n >= len, so the cyclic
// product IS the product.  The arithmetic is in the transforms between these kernels; the kernels are elementwise, one 16-byte
// element per lane (one 128-bit load and store), lanes along a column (unit stride), the column on grid.y: column c of a matrix
// lies at element c * ld.  One column is the same launch with grid.y = 1.  Nothing here is fused into a transform pass.
#pragma once
#include "field.cuh"

namespace sc {

#define PM_INDEX() ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x)

// frequency domain: out[c][i] = k * a[c][i] * b[c * ld_b + i], i < n   (c_m2 = k * R^2: undoes both Montgomery factors).
// ld_b == 0: one row of b for every column.  `out` may be `a` (every lane reads its own element before it stores it), which is why
// neither is __restrict__.  The pairs of a product tree are this kernel with b = a + pitch and ld_a = ld_b = 2 * pitch: row 2j
// times row 2j + 1 of the transformed matrix into row j of another one (out then is NOT a: row j would land on row 2j' of a
// neighbour); a square is b == a with ld_b == ld_a.
__global__ void __launch_bounds__(256) pm_mul_kernel(const Fe* a, uint64_t ld_a, const Fe* b, uint64_t ld_b, Fe* out, uint64_t ld_out, uint64_t n, Fe c_m2) {
    const uint64_t i = PM_INDEX();
    if (i >= n) return;
    const Fe x = a[blockIdx.y * ld_a + i], y = b[blockIdx.y * ld_b + i];
    out[blockIdx.y * ld_out + i] = mont_mul(mont_mul(x, y), c_m2);
}

// frequency domain: v[c][i] = k * v[c][i]^e, i < n, one exponent e >= 2 per launch: the square-and-multiply loop of mont_pow runs
// the same way in every lane.  k is passed as it is (no Montgomery factor): (v R)^e comes back as v^e R, and the last product
// with k drops the R.
__global__ void __launch_bounds__(256) pm_pow_kernel(Fe* __restrict__ v, uint64_t ld, uint64_t n, uint64_t e, Fe k) {
    const uint64_t i = PM_INDEX();
    if (i >= n) return;
    Fe* at = v + blockIdx.y * ld + i;
    *at = mont_mul(mont_pow(to_mont(*at), e), k);
}

// dst[c][i] = src[c][i], i < n: the first n coefficients of every column out of the transform's pitch into the caller's
__global__ void __launch_bounds__(256) pm_store_kernel(const Fe* __restrict__ src, uint64_t ld_src, Fe* __restrict__ dst, uint64_t ld_dst, uint64_t n) {
    const uint64_t i = PM_INDEX();
    if (i < n) dst[blockIdx.y * ld_dst + i] = src[blockIdx.y * ld_src + i];
}

}  // namespace sc

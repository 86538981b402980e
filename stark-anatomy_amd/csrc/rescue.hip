// rescue.hip -- the Rescue-Prime permutation (csrc/rescue_prime.cuh) over many inputs: the hash (code/rescue_prime.py:25-60) and the
// execution trace (:62-104) of the tutorial's signature scheme, one lane per input.
#include "core.h"
#include "rescue_prime.cuh"

namespace sci {

// One lane per input, no LDS: the permutation is a chain of ~4 000 paired Montgomery products in registers with one load and one
// (hash) or 55 (trace) stores per input.  The constants are the by-value argument P; the round index is uniform, so they are read
// with scalar loads.  TRACE: input k's register s at out[(2 k + s) * (rounds + 1) + t], t = 0..rounds -- one input's column is one run.
template <bool TRACE>
__global__ void __launch_bounds__(256) rescue_kernel(const Fe* __restrict__ in, uint64_t n, int rounds, RescueParams P, Fe* __restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (TRACE) rp_permute<true>(P, rounds, in[k], nullptr, out + k * RP_M * (uint64_t)(rounds + 1));
    else rp_permute<false>(P, rounds, in[k], out + k, nullptr);
}

static int rescue_launch(bool trace, const void* d_in, uint64_t n, const void* params, uint64_t rounds, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (rounds == 0 || rounds > (uint64_t)RP_MAX_ROUNDS) return fail(SC_ERR_BAD_ARG, "rescue prime: 1 .. 27 rounds expected");
    if (!params) return fail(SC_ERR_BAD_ARG, "rescue prime: null parameters");
    if (n && (!d_in || !d_out)) return fail(SC_ERR_BAD_ARG, "rescue prime: null buffer");
    if ((n + 255) / 256 > 0x7FFFFFFFull) return fail(SC_ERR_BAD_ARG, "rescue prime: too many inputs for one launch");
    RescueParams P;
    memset(&P, 0, sizeof P);
    const Fe* h = (const Fe*)params;                       // MDS (row-major), then 2 m rounds round constants, canonical
    const uint64_t count = RP_M * RP_M + 2 * RP_M * rounds;
    for (uint64_t i = 0; i < count; ++i) {
        Fe v{h[i].lo, h[i].hi};
        if (fe_ge_p(v)) return fail(SC_ERR_BAD_ARG, "rescue prime: a constant is not below p");
        v = to_mont(v);
        if (i < RP_M * RP_M) P.mds[i] = v;
        else P.rc[i - RP_M * RP_M] = v;
    }
    if (!n) return SC_OK;
    hipStream_t st = pick_stream(stream);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (trace) hipLaunchKernelGGL(rescue_kernel<true>, grid, dim3(256), 0, st, (const Fe*)d_in, n, (int)rounds, P, (Fe*)d_out);
    else hipLaunchKernelGGL(rescue_kernel<false>, grid, dim3(256), 0, st, (const Fe*)d_in, n, (int)rounds, P, (Fe*)d_out);
    HIPCHK(hipGetLastError());
    return SC_OK;
}

}  // namespace sci

int sc_rescue_prime_hash_dev(const void* d_in, uint64_t n, const void* params, uint64_t rounds, void* d_out, void* stream) {
    return rescue_launch(false, d_in, n, params, rounds, d_out, stream);
}
int sc_rescue_prime_trace_dev(const void* d_in, uint64_t n, const void* params, uint64_t rounds, void* d_out, void* stream) {
    return rescue_launch(true, d_in, n, params, rounds, d_out, stream);
}

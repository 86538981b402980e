// rescue.hip -- the Rescue-Prime permutation (csrc/rescue_prime.cuh) over many inputs: the hash (code/rescue_prime.py:25-60) and the
// execution trace (:62-104) of the tutorial's signature scheme, one lane per input; and the same permutation at any state width
// 2 .. 8 as a permutation, a sponge and all states.
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

// The same permutation at any width 2 .. 8 (rp_sponge_w): one lane per input, the state in registers, the constants `C` in memory
// at wave-uniform addresses.  Coalesced: element j of input k at in[j * ld_in + k], register j of its result at out[j * ld_out + k].
// TRACE: input k's register s at out[(M k + s) * (rounds + 1) + t] instead.  Four waves per SIMD: the widest state then stays inside
// 128 VGPRs without scratch (tools/kernel_regs.py rescue_wide; left alone, hipcc takes 132 at M = 8 and loses the fourth wave).
template <int M, bool TRACE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
rescue_wide_kernel(const Fe* __restrict__ C, int rounds, const Fe* in, uint64_t ld_in, uint64_t blocks, int rate, Fe* out, uint64_t ld_out, int out_len, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (TRACE) rp_sponge_w<M, true>(C, rounds, in + k, ld_in, 1, rate, nullptr, 0, 0, out + k * M * (uint64_t)(rounds + 1));
    else rp_sponge_w<M, false>(C, rounds, in + k, ld_in, blocks, rate, out + k, ld_out, out_len, nullptr);
}

enum WideKind { WIDE_PERMUTE, WIDE_SPONGE, WIDE_TRACE };
struct WideCall {
    WideKind kind;
    const void* d_in;
    uint64_t ld_in;
    void* d_out;
    uint64_t ld_out;
    uint64_t blocks, rate, out_len;   // what the kernel runs: a plain permutation is one block of rate m with every register stored
    uint64_t n, m, rounds;
};

template <int M>
static void rescue_wide_enqueue(const WideCall& c, const Fe* C, hipStream_t st) {
    const dim3 grid((unsigned)((c.n + 255) / 256));
    if (c.kind == WIDE_TRACE) hipLaunchKernelGGL((rescue_wide_kernel<M, true>), grid, dim3(256), 0, st, C, (int)c.rounds, (const Fe*)c.d_in, c.ld_in, c.blocks, (int)c.rate, (Fe*)c.d_out, c.ld_out, (int)c.out_len, c.n);
    else hipLaunchKernelGGL((rescue_wide_kernel<M, false>), grid, dim3(256), 0, st, C, (int)c.rounds, (const Fe*)c.d_in, c.ld_in, c.blocks, (int)c.rate, (Fe*)c.d_out, c.ld_out, (int)c.out_len, c.n);
}

// Checks everything, then stages the constants (Montgomery form) in a block of the call's own -- filled by kernel arguments
// (upload_small: the launch copies them, nothing is staged on the host and nothing is waited for) and handed back to the pool
// behind the streams in use -- and enqueues the one launch.
static int rescue_wide_launch(const WideCall& c, const void* params, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    const bool trace = c.kind == WIDE_TRACE;
    const std::string what = std::string("rescue prime ") + (trace ? "trace states: " : c.kind == WIDE_SPONGE ? "sponge: " : "permute: ");
    if (c.m < 2 || c.m > (uint64_t)RP_MAX_M) return fail(SC_ERR_BAD_ARG, what + "a state width of 2 .. 8 expected");
    if (c.rounds == 0 || c.rounds > (uint64_t)RP_MAX_ROUNDS) return fail(SC_ERR_BAD_ARG, what + "1 .. 27 rounds expected");
    if (c.kind == WIDE_SPONGE) {
        if (c.rate == 0 || c.rate >= c.m) return fail(SC_ERR_BAD_ARG, what + "a rate of 1 .. m - 1 expected");
        if (c.out_len == 0 || c.out_len > c.rate) return fail(SC_ERR_BAD_ARG, what + "an output length of 1 .. rate expected");
        if (c.blocks == 0) return fail(SC_ERR_BAD_ARG, what + "at least one block expected");
    }
    if (!params) return fail(SC_ERR_BAD_ARG, what + "null parameters");
    if (c.n && (!c.d_in || !c.d_out)) return fail(SC_ERR_BAD_ARG, what + "null buffer");
    if (c.ld_in < c.n || (!trace && c.ld_out < c.n)) return fail(SC_ERR_BAD_ARG, what + "a stride below n");
    if ((c.n + 255) / 256 > 0x7FFFFFFFull) return fail(SC_ERR_BAD_ARG, what + "too many inputs for one launch");
    if (c.n) {
        // the bytes read and the bytes written (128-bit sums: no stride or block count can wrap them)
        const u128 in_bytes = (((u128)c.blocks * c.rate - 1) * c.ld_in + c.n) * sizeof(Fe);
        const u128 out_bytes = (trace ? (u128)c.m * c.n * (c.rounds + 1) : ((u128)c.out_len - 1) * c.ld_out + c.n) * sizeof(Fe);
        const u128 a = (uintptr_t)c.d_in, b = (uintptr_t)c.d_out;
        const bool in_place = c.kind == WIDE_PERMUTE && c.d_in == c.d_out && c.ld_in == c.ld_out;     // every element is read by the lane that writes it
        if (a < b + out_bytes && b < a + in_bytes && !in_place) return fail(SC_ERR_BAD_ARG, what + "the output overlaps the input");
    }
    const uint64_t count = c.m * c.m + 2 * c.m * c.rounds;
    Fe host[RP_MAX_M * RP_MAX_M + 2 * RP_MAX_M * RP_MAX_ROUNDS];
    const Fe* h = (const Fe*)params;                       // MDS (row-major), then 2 m rounds round constants, canonical
    for (uint64_t i = 0; i < count; ++i) {
        const Fe v{h[i].lo, h[i].hi};
        if (fe_ge_p(v)) return fail(SC_ERR_BAD_ARG, what + "a constant is not below p");
        host[i] = to_mont(v);
    }
    if (!c.n) return SC_OK;
    hipStream_t st = pick_stream(stream);
    PoolTmpAsync block;
    SCCHK(block.get(sizeof host));
    if (!upload_small(block.p, host, count * sizeof(Fe), st)) return fail(SC_ERR_HIP, what + "the constants could not be enqueued");
    switch (c.m) {
        case 2: rescue_wide_enqueue<2>(c, block.fe(), st); break;
        case 3: rescue_wide_enqueue<3>(c, block.fe(), st); break;
        case 4: rescue_wide_enqueue<4>(c, block.fe(), st); break;
        case 5: rescue_wide_enqueue<5>(c, block.fe(), st); break;
        case 6: rescue_wide_enqueue<6>(c, block.fe(), st); break;
        case 7: rescue_wide_enqueue<7>(c, block.fe(), st); break;
        default: rescue_wide_enqueue<8>(c, block.fe(), st); break;
    }
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

int sc_rescue_prime_permute_dev(const void* d_in, uint64_t ld_in, void* d_out, uint64_t ld_out, uint64_t n, uint64_t m,
                                const void* params, uint64_t rounds, void* stream) {
    return rescue_wide_launch(WideCall{WIDE_PERMUTE, d_in, ld_in, d_out, ld_out, 1, m, m, n, m, rounds}, params, stream);
}
int sc_rescue_prime_sponge_dev(const void* d_msg, uint64_t ld_msg, uint64_t blocks, void* d_out, uint64_t ld_out, uint64_t out_len,
                               uint64_t n, uint64_t m, uint64_t rate, const void* params, uint64_t rounds, void* stream) {
    return rescue_wide_launch(WideCall{WIDE_SPONGE, d_msg, ld_msg, d_out, ld_out, blocks, rate, out_len, n, m, rounds}, params, stream);
}
int sc_rescue_prime_trace_states_dev(const void* d_in, uint64_t ld_in, uint64_t n, uint64_t m, const void* params, uint64_t rounds,
                                     void* d_out, void* stream) {
    return rescue_wide_launch(WideCall{WIDE_TRACE, d_in, ld_in, d_out, 0, 1, m, 0, n, m, rounds}, params, stream);
}

// CPU build of the Rescue-Prime permutation: the SAME rp_permute the HIP kernel runs (csrc/rescue_prime.cuh), compiled by g++ with the
// portable field arithmetic, one input at a time.  Test infrastructure (built by tests/test_rescue_prime_cpu.py).
#include <cstdint>
#include <cstring>
#include "../../stark-anatomy_amd/csrc/rescue_prime.cuh"

using namespace sc;

static RescueParams load(const void* params, int rounds) {
    RescueParams P;
    memset(&P, 0, sizeof P);
    const Fe* h = (const Fe*)params;
    for (int i = 0; i < RP_M * RP_M; ++i) P.mds[i] = to_mont(h[i]);
    for (int i = 0; i < 2 * RP_M * rounds; ++i) P.rc[i] = to_mont(h[RP_M * RP_M + i]);
    return P;
}

extern "C" {
// out[k] = hash of in[k]
void emu_rescue_hash(const void* in, uint64_t n, const void* params, int rounds, void* out) {
    const RescueParams P = load(params, rounds);
    for (uint64_t k = 0; k < n; ++k) rp_permute<false>(P, rounds, ((const Fe*)in)[k], (Fe*)out + k, nullptr);
}
// the kernel's trace layout: input k's register s at out[(2 k + s) * (rounds + 1) + t]
void emu_rescue_trace(const void* in, uint64_t n, const void* params, int rounds, void* out) {
    const RescueParams P = load(params, rounds);
    for (uint64_t k = 0; k < n; ++k) rp_permute<true>(P, rounds, ((const Fe*)in)[k], nullptr, (Fe*)out + k * RP_M * (rounds + 1));
}
}

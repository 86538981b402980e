// CPU build of the generic-width Rescue-Prime code: the SAME rp_sponge_w the HIP kernels run (csrc/rescue_prime.cuh), compiled by
// g++ with the portable field arithmetic, one input after the other.  Test infrastructure (built by tests/test_rescue_wide_cpu.py;
// with RESCUE_WIDE_MAIN a stand-alone program that the same test builds with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../stark-anatomy_amd/csrc/rescue_prime.cuh"

using namespace sc;

// the constants as the kernels read them: m * m + 2 * m * rounds words, Montgomery form
static std::vector<Fe> load(const void* params, int m, int rounds) {
    const Fe* h = (const Fe*)params;
    std::vector<Fe> C(m * m + 2 * m * rounds);
    for (size_t i = 0; i < C.size(); ++i) C[i] = to_mont(h[i]);
    return C;
}

template <int M>
static void run(bool trace, const Fe* C, int rounds, const Fe* in, uint64_t ld_in, uint64_t blocks, int rate, Fe* out, uint64_t ld_out,
                int out_len, uint64_t n) {
    for (uint64_t k = 0; k < n; ++k) {
        if (trace) rp_sponge_w<M, true>(C, rounds, in + k, ld_in, 1, rate, nullptr, 0, 0, out + k * M * (uint64_t)(rounds + 1));
        else rp_sponge_w<M, false>(C, rounds, in + k, ld_in, blocks, rate, out + k, ld_out, out_len, nullptr);
    }
}

static int dispatch(bool trace, int m, const void* params, int rounds, const void* in, uint64_t ld_in, uint64_t blocks, int rate, void* out,
                    uint64_t ld_out, int out_len, uint64_t n) {
    if (m < 2 || m > RP_MAX_M || rounds < 1 || rounds > RP_MAX_ROUNDS) return -1;
    const std::vector<Fe> C = load(params, m, rounds);
    const Fe* i = (const Fe*)in;
    Fe* o = (Fe*)out;
    switch (m) {
        case 2: run<2>(trace, C.data(), rounds, i, ld_in, blocks, rate, o, ld_out, out_len, n); break;
        case 3: run<3>(trace, C.data(), rounds, i, ld_in, blocks, rate, o, ld_out, out_len, n); break;
        case 4: run<4>(trace, C.data(), rounds, i, ld_in, blocks, rate, o, ld_out, out_len, n); break;
        case 5: run<5>(trace, C.data(), rounds, i, ld_in, blocks, rate, o, ld_out, out_len, n); break;
        case 6: run<6>(trace, C.data(), rounds, i, ld_in, blocks, rate, o, ld_out, out_len, n); break;
        case 7: run<7>(trace, C.data(), rounds, i, ld_in, blocks, rate, o, ld_out, out_len, n); break;
        default: run<8>(trace, C.data(), rounds, i, ld_in, blocks, rate, o, ld_out, out_len, n); break;
    }
    return 0;
}

extern "C" {
// what sc_rescue_prime_sponge_dev computes; a plain permutation (sc_rescue_prime_permute_dev) is blocks = 1, rate = out_len = m
int emu_wide_sponge(int m, const void* in, uint64_t ld_in, uint64_t blocks, int rate, void* out, uint64_t ld_out, int out_len, uint64_t n,
                    const void* params, int rounds) {
    return dispatch(false, m, params, rounds, in, ld_in, blocks, rate, out, ld_out, out_len, n);
}
// what sc_rescue_prime_trace_states_dev computes: register s of input k's state t at out[(m k + s) * (rounds + 1) + t]
int emu_wide_trace(int m, const void* in, uint64_t ld_in, uint64_t n, const void* params, int rounds, void* out) {
    return dispatch(true, m, params, rounds, in, ld_in, 1, m, out, 0, 0, n);
}
}

#ifdef RESCUE_WIDE_MAIN
// Every width on heap buffers of exactly the size the layout promises (a sanitizer build reports any access past them), strided
// and in place.  Self-checks that need no model: an input and the same input plus p permute alike, in place equals out of place,
// the last state of the trace is the permutation, and a sponge of one block is the permutation of the block over a zero capacity.
static bool same(const Fe* a, const Fe* b, size_t count) { return memcmp(a, b, count * sizeof(Fe)) == 0; }

int main() {
    const int rounds = 2;
    for (int m = 2; m <= RP_MAX_M; ++m) {
        const uint64_t n = 5, ld = n + 3;
        std::vector<Fe> params(m * m + 2 * m * rounds);
        for (size_t i = 0; i < params.size(); ++i) params[i] = Fe{0x9E3779B97F4A7C15ull * (i + 1), (0x1234567ull * (i + m)) << 20};   // far below p (top limb under 2^52)
        std::vector<Fe> in((m - 1) * ld + n), shifted(in.size()), out((m - 1) * n + n), out2(out.size());
        for (size_t i = 0; i < in.size(); ++i) {
            in[i] = Fe{i * 7 + 1, i << 8};
            shifted[i] = Fe{in[i].lo + P_LO, in[i].hi + P_HI};
        }
        if (emu_wide_sponge(m, in.data(), ld, 1, m, out.data(), n, m, n, params.data(), rounds)) return 1;
        emu_wide_sponge(m, shifted.data(), ld, 1, m, out2.data(), n, m, n, params.data(), rounds);
        if (!same(out.data(), out2.data(), out.size())) return printf("m = %d: x and x + p differ\n", m), 2;
        emu_wide_sponge(m, shifted.data(), ld, 1, m, shifted.data(), ld, m, n, params.data(), rounds);      // in place
        for (int s = 0; s < m; ++s)
            if (!same(shifted.data() + s * ld, out.data() + s * n, n)) return printf("m = %d: in place differs\n", m), 3;
        std::vector<Fe> trace(m * n * (rounds + 1));
        emu_wide_trace(m, in.data(), ld, n, params.data(), rounds, trace.data());
        for (uint64_t k = 0; k < n; ++k)
            for (int s = 0; s < m; ++s)
                if (!same(&trace[(m * k + s) * (rounds + 1) + rounds], &out[s * n + k], 1)) return printf("m = %d: trace end differs\n", m), 4;
        for (int rate = 1; rate < m; ++rate) {
            std::vector<Fe> msg((rate - 1) * ld + n), full((m - 1) * n + n, fe_zero()), digest((rate - 1) * n + n), want(full.size());
            for (int j = 0; j < rate; ++j)
                for (uint64_t k = 0; k < n; ++k) msg[j * ld + k] = full[j * n + k] = in[j * ld + k];
            emu_wide_sponge(m, msg.data(), ld, 1, rate, digest.data(), n, rate, n, params.data(), rounds);
            emu_wide_sponge(m, full.data(), n, 1, m, want.data(), n, m, n, params.data(), rounds);
            if (!same(digest.data(), want.data(), digest.size())) return printf("m = %d rate = %d: sponge differs\n", m, rate), 5;
        }
    }
    printf("rescue wide ok\n");
    return 0;
}
#endif

// grind.cuh -- proof-of-work grinding on the Fiat-Shamir transcript: one trial of the search as a lane function, and the kernel that
// runs one window of trials.
//
// The protocol (stark-anatomy_amd/grinding.py is the host specification):
//   pow_value(seed, nonce) = little-endian u64 of SHAKE-256(seed(32 bytes) || nonce(8 bytes, little-endian)).digest(8)
//   nonce is accepted at `bits` iff pow_value >> (64 - bits) == 0,  1 <= bits <= 63
// The 40-byte message fits SHAKE-256's 136-byte rate, so ONE trial is ONE Keccak-f[1600]: state words 0 .. 3 = the seed, word 4 =
// the nonce, word 5 = 0x1f (the domain suffix behind the message), word 16 = 1 << 63 (the last bit of the padding in byte 135), all
// others 0; pow_value is word 0 of the permuted state.
//
// One lane runs one trial with the whole state in registers (25 words, 50 VGPRs; the four seed words are wave-uniform and what
// depends on them alone is scalar work).  Two prunings, both by writing the first and the last round apart from the loop:
//   round 0   its input is written out as constants and zeros, so the compiler folds theta's column sums over the 18 zero words and
//             rho/pi of the words that are zero or constant;
//   round 23  only word 0 of the output is wanted: theta's five column sums, three words through rho, one chi (grind_last_round).
// Rounds 1 .. 22 are one loop whose body is a whole round; GRIND_UNROLLED instantiates it fully unrolled instead (A/B:
// sc_set_tuning("grind_unrolled")).
//
// The lane function compiles with g++ as well (tests/emu/grind_emu.cpp runs it against hashlib).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SC_GRIND_HD __host__ __device__ __forceinline__
#else
#define SC_GRIND_HD inline
#endif

namespace sc {

struct GrindTables {
    uint64_t rc[24];
};
// (a function-local constexpr table: the same object on the host and on the device)
SC_GRIND_HD uint64_t grind_rc(int round) {
    constexpr GrindTables T = {{0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
                                0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
                                0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
                                0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                                0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull}};
    return T.rc[round];
}

template <int N>
SC_GRIND_HD uint64_t grind_rotl(uint64_t x) {
    if (N == 0) return x;
#if defined(__HIP_DEVICE_COMPILE__)
    // two v_alignbit_b32 (the low dword of a 64-bit pair shifted right) instead of the two 64-bit shifts and the ors hipcc makes of the line below
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (N == 32) return ((uint64_t)lo << 32) | hi;
    constexpr uint32_t R = 32 - (N & 31);
    const uint32_t a = __builtin_amdgcn_alignbit(hi, lo, R), b = __builtin_amdgcn_alignbit(lo, hi, R);
    return N < 32 ? ((uint64_t)a << 32) | b : ((uint64_t)b << 32) | a;
#else
    return (x << (N & 63)) | (x >> ((64 - N) & 63));
#endif
}

// one round of Keccak-f[1600] on s[x + 5 y]; every index and rotation is a literal
SC_GRIND_HD void grind_round(uint64_t (&s)[25], uint64_t rc) {
    const uint64_t c0 = s[0] ^ s[5] ^ s[10] ^ s[15] ^ s[20], c1 = s[1] ^ s[6] ^ s[11] ^ s[16] ^ s[21], c2 = s[2] ^ s[7] ^ s[12] ^ s[17] ^ s[22],
                   c3 = s[3] ^ s[8] ^ s[13] ^ s[18] ^ s[23], c4 = s[4] ^ s[9] ^ s[14] ^ s[19] ^ s[24];
    const uint64_t d0 = c4 ^ grind_rotl<1>(c1), d1 = c0 ^ grind_rotl<1>(c2), d2 = c1 ^ grind_rotl<1>(c3), d3 = c2 ^ grind_rotl<1>(c4), d4 = c3 ^ grind_rotl<1>(c0);
    // theta, rho and pi: b[y + 5 ((2 x + 3 y) % 5)] = rotl(s[x + 5 y] ^ d[x], ROT[x + 5 y])
    uint64_t b[25];
    b[0] = s[0] ^ d0;                    b[10] = grind_rotl<1>(s[1] ^ d1);    b[20] = grind_rotl<62>(s[2] ^ d2);   b[5] = grind_rotl<28>(s[3] ^ d3);    b[15] = grind_rotl<27>(s[4] ^ d4);
    b[16] = grind_rotl<36>(s[5] ^ d0);   b[1] = grind_rotl<44>(s[6] ^ d1);    b[11] = grind_rotl<6>(s[7] ^ d2);    b[21] = grind_rotl<55>(s[8] ^ d3);   b[6] = grind_rotl<20>(s[9] ^ d4);
    b[7] = grind_rotl<3>(s[10] ^ d0);    b[17] = grind_rotl<10>(s[11] ^ d1);  b[2] = grind_rotl<43>(s[12] ^ d2);   b[12] = grind_rotl<25>(s[13] ^ d3);  b[22] = grind_rotl<39>(s[14] ^ d4);
    b[23] = grind_rotl<41>(s[15] ^ d0);  b[8] = grind_rotl<45>(s[16] ^ d1);   b[18] = grind_rotl<15>(s[17] ^ d2);  b[3] = grind_rotl<21>(s[18] ^ d3);   b[13] = grind_rotl<8>(s[19] ^ d4);
    b[14] = grind_rotl<18>(s[20] ^ d0);  b[24] = grind_rotl<2>(s[21] ^ d1);   b[9] = grind_rotl<61>(s[22] ^ d2);   b[19] = grind_rotl<56>(s[23] ^ d3);  b[4] = grind_rotl<14>(s[24] ^ d4);
    // chi
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int y = 0; y < 25; y += 5) {
        s[y + 0] = b[y + 0] ^ (~b[y + 1] & b[y + 2]);
        s[y + 1] = b[y + 1] ^ (~b[y + 2] & b[y + 3]);
        s[y + 2] = b[y + 2] ^ (~b[y + 3] & b[y + 4]);
        s[y + 3] = b[y + 3] ^ (~b[y + 4] & b[y + 0]);
        s[y + 4] = b[y + 4] ^ (~b[y + 0] & b[y + 1]);
    }
    s[0] ^= rc;
}

// word 0 of the state after one more round: b[0], b[1], b[2] come from s[0], s[6], s[12]
SC_GRIND_HD uint64_t grind_last_round(const uint64_t (&s)[25], uint64_t rc) {
    const uint64_t c0 = s[0] ^ s[5] ^ s[10] ^ s[15] ^ s[20], c1 = s[1] ^ s[6] ^ s[11] ^ s[16] ^ s[21], c2 = s[2] ^ s[7] ^ s[12] ^ s[17] ^ s[22],
                   c3 = s[3] ^ s[8] ^ s[13] ^ s[18] ^ s[23], c4 = s[4] ^ s[9] ^ s[14] ^ s[19] ^ s[24];
    const uint64_t b0 = s[0] ^ c4 ^ grind_rotl<1>(c1), b1 = grind_rotl<44>(s[6] ^ c0 ^ grind_rotl<1>(c2)), b2 = grind_rotl<43>(s[12] ^ c1 ^ grind_rotl<1>(c3));
    return b0 ^ (~b1 & b2) ^ rc;
}

// pow_value(seed, nonce): seed as four little-endian words
template <bool UNROLLED>
SC_GRIND_HD uint64_t grind_pow_value(uint64_t s0, uint64_t s1, uint64_t s2, uint64_t s3, uint64_t nonce) {
    uint64_t s[25] = {s0, s1, s2, s3, nonce, 0x1full, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1ull << 63, 0, 0, 0, 0, 0, 0, 0, 0};
    grind_round(s, grind_rc(0));
    if (UNROLLED) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int round = 1; round < 23; ++round) grind_round(s, grind_rc(round));
    } else {
#if defined(__HIPCC__)
#pragma clang loop unroll(disable)
#endif
        for (int round = 1; round < 23; ++round) grind_round(s, grind_rc(round));
    }
    return grind_last_round(s, grind_rc(23));
}

SC_GRIND_HD bool grind_accepts(uint64_t value, int bits) { return (value >> (64 - bits)) == 0; }

constexpr uint64_t GRIND_NONE = ~0ull;       // a member's word before any accepted trial: no offset from `start` reaches it (grind.hip)

#if defined(__HIPCC__)
// One window of trials for the members listed in `order` (blockIdx.y): the nonces start + o for o in [base, base + window), base +
// window - 1 <= the last offset of the search, so start + o never passes 2^64 - 1.  best[m]: the smallest accepted OFFSET of member m so
// far (GRIND_NONE: none), lowered with a 64-bit atomic minimum -- the minimum of a set does not depend on the order of the updates, so
// the word after the launch is the same in every run.  A lane walks the window in ascending strides and leaves once its offset is
// above the member's word (nothing behind it can lower the minimum); the launch writes nothing else and waits for nothing.
template <bool UNROLLED>
__global__ void __launch_bounds__(256) grind_window_kernel(const uint64_t* __restrict__ seeds, const uint32_t* __restrict__ order, uint64_t* best,
                                                           uint64_t start, uint64_t base, uint64_t window, int bits) {
    const uint32_t m = order[blockIdx.y];
    const uint64_t s0 = seeds[4 * (uint64_t)m], s1 = seeds[4 * (uint64_t)m + 1], s2 = seeds[4 * (uint64_t)m + 2], s3 = seeds[4 * (uint64_t)m + 3];
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < window; w += stride) {
        const uint64_t o = base + w;
        if (o > __hip_atomic_load(best + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        if (grind_accepts(grind_pow_value<UNROLLED>(s0, s1, s2, s3, start + o), bits)) atomicMin((unsigned long long*)(best + m), (unsigned long long)o);
    }
}
#endif

}  // namespace sc

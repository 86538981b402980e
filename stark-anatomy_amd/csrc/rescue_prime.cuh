// rescue_prime.cuh -- the Rescue-Prime permutation of the tutorial's signature scheme (reference code/rescue_prime.py:25-60 hash,
// :62-104 trace) for state width m = 2 (rate 1, capacity 1), alpha = 3, one lane per input.
//
// Host-and-device code like field.cuh: g++ compiles the same functions for the CPU emulation test (tests/emu/rescue_emu.cpp), hipcc
// for rescue_kernel (csrc/rescue.hip).  Everything runs in the Montgomery domain: the input is converted once on load, every value
// stored is converted back, and the MDS matrix and the round constants arrive in Montgomery form, so a product of a state value and
// a constant is one mont_mul and a round constant is one fe_add.
//
// Modular products per hash (N = 27 rounds): per round and state element 2 for x^3 and 142 for x^alphainv (below), plus the two
// 2 x 2 matrix products (8 per round): (2 * 144 + 8) * 27 = 7 992, and 2 conversions (in, out) = 7 994.  The trace converts each
// of its 28 states but the first back (2 * 27 instead of 1).  Both state elements go through mont_mul2 side by side: one lane, two
// independent chains.
#pragma once
#include "field.cuh"

namespace sc {

constexpr int RP_M = 2;                   // state width (the ABI fixes it)
constexpr int RP_MAX_ROUNDS = 27;         // the reference's N; the kernel-argument struct holds the constants of up to this many rounds

// The constants as one by-value kernel argument (1 792 bytes): every lane reads the same words, so they stay in SGPRs.
struct RescueParams {
    Fe mds[RP_M * RP_M];                          // row-major, Montgomery form
    Fe rc[2 * RP_M * RP_MAX_ROUNDS];              // round r: [2 r m, 2 r m + m) after the cube, [2 r m + m, 2 (r + 1) m) after the inverse
};

// a, b <- a^(2^n), b^(2^n)
SC_HD void rp_sqr2_n(Fe& a, Fe& b, int n) {
    for (int i = 0; i < n; ++i) mont_mul2(a, a, b, b, a, b);
}
// a, b <- a^(4^k) * a0, b^(4^k) * b0  (one step of the block chain below)
SC_HD void rp_block2(Fe& a, Fe& b, Fe a0, Fe b0, int k) {
    rp_sqr2_n(a, b, 2 * k);
    mont_mul2(a, a0, b, b0, a, b);
}

// (a, b) <- (a^3, b^3)
SC_HD void rp_cube2(Fe& a, Fe& b) {
    Fe a2, b2;
    mont_mul2(a, a, b, b, a2, b2);
    mont_mul2(a2, a, b2, b, a, b);
}

// (a, b) <- (a^alphainv, b^alphainv), alphainv = 3^-1 mod (p - 1) = (2p - 1) / 3, by an addition chain.
// With B = B_59 = (4^59 - 1) / 3 = 0101...01b (59 pairs):  alphainv = 1628 B + 543  (since 2^119 = 6 B + 2, alphainv = 271 * 2^119 +
// 2 B + 1).  x^(B_k) for B_k = (4^k - 1) / 3 doubles like a repunit: B_(i+j) = 4^j B_i + B_j, so x^(B_(i+j)) = (x^(B_i))^(4^j) * x^(B_j)
// along the addition chain 1, 2, 3, 5, 7, 14, 28, 56, 59 of k (116 squarings, 8 products).  Then 1628 = 11001011100b and 543 =
// 1000011111b are read together, bit by bit, as the base-2 digits B * bit(1628) + bit(543) -- digits x^B, x^(B+1) or x^1
// (10 squarings, 7 products, plus 1 for x^(B+1)).  In all 126 squarings and 16 products = 142 modular products, where
// square-and-multiply over the 128 bits (65 of them set) takes 127 + 64 = 191.
SC_HD void rp_invcube2(Fe& a, Fe& b) {
    const Fe a1 = a, b1 = b;                                   // B_1
    Fe a2 = a, b2 = b;  rp_block2(a2, b2, a1, b1, 1);          // B_2 = 4 B_1 + B_1
    Fe a3 = a2, b3 = b2; rp_block2(a3, b3, a1, b1, 1);         // B_3 = 4 B_2 + B_1
    Fe a5 = a3, b5 = b3; rp_block2(a5, b5, a2, b2, 2);         // B_5 = 4^2 B_3 + B_2
    Fe ac = a5, bc = b5; rp_block2(ac, bc, a2, b2, 2);         // B_7
    rp_block2(ac, bc, ac, bc, 7);                              // B_14 (the multiplier is read before the squarings: by value)
    rp_block2(ac, bc, ac, bc, 14);                             // B_28
    rp_block2(ac, bc, ac, bc, 28);                             // B_56
    rp_block2(ac, bc, a3, b3, 3);                              // B_59 = 4^3 B_56 + B_3
    const Fe ay = ac, by = bc;                                 // y = x^B
    Fe az, bz;
    mont_mul2(ay, a1, by, b1, az, bz);                         // z = x^(B + 1)
    // digits from bit 10 down to bit 0: y (leading), z, -, -, y, -, z, z, z, x, x
    rp_sqr2_n(ac, bc, 1); mont_mul2(ac, az, bc, bz, ac, bc);   // bit 9: z
    rp_sqr2_n(ac, bc, 3); mont_mul2(ac, ay, bc, by, ac, bc);   // bits 8, 7: none; bit 6: y
    rp_sqr2_n(ac, bc, 2); mont_mul2(ac, az, bc, bz, ac, bc);   // bit 5: none; bit 4: z
    rp_sqr2_n(ac, bc, 1); mont_mul2(ac, az, bc, bz, ac, bc);   // bit 3: z
    rp_sqr2_n(ac, bc, 1); mont_mul2(ac, az, bc, bz, ac, bc);   // bit 2: z
    rp_sqr2_n(ac, bc, 1); mont_mul2(ac, a1, bc, b1, ac, bc);   // bit 1: x
    rp_sqr2_n(ac, bc, 1); mont_mul2(ac, a1, bc, b1, a, b);     // bit 0: x
}

// the 2 x 2 matrix product, then the round constants c0, c1 added (all Montgomery form)
SC_HD void rp_mix(const RescueParams& P, Fe& a, Fe& b, Fe c0, Fe c1) {
    Fe t00, t01, t10, t11;
    mont_mul2(P.mds[0], a, P.mds[1], b, t00, t01);
    mont_mul2(P.mds[2], a, P.mds[3], b, t10, t11);
    a = fe_add(fe_add(t00, t01), c0);
    b = fe_add(fe_add(t10, t11), c1);
}

// One round (code/rescue_prime.py:31-57): cube, mix, constants; inverse cube, mix, constants.
SC_HD void rp_round(const RescueParams& P, int r, Fe& a, Fe& b) {
    rp_cube2(a, b);
    rp_mix(P, a, b, P.rc[4 * r + 0], P.rc[4 * r + 1]);
    rp_invcube2(a, b);
    rp_mix(P, a, b, P.rc[4 * r + 2], P.rc[4 * r + 3]);
}

// The permutation of one input x (any 128-bit value: it is reduced mod p first).  TRACE: every state 0..rounds, register s of state t at trace[s * (rounds + 1) + t]
// (canonical); otherwise *hash_out = state[0] after the last round.
template <bool TRACE>
SC_HD void rp_permute(const RescueParams& P, int rounds, Fe x, Fe* hash_out, Fe* trace) {
    if (fe_ge_p(x)) x = Fe{x.lo - P_LO, x.hi - P_HI - (x.lo < P_LO)};    // x mod p (x < 2^128 < 2p)
    Fe a = to_mont(x), b = fe_zero();
    if (TRACE) {
        trace[0] = x;
        trace[rounds + 1] = fe_zero();
    }
    for (int r = 0; r < rounds; ++r) {
        rp_round(P, r, a, b);
        if (TRACE) {
            Fe ca, cb;
            mont_mul2(a, fe_one(), b, fe_one(), ca, cb);    // from_mont of both
            trace[r + 1] = ca;
            trace[rounds + 1 + r + 1] = cb;
        }
    }
    if (!TRACE) *hash_out = from_mont(a);
}

}  // namespace sc

// rescue_prime.cuh -- the Rescue-Prime permutation of the tutorial's signature scheme (reference code/rescue_prime.py:25-60 hash,
// :62-104 trace) for state width m = 2 (rate 1, capacity 1), alpha = 3, one lane per input; below it the same permutation for any
// width 2 .. 8 with its constants in memory (permutation, sponge, all states).
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

// ---- any state width 2 <= M <= 8 (sc_rescue_prime_permute_dev / _sponge_dev / _trace_states_dev) ---------------------------------
//
// The same permutation for a compile-time width M: one lane per input, the M state elements in registers, alpha = 3.  The state goes
// through rp_cube2 / rp_invcube2 two elements at a time; an odd width leaves one element over, which takes the one-chain forms
// below (the same addition chain through mont_mul).  Modular products per permutation: per round and element 2 + 142, and two
// M x M matrix products: (144 M + 2 M^2) * rounds (M = 2, 27 rounds: the 7 992 above), plus one conversion per element loaded or stored.
//
// The constants no longer fit a kernel argument (M = 8, 27 rounds: 64 + 432 elements, 7 936 bytes): they are read from memory, at
// addresses every lane of a wave shares (scalar loads on the device).  `C`: M * M matrix entries, row-major, then 2 M rounds round
// constants (round r: [2 r M, 2 r M + M) after the cube, [2 r M + M, 2 (r + 1) M) after the inverse cube), all in Montgomery form.
//
// Register pressure is what bounds the width: the inverse cube of a pair keeps ten chain values next to the M state elements, the
// matrix product keeps the old and the new state.  So the pair loop and the loop over the matrix rows stay ROLLED -- the state
// (the new state) rotates through fixed registers, about 3 M^2 element moves per round next to its 72 M + M^2 paired products --
// and the chain's code exists once per kernel, not M / 2 times.
constexpr int RP_MAX_M = 8;

#if defined(__clang__)
#define SC_RP_ROLLED _Pragma("clang loop unroll(disable)")
#define SC_RP_UNROLLED _Pragma("unroll")
#else
#define SC_RP_ROLLED
#define SC_RP_UNROLLED
#endif

SC_HD Fe rp_reduce(Fe x) {                                     // x mod p for any 128-bit x (2^128 < 2p)
    if (fe_ge_p(x)) x = Fe{x.lo - P_LO, x.hi - P_HI - (x.lo < P_LO)};
    return x;
}

// the one-chain forms of rp_sqr2_n, rp_block2, rp_cube2 and rp_invcube2 (the element an odd width leaves over)
SC_HD void rp_sqr1_n(Fe& a, int n) {
    for (int i = 0; i < n; ++i) a = mont_mul(a, a);
}
SC_HD void rp_block1(Fe& a, Fe a0, int k) {
    rp_sqr1_n(a, 2 * k);
    a = mont_mul(a, a0);
}
SC_HD void rp_cube1(Fe& a) {
    a = mont_mul(mont_mul(a, a), a);
}
SC_HD void rp_invcube1(Fe& a) {
    const Fe a1 = a;
    Fe a2 = a;  rp_block1(a2, a1, 1);
    Fe a3 = a2; rp_block1(a3, a1, 1);
    Fe a5 = a3; rp_block1(a5, a2, 2);
    Fe ac = a5; rp_block1(ac, a2, 2);                          // B_7
    rp_block1(ac, ac, 7);
    rp_block1(ac, ac, 14);
    rp_block1(ac, ac, 28);
    rp_block1(ac, a3, 3);                                      // B_59
    const Fe ay = ac;
    const Fe az = mont_mul(ay, a1);
    rp_sqr1_n(ac, 1); ac = mont_mul(ac, az);
    rp_sqr1_n(ac, 3); ac = mont_mul(ac, ay);
    rp_sqr1_n(ac, 2); ac = mont_mul(ac, az);
    rp_sqr1_n(ac, 1); ac = mont_mul(ac, az);
    rp_sqr1_n(ac, 1); ac = mont_mul(ac, az);
    rp_sqr1_n(ac, 1); ac = mont_mul(ac, a1);
    rp_sqr1_n(ac, 1); a = mont_mul(ac, a1);
}

// s <- s rotated left by K places (constant indices only: the state stays in registers)
template <int M, int K>
SC_HD void rp_rotate(Fe (&s)[M]) {
    Fe t[K];
    SC_RP_UNROLLED
    for (int i = 0; i < K; ++i) t[i] = s[i];
    SC_RP_UNROLLED
    for (int i = 0; i + K < M; ++i) s[i] = s[i + K];
    SC_RP_UNROLLED
    for (int i = 0; i < K; ++i) s[M - K + i] = t[i];
}

// every element to its cube (INV: to its alphainv-th power).  Pairs go through s[0], s[1] and the state rotates by two; after M / 2
// pairs and the single element of an odd width the state has gone round once.
template <int M, bool INV>
SC_HD void rp_sbox_w(Fe (&s)[M]) {
    SC_RP_ROLLED
    for (int q = 0; q < M / 2; ++q) {
        if (INV) rp_invcube2(s[0], s[1]);
        else rp_cube2(s[0], s[1]);
        rp_rotate<M, 2>(s);
    }
    if (M & 1) {
        if (INV) rp_invcube1(s[0]);
        else rp_cube1(s[0]);
        rp_rotate<M, 1>(s);
    }
}

// s <- MDS s + c: row i of the matrix against the state, two products at a time (the last one of an odd width alone), the sums
// collected in t, which rotates by one per row
template <int M>
SC_HD void rp_mix_w(const Fe* mds, const Fe* c, Fe (&s)[M]) {
    Fe t[M];
    SC_RP_UNROLLED
    for (int i = 0; i < M; ++i) t[i] = fe_zero();
    SC_RP_ROLLED
    for (int i = 0; i < M; ++i) {
        const Fe* row = mds + i * M;
        Fe acc = c[i];
        SC_RP_UNROLLED
        for (int j = 0; j + 1 < M; j += 2) {
            Fe u, v;
            mont_mul2(row[j], s[j], row[j + 1], s[j + 1], u, v);
            acc = fe_add(acc, fe_add(u, v));
        }
        if (M & 1) acc = fe_add(acc, mont_mul(row[M - 1], s[M - 1]));
        rp_rotate<M, 1>(t);
        t[M - 1] = acc;
    }
    SC_RP_UNROLLED
    for (int i = 0; i < M; ++i) s[i] = t[i];
}

// One round on a Montgomery-form state: cube, mix, constants; inverse cube, mix, constants.
template <int M>
SC_HD void rp_round_w(const Fe* C, int r, Fe (&s)[M]) {
    const Fe* rc = C + M * M + 2 * M * r;
    rp_sbox_w<M, false>(s);
    rp_mix_w<M>(C, rc, s);
    rp_sbox_w<M, true>(s);
    rp_mix_w<M>(C, rc + M, s);
}

// What one lane does for input k of the three entries.  The state starts at zero; for each of `blocks` blocks, element j < rate of
// the block (any 128-bit value, reduced mod p) at in[(b * rate + j) * ld_in + k] is added into register j, then the state is
// permuted.  Afterwards registers 0 .. out_len - 1 go to out[j * ld_out + k] (canonical).  A plain permutation is one block of
// rate M with out_len M: the sum with the zero state is the load.  TRACE (one block): all rounds + 1 states instead, register s of
// state t at trace[s * (rounds + 1) + t].
template <int M, bool TRACE>
SC_HD void rp_sponge_w(const Fe* C, int rounds, const Fe* in, uint64_t ld_in, uint64_t blocks, int rate,
                       Fe* out, uint64_t ld_out, int out_len, Fe* trace) {
    Fe s[M];
    SC_RP_UNROLLED
    for (int j = 0; j < M; ++j) s[j] = fe_zero();
    for (uint64_t b = 0; b < blocks; ++b) {
        SC_RP_UNROLLED
        for (int j = 0; j < M; ++j)
            if (j < rate) {
                const Fe x = rp_reduce(in[(b * (uint64_t)rate + j) * ld_in]);
                if (TRACE) trace[(uint64_t)j * (rounds + 1)] = x;
                s[j] = fe_add(s[j], to_mont(x));
            } else if (TRACE) {
                trace[(uint64_t)j * (rounds + 1)] = fe_zero();
            }
        SC_RP_ROLLED
        for (int r = 0; r < rounds; ++r) {
            rp_round_w<M>(C, r, s);
            if (TRACE) {
                SC_RP_UNROLLED
                for (int j = 0; j < M; ++j) trace[(uint64_t)j * (rounds + 1) + r + 1] = from_mont(s[j]);
            }
        }
    }
    if (!TRACE) {
        SC_RP_UNROLLED
        for (int j = 0; j < M; ++j)
            if (j < out_len) out[(uint64_t)j * ld_out] = from_mont(s[j]);
    }
}

}  // namespace sc

// rescue_merkle.cuh -- the lane functions of the Rescue-Prime Merkle tree (csrc/rescue_merkle.hip, include/starkcore.h
// sc_rescue_merkle_*): a tree over the rows of a matrix whose leaves and nodes are digests of d field elements,
//     leaf(row) = sponge(row, out_len = d),   node(left, right) = sponge(left + right, out_len = d),
// the sponge being rescue_prime.cuh's permutation at a width M = 2 .. 8 with rate `rate`, padded with a single 1, then zeros up to a
// multiple of the rate (always at least the 1: len / rate + 1 blocks for a message of len elements).  There is no domain separation
// between leaves and nodes, like the tutorial's Merkle.
//
// Host-and-device code like rescue_prime.cuh: g++ compiles the same functions for the CPU emulation test
// (tests/emu/rescue_merkle_emu.cpp), hipcc for the kernels.  Two forms compute the same function, bit for bit (every value stored
// is a canonical residue, and a canonical residue does not depend on the order of the sums that produced it):
//
//   wide   one lane per node: rm_sponge_w keeps the M registers of a state in one lane, like rp_sponge_w, but takes its message
//          through a source functor and makes the padding up in registers -- nothing padded ever lives in memory.
//   split  one lane per state REGISTER: each lane takes its register through the one-element chains rp_cube1 / rp_invcube1, fetches
//          the other registers' powers across the lanes of its node for the mix and computes its own row of the matrix.  A lone
//          wave's time goes with the instructions of one lane: a narrow level takes a half (M = 3, 4) to a quarter (M = 8) of the
//          wide form's time -- 2 / M, not 1 / M, the wide lane's pairs being two independent chains side by side.
#pragma once
#include "rescue_prime.cuh"

namespace sc {

// ---- message sources: element i (any 128-bit word, i below the message's length) of the message of one node ---------------------
// a leaf: the `width` elements of row k of a coalesced matrix, p = d_rows + k
struct RmLeafSrc {
    const Fe* p;
    uint64_t ld;
    SC_HD Fe operator()(uint64_t i) const { return p[i * ld]; }
};
// a node: the digests of children 2 k and 2 k + 1 of the level below (element e of node c at below[e * w + c], w nodes), p = below + 2 k
struct RmNodeSrc {
    const Fe* p;
    uint64_t w;
    int d;
    SC_HD Fe operator()(uint64_t i) const {
        const uint64_t child = i >= (uint64_t)d;
        return p[(i - child * d) * w + child];
    }
};

// element i of the PADDED message in Montgomery form; x: the word loaded for it (read only where i < len)
SC_HD Fe rm_padded(Fe x, uint64_t i, uint64_t len) {
    if (i < len) return to_mont(rp_reduce(x));
    return i == len ? fe_mont_one() : fe_zero();
}

// ---- wide form ---------------------------------------------------------------------------------------------------------------------
// The sponge of one message of len elements over a zero state: s holds the final state in Montgomery form (the digest is
// from_mont of registers 0 .. d - 1).  The block loop and the round loop stay rolled, like rp_sponge_w's.
template <int M, class Src>
SC_HD void rm_sponge_w(const Fe* C, int rounds, const Src& src, uint64_t len, int rate, Fe (&s)[M]) {
    SC_RP_UNROLLED
    for (int j = 0; j < M; ++j) s[j] = fe_zero();
    const uint64_t blocks = len / (uint64_t)rate + 1;
    SC_RP_ROLLED
    for (uint64_t b = 0; b < blocks; ++b) {
        SC_RP_UNROLLED
        for (int j = 0; j < M; ++j)
            if (j < rate) {
                const uint64_t i = b * (uint64_t)rate + j;
                s[j] = fe_add(s[j], rm_padded(i < len ? src(i) : fe_zero(), i, len));
            }
        SC_RP_ROLLED
        for (int r = 0; r < rounds; ++r) rp_round_w<M>(C, r, s);
    }
}

// One lane's walk along an authentication path: the leaf's digest, then depth nodes, compared with the root (every word reduced
// mod p).  row: `width` contiguous elements; path: depth digests of d contiguous elements, the sibling leaf's first; bit j of
// index: whether the walk reaches level j from the right.  Between two levels the lane writes the next node's message -- its own
// digest and the sibling, in the order the bit says -- to its 2 d words of `pair` (element i at pair[i * ld_pair]) and reads it
// back as a plain strided message: the sponge then has the leaf kernel's source and no more registers to hold than that kernel.
template <int M>
SC_HD bool rm_verify_w(const Fe* C, int rounds, int rate, int d, const Fe* row, uint64_t width, uint64_t index, const Fe* path, int depth,
                       const Fe* root, Fe* pair, uint64_t ld_pair) {
    Fe s[M];
    SC_RP_ROLLED
    for (int lvl = -1; lvl < depth; ++lvl) {
        const bool leaf = lvl < 0;
        rm_sponge_w<M>(C, rounds, RmLeafSrc{leaf ? row : pair, leaf ? 1 : ld_pair}, leaf ? width : 2 * (uint64_t)d, rate, s);
        if (lvl + 1 < depth) {
            const uint64_t right = (index >> (lvl + 1)) & 1;
            const Fe* sibling = path + (uint64_t)(lvl + 1) * d;
            SC_RP_UNROLLED
            for (int j = 0; j < M; ++j)
                if (j < d) pair[(right * d + j) * ld_pair] = from_mont(s[j]);
            for (int e = 0; e < d; ++e) pair[((1 - right) * d + e) * ld_pair] = sibling[e];
        }
    }
    bool ok = true;
    SC_RP_UNROLLED
    for (int j = 0; j < M; ++j)
        if (j < d) ok = fe_eq(from_mont(s[j]), rp_reduce(root[j])) && ok;
    return ok;
}

// ---- split form: what ONE lane does with ITS register r; the caller supplies the exchange ---------------------------------------------
// the lane's share of a block: message element b * rate + r where r < rate (x: the word loaded for it), nothing otherwise
SC_HD Fe rm_split_absorb(Fe s, Fe x, uint64_t i, uint64_t len, bool in_rate) {
    return in_rate ? fe_add(s, rm_padded(x, i, len)) : s;
}
// the lane's power (INV: the alphainv-th, else the cube) ...
SC_HD Fe rm_split_power(Fe s, bool inv) {
    if (inv) rp_invcube1(s);
    else rp_cube1(s);
    return s;
}
// ... and, once it holds the powers pw[0 .. M - 1] of all registers of its node, its row of the matrix (row: M entries) plus its constant
template <int M>
SC_HD Fe rm_split_mix(const Fe (&row)[M], Fe c, const Fe (&pw)[M]) {
    Fe acc = c;
    SC_RP_UNROLLED
    for (int j = 0; j < M; ++j) acc = fe_add(acc, mont_mul(row[j], pw[j]));
    return acc;
}
// where in the constants `C` (M * M matrix entries, then 2 M per round) the lane of register r finds its constant of half round h (0: after the cube)
SC_HD uint64_t rm_split_constant(int M, int round, int h, int r) {
    return (uint64_t)M * M + 2ull * M * round + (uint64_t)h * M + r;
}

#if defined(__HIPCC__)
// The exchange on the device: every lane of the wave hands `mine` in and reads the M values of lanes base .. base + M - 1.
// Shuffles (ds_bpermute through __shfl), not LDS: 4 M dwords per half round next to the 2 or 142 Montgomery products of the power,
// no allocation, no barrier, and the nodes of a wave need not start at a power of two.  EVERY lane of the wave must get here
// (tail lanes and the lanes left over behind the last node of a wave included): callers mask loads and stores, never this call.
__device__ __forceinline__ Fe rm_shfl(Fe v, int lane) {
    const uint32_t a = __shfl((uint32_t)v.lo, lane, 64), b = __shfl((uint32_t)(v.lo >> 32), lane, 64);
    const uint32_t c = __shfl((uint32_t)v.hi, lane, 64), d = __shfl((uint32_t)(v.hi >> 32), lane, 64);
    return Fe{(uint64_t)a | ((uint64_t)b << 32), (uint64_t)c | ((uint64_t)d << 32)};
}
template <int M>
__device__ __forceinline__ void rm_exchange(Fe mine, int base, Fe (&pw)[M]) {
    SC_RP_UNROLLED
    for (int j = 0; j < M; ++j) pw[j] = rm_shfl(mine, base + j);
}

// One lane's walk through the sponge of one message.  r: its register, base: the first lane of its node in the wave, live: whether
// the lane belongs to a node at all (a lane that does not runs along on register 0's constants and loads nothing).  `word(i, want)`
// returns the raw word of message element i; it is called by EVERY lane exactly once per block (it may itself exchange), with
// want = false where the lane absorbs nothing or i lies in the padding.  Returns the lane's register of the final state, Montgomery form.
template <int M, class Word>
__device__ __forceinline__ Fe rm_sponge_split(const Fe* __restrict__ C, int rounds, const Word& word, uint64_t len, int rate, int r, int base, bool live) {
    Fe row[M];
    SC_RP_UNROLLED
    for (int j = 0; j < M; ++j) row[j] = C[r * M + j];
    const bool in_rate = live && r < rate;
    const uint64_t blocks = len / (uint64_t)rate + 1;
    Fe s = fe_zero();
    SC_RP_ROLLED
    for (uint64_t b = 0; b < blocks; ++b) {
        const uint64_t i = b * (uint64_t)rate + r;
        const Fe x = word(i, in_rate && i < len);
        s = rm_split_absorb(s, x, i, len, in_rate);
        SC_RP_ROLLED
        for (int rd = 0; rd < rounds; ++rd) {
            SC_RP_ROLLED
            for (int h = 0; h < 2; ++h) {
                Fe pw[M];
                rm_exchange<M>(rm_split_power(s, h != 0), base, pw);
                s = rm_split_mix<M>(row, C[rm_split_constant(M, rd, h, r)], pw);
            }
        }
    }
    return s;
}
#endif

}  // namespace sc

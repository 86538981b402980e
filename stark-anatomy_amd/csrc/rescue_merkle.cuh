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
//
// Below the sponges, in both forms again: the TRACE of a path -- every state of the walk from a leaf digest to the root, with the
// sibling and the direction bit beside it -- as the execution trace of a membership proof (rm_path_trace_w, rm_path_trace_split;
// DESIGN.md 3.9c).
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

// ---- the trace of a path (sc_rescue_merkle_path_trace_dev): every state of the walk from a leaf DIGEST to the root, for trees whose
// node is one permutation (2 d < rate: the padded message left + right + [1] + zeros is one block).  W = M + d + 1 registers -- the
// state, the sibling, the direction bit -- and T = depth * (rounds + 1) + 1 rows, register s of row t at out[s * T + t], canonical:
//   row 0                      the leaf digest in registers 0 .. d - 1, zeros elsewhere
//   row 1 + lvl (rounds + 1)   the first state of level lvl: the digest reached and path[lvl], in the order bit lvl of the index says,
//                              then 1, then zeros; the `rounds` rows behind it hold the state after each round
// and every row of a level carries path[lvl] and the bit in the sibling and bit registers.  The digest a level starts from is
// registers 0 .. d - 1 of the row before its first: row lvl (rounds + 1).
SC_HD uint64_t rm_trace_rows(int depth, int rounds) { return (uint64_t)depth * (rounds + 1) + 1; }
// which element of a digest register r of a level's first state holds (r < 2 d; 0 otherwise, so that everybody may load one)
SC_HD int rm_trace_element(int r, int d) { return r < d ? r : (r < 2 * d ? r - d : 0); }
// register r of a level's first state, canonical; own, sib: element rm_trace_element(r, d) of the digest reached and of the sibling
SC_HD Fe rm_trace_first(Fe own, Fe sib, int r, int d, unsigned bit) {
    if (r < 2 * d) {
        const bool walk = (unsigned)(r >= d) == bit;
        return Fe{walk ? own.lo : sib.lo, walk ? own.hi : sib.hi};
    }
    return r == 2 * d ? fe_one() : fe_zero();
}
// column `col` (one run of T elements) from row t0 on: `count` copies of v
SC_HD void rm_trace_fill(Fe* col, uint64_t t0, int count, Fe v) {
    for (int i = 0; i < count; ++i) col[t0 + i] = v;
}

// wide: one lane walks the whole path.  The hand-over between two levels needs no buffer: the digest reached is read back from the
// row the lane has just written (its own store, in program order), so the state array is only ever indexed by constants.
template <int M>
SC_HD void rm_path_trace_w(const Fe* C, int rounds, int d, const Fe* leaf, uint64_t index, const Fe* path, int depth, Fe* out, uint64_t T) {
    SC_RP_UNROLLED
    for (int j = 0; j < M; ++j) out[(uint64_t)j * T] = j < d ? rp_reduce(leaf[j]) : fe_zero();
    for (int e = 0; e <= d; ++e) out[(uint64_t)(M + e) * T] = fe_zero();
    // the sibling and bit columns first, the walk behind them: the walk then reads its siblings and bits from the trace itself, and
    // the round loop keeps one pointer next to the state instead of three and the index
    SC_RP_ROLLED
    for (int lvl = 0; lvl < depth; ++lvl) {
        const uint64_t t0 = (uint64_t)lvl * (rounds + 1);
        for (int e = 0; e < d; ++e) rm_trace_fill(out + (uint64_t)(M + e) * T, t0 + 1, rounds + 1, rp_reduce(path[(uint64_t)lvl * d + e]));
        rm_trace_fill(out + (uint64_t)(M + d) * T, t0 + 1, rounds + 1, Fe{(index >> lvl) & 1, 0});
    }
    Fe s[M];
    SC_RP_ROLLED
    for (int lvl = 0; lvl < depth; ++lvl) {
        const uint64_t t0 = (uint64_t)lvl * (rounds + 1);
        const unsigned bit = (unsigned)out[(uint64_t)(M + d) * T + t0 + 1].lo;
        SC_RP_UNROLLED
        for (int j = 0; j < M; ++j) {
            const int e = rm_trace_element(j, d);
            const Fe x = rm_trace_first(out[(uint64_t)e * T + t0], out[(uint64_t)(M + e) * T + t0 + 1], j, d, bit);
            out[(uint64_t)j * T + t0 + 1] = x;
            s[j] = to_mont(x);
        }
        SC_RP_ROLLED
        for (int r = 0; r < rounds; ++r) {
            rp_round_w<M>(C, r, s);
            // a ROLLED store loop, the state rotating through s[0] like rp_sbox_w's: one running address instead of M column
            // addresses kept across the round (16 VGPRs at M = 8, which the round does not have to spare)
            Fe* q = out + t0 + 2 + r;
            SC_RP_ROLLED
            for (int j = 0; j < M; ++j) {
                *q = from_mont(s[0]);
                q += T;
                rp_rotate<M, 1>(s);
            }
        }
    }
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

// One lane's share of the trace of a path (the layout above): the column of ITS state register r, and -- the item's own lanes, no
// others -- the sibling column M + r where r < d and the bit column where r == d (d < M always: 2 d < rate < M).  The digest reached
// stays with lanes 0 .. d - 1 of the item and reaches the lanes that start from it by a shuffle EVERY lane executes; a lane that is
// not live runs along on register 0's constants, loads and stores nothing.
template <int M>
__device__ __forceinline__ void rm_path_trace_split(const Fe* __restrict__ C, int rounds, int d, const Fe* leaf, uint64_t index, const Fe* path, int depth,
                                                    Fe* out, uint64_t T, int r, int base, bool live) {
    Fe row[M];
    SC_RP_UNROLLED
    for (int j = 0; j < M; ++j) row[j] = C[r * M + j];
    const int e = rm_trace_element(r, d);
    const bool state_of_path = live && r < 2 * d, sibling_column = live && r < d, bit_column = live && r == d;
    Fe* mine = out + (uint64_t)r * T;                 // the lane's state column
    Fe* side = out + (uint64_t)(M + r) * T;           // its sibling or bit column (written only where r <= d)
    Fe own = sibling_column ? rp_reduce(leaf[r]) : fe_zero();
    if (live) mine[0] = own;
    if (sibling_column || bit_column) side[0] = fe_zero();
    SC_RP_ROLLED
    for (int lvl = 0; lvl < depth; ++lvl) {
        const unsigned bit = (unsigned)((index >> lvl) & 1);
        const uint64_t t0 = (uint64_t)lvl * (rounds + 1);
        const Fe sib = state_of_path ? rp_reduce(path[(uint64_t)lvl * d + e]) : fe_zero();
        const Fe reached = rm_shfl(own, base + e);                                // every lane
        const Fe x = rm_trace_first(reached, sib, r, d, bit);
        if (live) mine[t0 + 1] = x;
        if (sibling_column) rm_trace_fill(side, t0 + 1, rounds + 1, sib);
        if (bit_column) rm_trace_fill(side, t0 + 1, rounds + 1, Fe{bit, 0});
        Fe s = to_mont(x);
        SC_RP_ROLLED
        for (int rd = 0; rd < rounds; ++rd) {
            SC_RP_ROLLED
            for (int h = 0; h < 2; ++h) {
                Fe pw[M];
                rm_exchange<M>(rm_split_power(s, h != 0), base, pw);
                s = rm_split_mix<M>(row, C[rm_split_constant(M, rd, h, r)], pw);
            }
            own = from_mont(s);
            if (live) mine[t0 + 2 + rd] = own;
        }
    }
}
#endif

}  // namespace sc

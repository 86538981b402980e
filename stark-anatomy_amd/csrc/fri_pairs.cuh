// fri_pairs.cuh -- pair leaves for FRI (not in the reference): a round's codeword cw of n elements is committed as the
// ROW tree (csrc/merkle_rows.cuh) of its two halves,
//
//   leaf i = BLAKE2b-512( cw[i] || cw[i + n/2], person = "sc-merkle-row" ),   i < n/2
//
// so the two points of a colinearity test open with ONE authentication path of log2(n/2) digests.
//
// From the second round on the codeword is the split-and-fold of the previous one (N elements in, N/2 out, q = N/4 leaves):
//   out[i] = (a + b)/2 + (a - b) * c * w^-i,   a = in[i], b = in[i + N/2], c = alpha / (2 * offset)
// and leaf j hashes out[j] || out[j + q].  PairFold is that leaf stage for merkle_subtree_kernel's Rows parameter: lane j folds both
// members of its pair, stores them to the folded codeword and hashes the 32-byte row out of registers -- a folded element never
// travels through memory between fold and hash.  Which four inputs, which two outputs and which twiddle exponents a lane takes is
// written once (pair_fold_lane), for the kernel and tests/emu/fri_pairs_emu.cpp.
#pragma once
#include "merkle_rows.cuh"

namespace sc {

struct PairFoldLane {
    uint64_t in[4];     // a0, b0, a1, b1: out[k] folds in[2k] and in[2k + 1]
    uint64_t out[2];    // the two members of leaf j, in the order they are hashed
    uint64_t exp[2];    // out[k] takes the twiddle w^-exp[k]
};
// lane j < q of a fold of 4q elements into 2q
SC_HD PairFoldLane pair_fold_lane(uint64_t j, uint64_t q) {
    PairFoldLane L;
    L.in[0] = j;       L.in[1] = j + 2 * q;
    L.in[2] = j + q;   L.in[3] = j + 3 * q;
    L.out[0] = j;      L.out[1] = j + q;
    L.exp[0] = j;      L.exp[1] = j + q;
    return L;
}
// the pair a lane hashes, as row_leaf_walk's source
struct PairSource {
    Fe v[2];
    SC_HD void gate(bool) const {}
    SC_HD Fe at(uint32_t c) const { return v[c]; }
};
// threads per opened pair of fri_pairs_query_kernel: one per value, one per 16-byte quarter of a path digest
SC_HD uint64_t pair_query_threads(uint32_t logL) { return 2ull + 4ull * logL; }

#if defined(__HIPCC__)

struct PairFold {
    static constexpr bool on = true;                // (merkle_subtree_kernel's Rows parameter)
    FoldIn f;
    uint64_t q;                                      // leaves of the tree = a quarter of the fold's input

    __device__ __forceinline__ Fe folded(Fe a, Fe b, uint64_t e) const {
        const Fe t = mont_mul(pow2level(f.lo, f.hi, e), f.c_m);                  // (c * w^-e) in Montgomery form, as fri_fold_kernel has it
        return fe_add(fe_half(fe_add(a, b)), mont_mul(fe_sub(a, b), t));
    }
    // the two folds run one after the other, and the compression only behind both stores: a Montgomery product and a BLAKE2b state
    // are alive in turn, not at once
    __device__ __forceinline__ void leaf(uint64_t j, uint64_t h[8]) const {
        const PairFoldLane L = pair_fold_lane(j, q);
        const Fe a0 = f.in[L.in[0]], b0 = f.in[L.in[1]], a1 = f.in[L.in[2]], b1 = f.in[L.in[3]];
        entry_prio(false);
        PairSource pair;
        pair.v[0] = folded(a0, b0, L.exp[0]);
        f.out[L.out[0]] = pair.v[0];
        pair.v[1] = folded(a1, b1, L.exp[1]);
        f.out[L.out[1]] = pair.v[1];
        row_leaf_walk(2u, pair, RowColumns::Compress{}, h);
    }
};

// Every opening of a proof's query phase in one launch: codeword j is a vector of 2 L_j elements under a pair tree of L_j leaves;
// opening i of it writes the pair {cw[a], cw[a + L_j]} and the log2(L_j) digests of leaf a's path.  thread_off / idx_off / path_off
// are exclusive prefix sums over the codewords (the scheme of merkle_query_multi_kernel).
constexpr int PAIRS_MAX_TREES = 32;
struct PairTree {
    const uint64_t* levels;
    const Fe* elems;
    uint64_t L;
    uint32_t logL;
    uint32_t per_query;      // 2 + 4 * logL threads per opened pair
    uint64_t thread_off;     // first thread of this codeword
    uint64_t idx_off;        // first index / first output pair of this codeword
    uint64_t path_off;       // first output digest of this codeword
};
struct PairTrees {
    PairTree t[PAIRS_MAX_TREES];
    uint64_t total_threads;
    int count;
};
#ifndef SC_ROWS_NO_KERNELS      // (merkle_rows.cuh: the plain kernels of the row stages have one home, merkle_rows.hip)
__global__ void __launch_bounds__(256) fri_pairs_query_kernel(const PairTrees Q, const uint64_t* __restrict__ indices, Fe* __restrict__ pairs_out,
                                                              uint64_t* __restrict__ paths_out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Q.total_threads) return;
    int w = 0;
    for (int i = 1; i < Q.count; ++i) if (t >= Q.t[i].thread_off) w = i;
    const PairTree& T = Q.t[w];
    const uint64_t local = t - T.thread_off;
    const uint64_t q = local / T.per_query;
    const uint32_t r = (uint32_t)(local % T.per_query);
    const uint64_t idx = indices[T.idx_off + q];
    if (r < 2u) {
        pairs_out[2 * (T.idx_off + q) + r] = T.elems[idx + (r ? T.L : 0ull)];
    } else {
        const uint32_t quarter = (r - 2u) & 3u, l = (r - 2u) >> 2;
        const uint64_t off = (l == 0) ? 0 : (2 * T.L - (T.L >> (l - 1)));
        const uint64_t node = (idx >> l) ^ 1ull;
        const ulonglong2* s = reinterpret_cast<const ulonglong2*>(T.levels + 8 * (off + node));
        ulonglong2* o = reinterpret_cast<ulonglong2*>(paths_out + 8 * (T.path_off + q * T.logL + l));
        o[quarter] = s[quarter];
    }
}
#endif  // SC_ROWS_NO_KERNELS

#ifndef SC_MERKLE_NO_KERNELS    // (merkle.cuh: QueryDone and the kernels around it belong to merkle_fri.hip)
// Its sibling for sc_fri_prove_pairs_dev: the pair openings AND the caller's further (ordinary tree, vector) pairs in one launch, the
// answers possibly straight into pinned host memory.  The first Q.pair_trees entries are pair trees as above; the entries behind them
// are ordinary trees of L = N leaves over N elements (per_query = 1 + 4 logL: the opened element, then the path), whose openings are
// numbered behind all pair openings: element idx_off + q - Q.pair_openings of elems_out.  `indices` may live in host memory: the first
// lane of every run of lanes that serve one opening loads it and hands it on (the scheme of merkle_query_multi_kernel, as is `done`).
struct ProveOpenings {
    PairTrees Q;
    int pair_trees;
    uint64_t pair_openings;
};
__global__ void __launch_bounds__(256) fri_pairs_prove_query_kernel(const ProveOpenings O, const uint64_t* __restrict__ indices, Fe* __restrict__ pairs_out,
                                                                    Fe* __restrict__ elems_out, uint64_t* __restrict__ paths_out, const QueryDone done) {
    const PairTrees& Q = O.Q;
    const uint64_t t_raw = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t_raw < Q.total_threads;
    const uint64_t t = live ? t_raw : Q.total_threads - 1;
    int w = 0;
    for (int i = 1; i < Q.count; ++i) if (t >= Q.t[i].thread_off) w = i;
    const PairTree& T = Q.t[w];
    const bool pair = w < O.pair_trees;
    const uint64_t local = t - T.thread_off;
    const uint64_t q = local / T.per_query;
    const uint32_t r = (uint32_t)(local % T.per_query);
    const uint64_t qn = T.idx_off + q;                        // the opening's number: non-decreasing along the lanes
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = __shfl_up(qn, 1);
    const bool leader = lane == 0 || below != qn;
    const uint64_t leaders = __ballot(leader);
    const uint64_t mine = leader ? indices[qn] : 0ull;
    const int src = 63 - __builtin_clzll(leaders & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull)));
    const uint64_t idx = __shfl(mine, src);
    const uint32_t values = pair ? 2u : 1u;                   // threads of an opening that copy a value; the others a quarter of a digest
    if (live) {
        if (r < values) {
            if (pair) pairs_out[2 * qn + r] = T.elems[idx + (r ? T.L : 0ull)];
            else elems_out[qn - O.pair_openings] = T.elems[idx];
        } else {
            const uint32_t quarter = (r - values) & 3u, l = (r - values) >> 2;
            const uint64_t off = (l == 0) ? 0 : (2 * T.L - (T.L >> (l - 1)));
            const uint64_t node = (idx >> l) ^ 1ull;
            const ulonglong2* s = reinterpret_cast<const ulonglong2*>(T.levels + 8 * (off + node));
            ulonglong2* o = reinterpret_cast<ulonglong2*>(paths_out + 8 * (T.path_off + q * T.logL + l));
            o[quarter] = s[quarter];
        }
    }
    if (done.host_flag) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned arrived = atomicAdd(done.ticket, 1u);
            if (arrived == gridDim.x - 1) {
                *done.ticket = 0;
                __threadfence_system();
                done.host_flag[0] = done.seq;
            }
        }
    }
}
#endif  // SC_MERKLE_NO_KERNELS

#endif  // __HIPCC__

}  // namespace sc

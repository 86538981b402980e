// merkle_forest.cuh -- a FOREST of BLAKE2b-512 Merkle trees: `count` trees of N leaves each over one device matrix [count][N] of
// residues, built by ONE set of launches (Merkle.commit_batch, Fri.prove_batch).  Hashing is merkle.cuh's (leaf = H(decimal ASCII),
// node = H(left || right), merkle.py:11-14); what is new here is only WHO hashes WHAT:
//
//   layout   tree-major: tree t is a block of 2N digests at digest t * 2N, with the single tree's level offsets inside it (level 0 at
//            0, level l >= 1 at 2N - (N >> (l - 1)), the root at 2N - 2; the last digest of a block is unused), so every opening is the
//            single tree's gather plus a base.
//   numbering  node n of tree t at level l (N >> l nodes per tree) has the FLAT number t * (N >> l) + n: a level of the forest is one
//            row of count * (N >> l) digests.  A parent's flat number is half its children's (N is a power of two, so siblings never
//            straddle two trees): climbing the forest is climbing ONE tree of count * N leaves and stopping log2 N levels up.
//   launches a workgroup owns 256 consecutive flat nodes of the launch's start level and climbs up to 8 levels of their subtree(s)
//            through LDS (the scheme of merkle_subtree_kernel).  With N >= 256 those are 256 nodes of one tree; with a level narrower
//            than 256 they are 256 / width whole trees, so the narrow levels -- one lone workgroup per tree in the single-tree build --
//            are count times as wide here, and trees of fewer than 256 leaves share a workgroup from the leaves on.  A forest of
//            2^12-leaf trees is two launches (levels 0-8, then 8-12), of 2^8-leaf trees one.  Plain launches, stream-ordered.
//   fold     the leaf stage may compute its leaves as the split-and-fold of fri.py:85 of the previous round's matrix [count][2N], as
//            merkle_subtree_kernel's FoldIn does, with ONE challenge per tree: c_m = alpha_t / (2 offset) is read from a device array
//            [count]; the power table of omega^-1 is the forest's.  The element is fold_element's, bit for bit.
//   rows     the leaf stage may instead hash ROWS (csrc/merkle_rows.cuh: a row forest, tree t = the row commitment of its own w columns,
//            which lie in a few matrices described by segments): the Rows template parameter, as merkle_subtree_kernel has one.  Only
//            level 0 differs -- h comes from row_leaf_walk over the one-lane compression, no LDS is used before the climb -- and the
//            tree is the LANE's (trees of fewer than 256 rows share a workgroup); everything above is the same code.
//
// The indexing is written as SC_HD functions so that tests/emu/merkle_forest_emu.cpp runs the same numbering on the host.
#pragma once
#include "field.cuh"
#if defined(__HIPCC__)
#include "merkle.cuh"
#endif

namespace sc {

constexpr uint32_t FOREST_WG = 256;          // flat nodes per workgroup at a launch's start level
constexpr int FOREST_LAUNCH_LEVELS = 8;      // levels climbed per launch at most (256 -> 1)

struct ForestShape {
    uint64_t N;          // leaves per tree (power of two)
    uint64_t count;      // trees
    int logN;
};

SC_HD uint64_t forest_level_off(uint64_t N, int l) { return l == 0 ? 0 : 2 * N - (N >> (l - 1)); }
SC_HD uint64_t forest_tree_base(uint64_t N, uint64_t tree) { return tree * 2 * N; }
// where flat node `flat` of level `level` lives (digest index from the forest's base); false: beyond the last tree (the padding of
// the last workgroup)
SC_HD bool forest_place(const ForestShape& s, int level, uint64_t flat, uint64_t* digest, uint64_t* tree_out = nullptr) {
    const int lw = s.logN - level;                     // log2 of the level's width inside one tree
    const uint64_t tree = flat >> lw, node = flat & ((1ull << lw) - 1ull);
    *digest = forest_tree_base(s.N, tree) + forest_level_off(s.N, level) + node;
    if (tree_out) *tree_out = tree;
    return tree < s.count;
}
// the launches of a build: launch k starts at level lvl0 = 8 k and climbs forest_launch_levels(logN, lvl0) levels
SC_HD int forest_launch_levels(int logN, int lvl0) { return logN - lvl0 < FOREST_LAUNCH_LEVELS ? logN - lvl0 : FOREST_LAUNCH_LEVELS; }
SC_HD uint64_t forest_launch_workgroups(const ForestShape& s, int lvl0) { return (s.count * (s.N >> lvl0) + FOREST_WG - 1) / FOREST_WG; }
// after climbing l levels a workgroup holds 256 >> l nodes; its node p there has this flat number
SC_HD uint64_t forest_wg_flat(uint64_t wg, int l, uint32_t p) { return wg * (FOREST_WG >> l) + p; }

// ---- openings: for any number of (forest, matrix) pairs, the elements and authentication paths at positions (tree, index)
constexpr int FOREST_QUERY_MAX_PAIRS = 32;
struct ForestQueryPair {
    const uint64_t* levels;
    const Fe* elems;         // the forest's matrix [count][N]
    uint64_t N;
    uint32_t logN;
    uint32_t per_query;      // 4 * logN + 1 threads per opening: a 16-byte quarter of every path digest, and the element
    uint64_t thread_off;     // exclusive prefix sums over the pairs: first thread, first opening, first output digest
    uint64_t idx_off;
    uint64_t path_off;
};
struct ForestQuery {
    ForestQueryPair p[FOREST_QUERY_MAX_PAIRS];
    uint64_t total_threads;
    int count;
};
// which opening and which part of it thread t copies
SC_HD void forest_query_route(const ForestQuery& Q, uint64_t t, int* pair, uint64_t* q, uint32_t* r) {
    int w = 0;
    for (int i = 1; i < Q.count; ++i) if (t >= Q.p[i].thread_off) w = i;
    const uint64_t local = t - Q.p[w].thread_off;
    *pair = w;
    *q = local / Q.p[w].per_query;
    *r = (uint32_t)(local % Q.p[w].per_query);
}
// digest l of the path of (tree, index): level l's sibling of the node above the leaf (merkle.py:16-27)
SC_HD uint64_t forest_path_digest(uint64_t N, uint64_t tree, uint64_t index, uint32_t l) {
    return forest_tree_base(N, tree) + forest_level_off(N, (int)l) + ((index >> l) ^ 1ull);
}

#if defined(__HIPCC__)

struct ForestFold {
    const Fe* in;        // previous round's matrix [count][2N]
    Fe* out;             // folded matrix [count][N]
    const Fe* lo;        // two-level power table of omega^-1
    const Fe* hi;
    const Fe* c_m;       // [count]: alpha_t / (2 * offset), Montgomery form
};

// one level by the four-lane path (merkle.cuh: blake2b_node_4lane), `parents` <= 64 nodes of the workgroup, stored by flat number
__device__ __forceinline__ void forest_level_4lane(const uint64_t* src, uint64_t* dst, uint64_t* __restrict__ levels, const ForestShape& s, int level,
                                                   uint64_t flat0, uint32_t parents, uint32_t t, uint64_t* roots_out) {
    const uint32_t j = t & 3u, n = t >> 2;
    if (n >= parents) return;                          // (whole quads)
    uint64_t lo, hi;
    blake2b_node_4lane(src + 17u * n, j, lo, hi);
    dst[lin_off(n) + j] = lo;
    dst[lin_off(n) + 4u + j] = hi;
    uint64_t dig, tree;
    if (forest_place(s, level, flat0 + n, &dig, &tree)) {
        levels[8 * dig + j] = lo;
        levels[8 * dig + 4u + j] = hi;
        if (roots_out && level == s.logN) { roots_out[8 * tree + j] = lo; roots_out[8 * tree + 4u + j] = hi; }
    }
}

// LEAVES: the launch starts at level 0 and hashes the residues (FOLD: computes them first); else it reads its 256 nodes from the forest.
// FOUR_LANE: a launch of few workgroups (latency-bound): from 128 nodes per workgroup down, four lanes per compression.
// roots_out (optional, may be pinned host memory): the launch that reaches the roots also writes them there, 64 bytes per tree.
// Rows (with LEAVES): another leaf stage altogether -- rows.leaf(tree, i, h) hashes row i of tree `tree` into h (csrc/merkle_rows.cuh:
// RowForestColumns, a ROW forest); the default, NoRows, is the decimal leaf of one residue and leaves every instantiation as it was.
template <bool LEAVES, bool FOUR_LANE, bool FOLD, class Rows = NoRows>
__global__ void __launch_bounds__(256) forest_climb_kernel(const Fe* __restrict__ elems, uint64_t* __restrict__ levels, const ForestShape s, int lvl0, int nlev,
                                                           const ForestFold fold, uint64_t* roots_out, const Rows rows = Rows()) {
    __shared__ uint4 cur[(LEAVES && !Rows::on) ? 256 * 5 : 256 * 4];   // this level's digests (16 KiB); before that, the decimal leaf stage's 80 bytes per thread
    constexpr bool four_lane = FOUR_LANE && (SC_MERKLE_4LANE != 0);
    constexpr uint32_t FOUR_LANE_FROM = SC_FOUR_LANE_FROM;
    __shared__ uint64_t linA[four_lane ? (SC_FOUR_LANE_FROM / 2) * 17 : 1], linB[four_lane ? (SC_FOUR_LANE_FROM / 4) * 17 : 1];
    const uint32_t t = threadIdx.x;
    const uint64_t wg = blockIdx.x;
    uint64_t h[8];
    {
        uint64_t dig, tree;
        const uint64_t flat = forest_wg_flat(wg, 0, t);
        const bool there = forest_place(s, lvl0, flat, &dig, &tree);
        entry_prio(true);
        if constexpr (LEAVES && Rows::on) {
            // the tree is the lane's own (trees of fewer than 256 rows share a workgroup); a lane past the last tree loads nothing
#pragma unroll
            for (int k = 0; k < 8; ++k) h[k] = 0;
            if (there) rows.leaf(tree, flat & (s.N - 1), h);      // (lowers the entry priority behind each block's loads)
            entry_prio(false);
        } else if (LEAVES) {
            uint64_t m[16];
            Fe e = Fe{0, 0};
            if (there) {
                if constexpr (FOLD) {
                    FoldIn f;
                    f.in = fold.in + tree * 2 * s.N; f.out = nullptr; f.lo = fold.lo; f.hi = fold.hi; f.c_m = fold.c_m[tree];
                    e = fold_element(f, flat & (s.N - 1), s.N);
                    fold.out[flat] = e;
                } else {
                    e = elems[flat];
                }
            }
            entry_prio(false);
            uint32_t len = leaf_message_lds(e, m, reinterpret_cast<uint8_t*>(cur) + LEAF_SLOT_BYTES * t);
            blake2b_single_block(m, len, h);
            __syncthreads();                               // every thread is done with its slot of `cur` before digests are published there
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) h[k] = 0;
            if (there) {
                const ulonglong2* src = reinterpret_cast<const ulonglong2*>(levels + 8 * dig);
#pragma unroll
                for (int k = 0; k < 4; ++k) { ulonglong2 v = src[k]; h[2 * k] = v.x; h[2 * k + 1] = v.y; }
            }
            entry_prio(false);
        }
    }
    uint32_t width = 256;
    int l = 0;
    for (;; ++l) {
        if (t < width) {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                uint4 v;
                v.x = (uint32_t)h[2 * k]; v.y = (uint32_t)(h[2 * k] >> 32); v.z = (uint32_t)h[2 * k + 1]; v.w = (uint32_t)(h[2 * k + 1] >> 32);
                cur[dig_slot(t, k)] = v;
            }
            if constexpr (four_lane) {
                if (width == FOUR_LANE_FROM) {
#pragma unroll
                    for (uint32_t w = 0; w < 8; ++w) linA[lin_off(t) + w] = h[w];
                }
            }
        }
        __syncthreads();
        if (LEAVES || l > 0) {
            // (16-byte quarters of consecutive flat nodes: coalesced inside a tree, and a tree's level is contiguous)
            for (uint32_t q = t; q < width * 4u; q += 256u) {
                uint64_t dig, tree;
                if (forest_place(s, lvl0 + l, forest_wg_flat(wg, l, q >> 2), &dig, &tree)) {
                    const uint4 v = cur[dig_slot(q >> 2, q & 3u)];
                    reinterpret_cast<uint4*>(levels + 8 * dig)[q & 3u] = v;
                    if (roots_out && lvl0 + l == s.logN) reinterpret_cast<uint4*>(roots_out + 8 * tree)[q & 3u] = v;
                }
            }
        }
        if (l == nlev) return;
        if constexpr (four_lane) {
            if (width == FOUR_LANE_FROM) break;
        }
        width >>= 1;
        if (t < width) {
            uint64_t m[16];
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                uint4 v = cur[dig_slot(2 * t + (k >> 2), k & 3u)];
                m[2 * k] = ((uint64_t)v.y << 32) | v.x;
                m[2 * k + 1] = ((uint64_t)v.w << 32) | v.z;
            }
            blake2b_single_block(m, 128u, h);
        }
        __syncthreads();                               // everyone has read `cur` before it is overwritten
    }
    if constexpr (four_lane) {
        uint64_t* src = linA;
        uint64_t* dst = linB;
        for (++l; l <= nlev; ++l) {
            width >>= 1;
            forest_level_4lane(src, dst, levels, s, lvl0 + l, forest_wg_flat(wg, l, 0), width, t, roots_out);
            __syncthreads();
            uint64_t* sw = src; src = dst; dst = sw;
        }
    }
}

#ifndef SC_MERKLE_NO_KERNELS      // (merkle.cuh: a translation unit that wants the kernel templates only -- merkle_rows.hip's row forests)
// the forest form of merkle_query_multi_kernel: opening q of the launch is (trees[q], indices[q]) in the pair its number falls into
__global__ void __launch_bounds__(256) forest_query_kernel(const ForestQuery Q, const uint64_t* __restrict__ trees, const uint64_t* __restrict__ indices,
                                                           Fe* __restrict__ elems_out, uint64_t* __restrict__ paths_out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Q.total_threads) return;
    int w;
    uint64_t q;
    uint32_t r;
    forest_query_route(Q, t, &w, &q, &r);
    const ForestQueryPair& T = Q.p[w];
    const uint64_t tree = trees[T.idx_off + q], idx = indices[T.idx_off + q];
    if (r == T.per_query - 1) {
        elems_out[T.idx_off + q] = T.elems[tree * T.N + idx];
    } else {
        const uint32_t quarter = r & 3u, l = r >> 2;
        const ulonglong2* src = reinterpret_cast<const ulonglong2*>(T.levels + 8 * forest_path_digest(T.N, tree, idx, l));
        ulonglong2* o = reinterpret_cast<ulonglong2*>(paths_out + 8 * (T.path_off + q * T.logN + l));
        o[quarter] = src[quarter];
    }
}
#endif  // SC_MERKLE_NO_KERNELS

#endif  // __HIPCC__

}  // namespace sc

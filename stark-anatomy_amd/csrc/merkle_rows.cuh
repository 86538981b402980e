// merkle_rows.cuh -- row commitments: ONE Merkle tree over the rows of a matrix of codewords (not in the reference).
//
//   leaf i = BLAKE2b-512( col[0][i] || col[1][i] || ... || col[w-1][i], person = "sc-merkle-row" )   16 little-endian bytes per value
//   node   = BLAKE2b-512( left || right )                                                             as in merkle.cuh
//
// The personalisation (bytes 48 .. 63 of BLAKE2b's parameter block, XORed into h[6] and h[7]) keeps leaves and nodes apart: a row of
// eight values is 128 bytes, the length of a node's message.  A message of 16 w bytes takes ceil(16 w / 128) compressions; the state
// is kept across the blocks and the message words are refilled eight values per block.
//
// The block walk -- which column lands in which message word of which block, the byte counter, the final flag, the personalised
// initial state -- is written ONCE, for the host and the device, over the compression function: the kernels run it with the unrolled
// one-lane rounds of merkle.cuh, sc_merkle_row_leaf and tests/emu/merkle_rows_emu.cpp with transcript.h's blake2b_compress.
#pragma once
#include "merkle.cuh"
#include "merkle_forest.cuh"

namespace sc {

constexpr uint32_t ROWS_MAX_COLUMNS = 256;          // SC_MERKLE_ROWS_MAX_COLUMNS of include/starkcore.h
// "sc-merkle-row", zero-padded to 16 bytes, as two little-endian words
constexpr uint64_t ROW_PERSON_LO = 0x6C6B72656D2D6373ull, ROW_PERSON_HI = 0x000000776F722D65ull;

SC_HD void row_leaf_initial_state(uint64_t h[8]) {
    h[0] = 0x6A09E667F3BCC908ull ^ 0x01010040ull;   // digest 64, key 0, fanout 1, depth 1
    h[1] = 0xBB67AE8584CAA73Bull; h[2] = 0x3C6EF372FE94F82Bull; h[3] = 0xA54FF53A5F1D36F1ull;
    h[4] = 0x510E527FADE682D1ull; h[5] = 0x9B05688C2B3E6C1Full;
    h[6] = 0x1F83D9ABFB41BD6Bull ^ ROW_PERSON_LO;
    h[7] = 0x5BE0CD19137E2179ull ^ ROW_PERSON_HI;
}

// The leaf digest of one row of w >= 1 values into h.
//   source.at(c)                 the row's value in column c (called once per column, in column order)
//   source.gate(on)              brackets the loads of one block (the kernels raise their wave's priority there)
//   compress(h, m, t, last)      one BLAKE2b compression of the block m[16]; t = bytes of the message so far, this block included
// A last block that is exactly full is the final one (no empty block follows it); a partial last block is zero-padded.
template <class Source, class Compress>
SC_HD void row_leaf_walk(uint32_t w, Source source, Compress compress, uint64_t h[8]) {
    row_leaf_initial_state(h);
    const uint32_t blocks = (w + 7u) >> 3;
    for (uint32_t b = 0; b < blocks; ++b) {
        uint64_t m[16];
        source.gate(true);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t c = 8u * b + j;
            Fe e = Fe{0, 0};
            if (c < w) e = source.at(c);
            m[2 * j] = e.lo;
            m[2 * j + 1] = e.hi;
        }
        source.gate(false);
        const bool last = b + 1 == blocks;
        compress(h, m, last ? 16ull * w : 128ull * (b + 1), last);
    }
}

// ---- row FORESTS: `count` row trees of N rows and w columns each, built by forest_climb_kernel (csrc/merkle_forest.cuh) with the row
// leaf stage above.  In a batch the columns are not count * w allocations: they are the columns of a few matrices (the prover's: the
// boundary-quotient LDE matrix [K R][N] and the randomizer LDE matrix [K][N]), so they are described by up to ROW_FOREST_MAX_SEGMENTS
// SEGMENTS instead of a pointer each.  Segment s is a matrix of count * per_tree[s] columns, `pitch` >= N elements apart; tree t's
// columns are, segment after segment, columns t * per_tree .. t * per_tree + per_tree - 1 of that segment:
//     column c of tree t at row i  =  base_s[(t * per_tree_s + (c - first_s)) * pitch_s + i],     first_s = per_tree_0 + .. + per_tree_{s-1}
// w = sum of per_tree, 1 <= w <= 256.  The lookup is written once, for the kernels and tests/emu/row_forest_emu.cpp.
constexpr uint32_t ROW_FOREST_MAX_SEGMENTS = 8;     // SC_ROW_FOREST_MAX_SEGMENTS of include/starkcore.h
struct RowSegment {                                  // sc_row_segment_t
    const Fe* base;
    uint64_t per_tree;
    uint64_t pitch;
};
struct RowSegments {
    RowSegment seg[ROW_FOREST_MAX_SEGMENTS];
    uint32_t n, w;
};
// the segment that holds column c, reached from the segment of an earlier column (a row is walked in column order)
struct RowSegmentCursor { uint32_t s = 0, first = 0; };
SC_HD void row_segment_seek(const RowSegments& S, uint32_t c, RowSegmentCursor& k) {
    while (c >= k.first + (uint32_t)S.seg[k.s].per_tree) {          // (c < w: ends inside the table)
        k.first += (uint32_t)S.seg[k.s].per_tree;
        ++k.s;
    }
}
SC_HD uint64_t row_segment_element(const RowSegment& g, uint64_t tree, uint32_t column, uint64_t i) { return (tree * g.per_tree + column) * g.pitch + i; }
SC_HD const Fe* row_segment_address(const RowSegments& S, uint64_t tree, uint32_t c, uint64_t i, RowSegmentCursor& k) {
    row_segment_seek(S, c, k);
    const RowSegment& g = S.seg[k.s];
    return g.base + row_segment_element(g, tree, c - k.first, i);
}
// threads per opened position of row_forest_query_kernel: one per value, one per 16-byte quarter of a path digest
SC_HD uint64_t row_forest_query_threads(uint32_t w, uint32_t logN) { return (uint64_t)w + 4ull * logN; }

#if defined(__HIPCC__)

// The columns of a row tree as a kernel argument: the w columns are separate device vectors (the boundary quotients are the rows of
// one LDE matrix, the randomizer is an allocation of its own), so the kernels take a table of pointers, not a matrix with a leading
// dimension.  The table lives in the kernel-argument segment: the pointers are wave-uniform scalar loads, nothing is uploaded and
// nothing has to outlive the launch.  Lane t of a workgroup reads col[c][base + t]: 16 contiguous bytes per lane, coalesced per column.
struct RowColumns {
    static constexpr bool on = true;                // (merkle_subtree_kernel's Rows parameter)
    const Fe* col[ROWS_MAX_COLUMNS];
    uint32_t w;

    struct Source {
        const RowColumns& C;
        uint64_t row;
        __device__ __forceinline__ void gate(bool on) const { entry_prio(on); }
        __device__ __forceinline__ Fe at(uint32_t c) const { return C.col[c][row]; }
    };
    struct Compress {
        __device__ __forceinline__ void operator()(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last) const { blake2b_compress_block(m, t, last, h); }
    };
    __device__ __forceinline__ void leaf(uint64_t row, uint64_t h[8]) const { row_leaf_walk(w, Source{*this, row}, Compress{}, h); }
};

// SC_ROWS_NO_KERNELS: a translation unit that wants the leaf stages of this header only (merkle_fri.hip: the pair form of the persistent
// tail kernel hashes pair leaves) defines it; the plain kernels have one home, merkle_rows.hip.
#ifndef SC_ROWS_NO_KERNELS
// level 0 of a tree of fewer than 256 leaves (from 256 up the row stage is the entry of merkle_subtree_kernel<true, *, false, RowColumns>)
__global__ void __launch_bounds__(256) merkle_rows_leaf_kernel(const RowColumns C, uint64_t* __restrict__ digests, uint64_t N) {
    __shared__ uint4 sm[256 * 4];
    const uint64_t base = (uint64_t)blockIdx.x * 256u;
    const uint32_t n_here = (uint32_t)((N - base) < 256u ? (N - base) : 256u);
    const bool active = threadIdx.x < n_here;
    uint64_t h[8];
    if (active) C.leaf(base + threadIdx.x, h);
    store_digests_coalesced(sm, h, active, digests, base, n_here);
}

// k opened rows in one launch: per position its w values (rows_out [k][w], 16 bytes each) and its authentication path (paths_out,
// 64 * logN bytes per position, digest l = level_l[(index >> l) ^ 1]).  One thread per value and per 16-byte quarter of a digest.
__global__ void __launch_bounds__(256) merkle_rows_query_kernel(const RowColumns C, const uint64_t* __restrict__ levels, uint64_t N, int logN,
                                                                const uint64_t* __restrict__ indices, uint64_t k, Fe* __restrict__ rows_out, uint64_t* __restrict__ paths_out) {
    const uint64_t per = (uint64_t)C.w + 4ull * (uint64_t)logN;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * per) return;
    const uint64_t q = t / per;
    const uint32_t r = (uint32_t)(t % per);
    const uint64_t idx = indices[q];
    if (r < C.w) {
        rows_out[q * C.w + r] = C.col[r][idx];
    } else {
        const uint32_t quarter = (r - C.w) & 3u, l = (r - C.w) >> 2;
        const uint64_t off = (l == 0) ? 0 : (2 * N - (N >> (l - 1)));
        const uint64_t node = (idx >> l) ^ 1ull;
        const ulonglong2* s = reinterpret_cast<const ulonglong2*>(levels + 8 * (off + node));
        ulonglong2* o = reinterpret_cast<ulonglong2*>(paths_out + 8 * (q * (uint64_t)logN + l));
        o[quarter] = s[quarter];
    }
}

#endif  // SC_ROWS_NO_KERNELS

// The segments of a row forest as a kernel argument (forest_climb_kernel's Rows parameter): the table is wave-uniform and read by
// scalar loads from the kernel-argument segment, the SEGMENT of a column is wave-uniform (columns are walked in step), the TREE is the
// lane's own -- trees of fewer than 256 rows share a workgroup -- so the address is computed per lane.  Lane (tree, row) reads 16
// contiguous bytes per column; the lanes of one tree are coalesced.
struct RowForestColumns {
    static constexpr bool on = true;
    RowSegments S;

    struct Source {
        const RowSegments& S;
        uint64_t tree, row;
        RowSegmentCursor k;
        __device__ __forceinline__ void gate(bool on) const { entry_prio(on); }
        __device__ __forceinline__ Fe at(uint32_t c) { return *row_segment_address(S, tree, c, row, k); }
    };
    __device__ __forceinline__ void leaf(uint64_t tree, uint64_t row, uint64_t h[8]) const {
        row_leaf_walk(S.w, Source{S, tree, row, RowSegmentCursor{}}, RowColumns::Compress{}, h);
    }
};

#ifndef SC_ROWS_NO_KERNELS
// k opened rows of a row forest in one launch: per position (trees[q], indices[q]) its w values (rows_out [k][w], 16 bytes each) and its
// authentication path (paths_out, 64 * logN bytes per position, digest l at forest_path_digest).  One thread per value and per 16-byte
// quarter of a digest.
__global__ void __launch_bounds__(256) row_forest_query_kernel(const RowSegments S, const uint64_t* __restrict__ levels, uint64_t N, int logN,
                                                               const uint64_t* __restrict__ trees, const uint64_t* __restrict__ indices, uint64_t k,
                                                               Fe* __restrict__ rows_out, uint64_t* __restrict__ paths_out) {
    const uint64_t per = row_forest_query_threads(S.w, (uint32_t)logN);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * per) return;
    const uint64_t q = t / per;
    const uint32_t r = (uint32_t)(t % per);
    const uint64_t tree = trees[q], idx = indices[q];
    if (r < S.w) {
        RowSegmentCursor cur;
        rows_out[q * S.w + r] = *row_segment_address(S, tree, r, idx, cur);
    } else {
        const uint32_t quarter = (r - S.w) & 3u, l = (r - S.w) >> 2;
        const ulonglong2* s = reinterpret_cast<const ulonglong2*>(levels + 8 * forest_path_digest(N, tree, idx, l));
        ulonglong2* o = reinterpret_cast<ulonglong2*>(paths_out + 8 * (q * (uint64_t)logN + l));
        o[quarter] = s[quarter];
    }
}

#endif  // SC_ROWS_NO_KERNELS

#endif  // __HIPCC__

}  // namespace sc

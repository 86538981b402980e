// merkle_rows.hip -- row commitments (csrc/merkle_rows.cuh): one Merkle tree over the rows of a matrix of codewords
// whose columns are separate device vectors.  The tree is an ordinary sc_merkle_t: the climb above the leaf stage, the root's way to
// the host and everything that reads a tree are merkle_fri.hip's.  Row FORESTS (count such trees in one set of launches, the columns
// described by segments): the leaf stage of merkle_fri.hip's forest_build and a query kernel of their own; the result is an ordinary
// sc_merkle_forest_t.  Pair leaves for FRI (csrc/fri_pairs.cuh) live here too: a round's codeword under the row tree of
// its two halves, built by the row stage above or, behind a fold, by a leaf stage that computes the fold itself.
#define SC_MERKLE_NO_KERNELS
#include "core.h"
#include "merkle_rows.cuh"
#include "fri_pairs.cuh"
#include "transcript.h"

namespace {

int rows_check(const char* what, const void* const* d_cols, uint64_t w, uint64_t N) {
    if (!d_cols) return fail(SC_ERR_BAD_ARG, std::string(what) + ": null argument");
    if (w == 0 || w > SC_MERKLE_ROWS_MAX_COLUMNS) return fail(SC_ERR_BAD_ARG, std::string(what) + ": 1 .. 256 columns");
    for (uint64_t c = 0; c < w; ++c) if (!d_cols[c]) return fail(SC_ERR_BAD_ARG, std::string(what) + ": null column");
    if (!is_pow2(N)) return fail(SC_ERR_NOT_POW2, "length must be power of two");
    return SC_OK;
}

void rows_table(const void* const* d_cols, uint64_t w, RowColumns& C) {
    for (uint64_t c = 0; c < ROWS_MAX_COLUMNS; ++c) C.col[c] = c < w ? (const Fe*)d_cols[c] : nullptr;
    C.w = (uint32_t)w;
}

int rows_build(const void* const* d_cols, uint64_t w, uint64_t N, uint8_t root_out[64], sc_merkle_t** tree, hipStream_t st, BuildMode mode) {
    RowColumns C;
    rows_table(d_cols, w, C);
    // the leaf stage of merkle_build_device: below 256 leaves a plain launch (nlev < 0), from there up the entry of the fused subtree
    // launch -- leaves plus nlev levels through LDS, the level_off layout of the decimal trees
    const LeafStage leaves = [&C](uint64_t* levels, uint64_t n, int nlev, bool four_lane, hipStream_t s) {
        if (nlev < 0) hipLaunchKernelGGL(merkle_rows_leaf_kernel, dim3(1), dim3(256), 0, s, C, levels, n);
        else if (four_lane) hipLaunchKernelGGL((merkle_subtree_kernel<true, true, false, RowColumns>), dim3((unsigned)(n / 256)), dim3(256), 0, s, (const Fe*)nullptr, levels, n, 0, nlev, FoldIn(), C);
        else hipLaunchKernelGGL((merkle_subtree_kernel<true, false, false, RowColumns>), dim3((unsigned)(n / 256)), dim3(256), 0, s, (const Fe*)nullptr, levels, n, 0, nlev, FoldIn(), C);
    };
    return merkle_build_device(nullptr, N, root_out, tree, st, mode, nullptr, &leaves);
}

// ---- row forests: the checks of both entries, and the segment table as the kernels take it
int row_forest_table(const char* what, const sc_row_segment_t* segs, uint64_t n_segs, uint64_t N, RowSegments& S) {
    if (!segs) return fail(SC_ERR_BAD_ARG, std::string(what) + ": null argument");
    if (n_segs == 0 || n_segs > SC_ROW_FOREST_MAX_SEGMENTS) return fail(SC_ERR_BAD_ARG, std::string(what) + ": 1 .. 8 segments");
    uint64_t w = 0;
    for (uint64_t s = 0; s < ROW_FOREST_MAX_SEGMENTS; ++s) {
        if (s >= n_segs) { S.seg[s] = RowSegment{nullptr, 0, 0}; continue; }
        if (!segs[s].base) return fail(SC_ERR_BAD_ARG, std::string(what) + ": null segment");
        if (segs[s].per_tree == 0 || segs[s].per_tree > SC_MERKLE_ROWS_MAX_COLUMNS || (w += segs[s].per_tree) > SC_MERKLE_ROWS_MAX_COLUMNS)
            return fail(SC_ERR_BAD_ARG, std::string(what) + ": 1 .. 256 columns per tree");
        if (segs[s].pitch < N) return fail(SC_ERR_BAD_ARG, std::string(what) + ": a segment's pitch is at least N");
        S.seg[s] = RowSegment{(const Fe*)segs[s].base, segs[s].per_tree, segs[s].pitch};
    }
    S.n = (uint32_t)n_segs;
    S.w = (uint32_t)w;
    return SC_OK;
}

}  // namespace

extern "C" {

int sc_merkle_row_forest_build_dev(const sc_row_segment_t* segs, uint64_t n_segs, uint64_t N, uint64_t count, sc_merkle_forest_t** forest, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!forest) return fail(SC_ERR_BAD_ARG, "sc_merkle_row_forest_build_dev: null argument");
    if (N >= 2 && !is_pow2(N)) return fail(SC_ERR_NOT_POW2, "length must be power of two");
    RowForestColumns C;
    SCCHK(row_forest_table("sc_merkle_row_forest_build_dev", segs, n_segs, N, C.S));
    SCCHK(forest_args(N, count, 2));
    // the leaf stage of forest_build: the launch that starts at level 0 hashes rows; the launches above it are the decimal forests'
    const ForestLeafStage leaves = [&C](uint64_t* levels, uint64_t n, uint64_t trees, int nlev, bool four_lane, unsigned wgs, uint64_t* roots, hipStream_t s) {
        const ForestShape shape{n, trees, ilog2(n)};
        if (four_lane) hipLaunchKernelGGL((forest_climb_kernel<true, true, false, RowForestColumns>), dim3(wgs), dim3(256), 0, s, (const Fe*)nullptr, levels, shape, 0, nlev, ForestFold{}, roots, C);
        else hipLaunchKernelGGL((forest_climb_kernel<true, false, false, RowForestColumns>), dim3(wgs), dim3(256), 0, s, (const Fe*)nullptr, levels, shape, 0, nlev, ForestFold{}, roots, C);
    };
    return forest_build(nullptr, N, count, nullptr, nullptr, forest, pick_stream(stream), &leaves);
}

int sc_merkle_row_forest_query_dev(const sc_merkle_forest_t* forest, const sc_row_segment_t* segs, uint64_t n_segs, const uint64_t* trees, const uint64_t* indices, uint64_t k,
                                   void* rows_out, uint8_t* paths_out) {
    std::unique_lock<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!forest) return fail(SC_ERR_BAD_ARG, "sc_merkle_row_forest_query_dev: null argument");
    RowSegments S;
    SCCHK(row_forest_table("sc_merkle_row_forest_query_dev", segs, n_segs, forest->N, S));
    if (k && (!trees || !indices || !rows_out || !paths_out)) return fail(SC_ERR_BAD_ARG, "sc_merkle_row_forest_query_dev: null argument");
    for (uint64_t i = 0; i < k; ++i)
        if (trees[i] >= forest->count || indices[i] >= forest->N) return fail(SC_ERR_BAD_ARG, "cannot open invalid index");
    if (k == 0) return SC_OK;
    hipStream_t st = g.stream;
    if (!forest->have_roots && forest->st != st) HIPCHK(hipStreamWaitEvent(st, forest->done, 0));     // built on another stream: ordered in front of the gather
    const uint64_t w = S.w;
    const size_t idx_bytes = (k * 8 + 255) & ~255ull;
    const size_t row_bytes = k * w * sizeof(Fe), path_bytes = k * 64 * (size_t)forest->logN;
    // a buffer of sc_host_alloc is written by the kernel itself (the stores cross the bus as they are made); any other host pointer
    // is served through device scratch and a copy
    const bool rows_direct = host_pool_holds(rows_out, row_bytes), paths_direct = host_pool_holds(paths_out, path_bytes);
    const size_t row_stage = rows_direct ? 0 : (row_bytes + 255) & ~255ull, path_stage = paths_direct ? 0 : path_bytes;
    void* buf;
    SCCHK(scratch(5, 2 * idx_bytes + row_stage + path_stage + 256, &buf));
    uint64_t* d_trees = (uint64_t*)buf;
    uint64_t* d_idx = (uint64_t*)((char*)buf + idx_bytes);
    Fe* d_rows = rows_direct ? (Fe*)rows_out : (Fe*)((char*)buf + 2 * idx_bytes);
    uint64_t* d_paths = paths_direct ? (uint64_t*)paths_out : (uint64_t*)((char*)buf + 2 * idx_bytes + row_stage);
    SCCHK(upload(d_trees, trees, k * 8, st));
    SCCHK(upload(d_idx, indices, k * 8, st));
    const uint64_t total = k * row_forest_query_threads((uint32_t)w, (uint32_t)forest->logN);
    hipLaunchKernelGGL(row_forest_query_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, S, (const uint64_t*)forest->d_levels, forest->N, forest->logN,
                       (const uint64_t*)d_trees, (const uint64_t*)d_idx, k, d_rows, d_paths);
    HIPCHK(hipGetLastError());
    if (!rows_direct) HIPCHK(hipMemcpyAsync(rows_out, d_rows, row_bytes, hipMemcpyDeviceToHost, st));
    if (!paths_direct) HIPCHK(hipMemcpyAsync(paths_out, d_paths, path_bytes, hipMemcpyDeviceToHost, st));
    if (rows_direct && paths_direct) {                     // nothing but the kernel's own stores to wait for: poll, as sc_merkle_forest_query_dev does
        hipEvent_t ev = event_get();
        if (ev) {
            hipError_t e = hipEventRecord(ev, st);
            int rc = e == hipSuccess ? wait_polled(nullptr, ev) : fail(SC_ERR_HIP, hipGetErrorString(e));
            g_event_pool.push_back(ev);
            return rc;
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    return SC_OK;
}

int sc_merkle_rows_build_dev(const void* const* d_cols, uint64_t w, uint64_t N, uint8_t root_out[64], sc_merkle_t** tree, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!root_out && !tree) return fail(SC_ERR_BAD_ARG, "sc_merkle_rows_build_dev: null argument");
    SCCHK(rows_check("sc_merkle_rows_build_dev", d_cols, w, N));
    return rows_build(d_cols, w, N, root_out, tree, pick_stream(stream), BUILD_SYNC);
}

int sc_merkle_rows_build_async_dev(const void* const* d_cols, uint64_t w, uint64_t N, sc_merkle_t** tree, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree) return fail(SC_ERR_BAD_ARG, "sc_merkle_rows_build_async_dev: null argument");
    SCCHK(rows_check("sc_merkle_rows_build_async_dev", d_cols, w, N));
    return rows_build(d_cols, w, N, nullptr, tree, pick_stream(stream), BUILD_ASYNC);
}

int sc_merkle_rows_query_dev(const sc_merkle_t* tree, const void* const* d_cols, uint64_t w, const uint64_t* indices, uint64_t k, void* rows_out, uint8_t* paths_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree) return fail(SC_ERR_BAD_ARG, "sc_merkle_rows_query_dev: null argument");
    SCCHK(rows_check("sc_merkle_rows_query_dev", d_cols, w, tree->N));
    if (k && (!indices || !rows_out || (tree->logN > 0 && !paths_out))) return fail(SC_ERR_BAD_ARG, "sc_merkle_rows_query_dev: null argument");
    for (uint64_t i = 0; i < k; ++i) if (indices[i] >= tree->N) return fail(SC_ERR_BAD_ARG, "cannot open invalid index");
    if (k == 0) return SC_OK;
    const size_t idx_bytes = (k * 8 + 255) & ~255ull;
    const size_t row_bytes = k * w * sizeof(Fe), path_bytes = k * 64 * (size_t)tree->logN;
    // a buffer of sc_host_alloc is written by the kernel itself (the stores cross the bus as they are made); any other host pointer
    // is served through device scratch and a copy
    const bool rows_direct = host_pool_holds(rows_out, row_bytes), paths_direct = !path_bytes || host_pool_holds(paths_out, path_bytes);
    const size_t row_stage = rows_direct ? 0 : (row_bytes + 255) & ~255ull, path_stage = paths_direct ? 0 : path_bytes;
    void* buf;
    SCCHK(scratch(5, idx_bytes + row_stage + path_stage + 256, &buf));
    uint64_t* d_idx = (uint64_t*)buf;
    Fe* d_rows = rows_direct ? (Fe*)rows_out : (Fe*)((char*)buf + idx_bytes);
    uint64_t* d_paths = paths_direct ? (uint64_t*)paths_out : (uint64_t*)((char*)buf + idx_bytes + row_stage);
    SCCHK(upload(d_idx, indices, k * 8, g.stream));
    RowColumns C;
    rows_table(d_cols, w, C);
    const uint64_t total = k * (w + 4ull * (uint64_t)tree->logN);
    hipLaunchKernelGGL(merkle_rows_query_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, g.stream, C, (const uint64_t*)tree->d_levels, tree->N, tree->logN,
                       (const uint64_t*)d_idx, k, d_rows, d_paths);
    HIPCHK(hipGetLastError());
    if (!rows_direct) HIPCHK(hipMemcpyAsync(rows_out, d_rows, row_bytes, hipMemcpyDeviceToHost, g.stream));
    if (!paths_direct) HIPCHK(hipMemcpyAsync(paths_out, d_paths, path_bytes, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return SC_OK;
}

// ---- pair leaves for FRI (csrc/fri_pairs.cuh): a round's codeword under the row tree of its two halves
// one round of the commit phase with pair leaves: the fold of d_in (N elements) into d_out (N/2) and the pair tree over d_out (N/4
// leaves), enqueued.  From 256 leaves up the leaf stage of the tree computes the fold (PairFold); below, the fold kernel and the plain
// row leaf launch over {d_out, d_out + N/4}.
int sc_fri_fold_pairs_commit_dev(const void* d_in, uint64_t N, const uint64_t alpha[2], const uint64_t offset[2], const uint64_t omega[2], void* d_out,
                                 sc_merkle_t** tree, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !d_in || !d_out || !alpha || !offset || !omega) return fail(SC_ERR_BAD_ARG, "sc_fri_fold_pairs_commit_dev: null argument");
    if (N < 4 || !is_pow2(N)) return fail(SC_ERR_NOT_POW2, "sc_fri_fold_pairs_commit_dev: codeword length must be a power of two >= 4");
    return fold_pairs_and_build((const Fe*)d_in, N, fe_from(alpha), fe_from(offset), fe_from(omega), (Fe*)d_out, tree, pick_stream(stream));
}
}  // extern "C"

namespace sci {
int pair_tree_start(const Fe* d_codeword, uint64_t n, sc_merkle** tree, hipStream_t st) {
    const void* halves[2] = {d_codeword, d_codeword + n / 2};
    return rows_build(halves, 2, n / 2, nullptr, tree, st, BUILD_ASYNC);
}
int fold_pairs_and_build(const Fe* d_in, uint64_t N, Fe alpha, Fe offset, Fe omega, Fe* d_out, sc_merkle** tree, hipStream_t st) {
    const uint64_t q = N / 4;
    if (q < 256) {
        SCCHK(fold_device(d_in, N, alpha, offset, omega, d_out, st));
        return pair_tree_start(d_out, N / 2, tree, st);
    }
    PairFold P;
    SCCHK(fold_prepare(d_in, N, alpha, offset, omega, d_out, st, &P.f));
    P.q = q;
    // the launch plan of the row stage (rows_build): nlev levels of every 256-leaf subtree behind the leaves, four lanes per hash on
    // the narrow levels of a latency-bound launch
    const LeafStage leaves = [&P](uint64_t* levels, uint64_t n, int nlev, bool four_lane, hipStream_t s) {
        if (four_lane) hipLaunchKernelGGL((merkle_subtree_kernel<true, true, false, PairFold>), dim3((unsigned)(n / 256)), dim3(256), 0, s, (const Fe*)nullptr, levels, n, 0, nlev, FoldIn(), P);
        else hipLaunchKernelGGL((merkle_subtree_kernel<true, false, false, PairFold>), dim3((unsigned)(n / 256)), dim3(256), 0, s, (const Fe*)nullptr, levels, n, 0, nlev, FoldIn(), P);
    };
    return merkle_build_device(nullptr, q, nullptr, tree, st, BUILD_ASYNC, nullptr, &leaves);
}
}  // namespace sci

extern "C" {

// every opening of a proof's query phase in one launch: codeword j = 2 L_j elements at d_codewords[j] under the pair tree trees[j] of
// L_j leaves; counts[j] of the concatenated `indices` belong to it; per opening the pair (32 bytes) and the path (64 * log2 L_j bytes),
// packed codeword after codeword
int sc_fri_pairs_query_dev(uint64_t n, const sc_merkle_t* const* trees, const void* const* d_codewords, const uint64_t* indices, const uint64_t* counts,
                           void* pairs_out, uint8_t* paths_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (n == 0) return SC_OK;
    if (!trees || !d_codewords || !counts) return fail(SC_ERR_BAD_ARG, "sc_fri_pairs_query_dev: null argument");
    uint64_t total = 0;
    size_t path_bytes = 0;
    for (uint64_t t = 0; t < n; ++t) {
        if (!trees[t] || !d_codewords[t]) return fail(SC_ERR_BAD_ARG, "sc_fri_pairs_query_dev: null tree or codeword");
        if (counts[t] && !indices) return fail(SC_ERR_BAD_ARG, "sc_fri_pairs_query_dev: null argument");
        for (uint64_t i = 0; i < counts[t]; ++i) if (indices[total + i] >= trees[t]->N) return fail(SC_ERR_BAD_ARG, "cannot open invalid index");
        total += counts[t];
        path_bytes += counts[t] * 64 * (size_t)trees[t]->logN;
    }
    if (total == 0) return SC_OK;
    if (!pairs_out || (path_bytes && !paths_out)) return fail(SC_ERR_BAD_ARG, "sc_fri_pairs_query_dev: null argument");
    // a tree that was only enqueued (on whatever stream) is complete once its root has landed
    for (uint64_t t = 0; t < n; ++t)
        if (counts[t] && !trees[t]->have_root) SCCHK(merkle_root_wait(const_cast<sc_merkle_t*>(trees[t])));
    const size_t idx_bytes = (total * 8 + 255) & ~255ull;
    const size_t pair_bytes = total * 2 * sizeof(Fe);
    // a buffer of sc_host_alloc is written by the kernel itself; any other host pointer is served through device scratch and a copy
    const bool pairs_direct = host_pool_holds(pairs_out, pair_bytes), paths_direct = !path_bytes || host_pool_holds(paths_out, path_bytes);
    const size_t pair_stage = pairs_direct ? 0 : (pair_bytes + 255) & ~255ull, path_stage = paths_direct ? 0 : path_bytes;
    void* buf;
    SCCHK(scratch(5, idx_bytes + pair_stage + path_stage + 256, &buf));
    uint64_t* d_idx = (uint64_t*)buf;
    Fe* d_pairs = pairs_direct ? (Fe*)pairs_out : (Fe*)((char*)buf + idx_bytes);
    uint64_t* d_paths = paths_direct ? (uint64_t*)paths_out : (uint64_t*)((char*)buf + idx_bytes + pair_stage);
    SCCHK(upload(d_idx, indices, total * 8, g.stream));
    // one launch per PAIRS_MAX_TREES codewords (a proof: one launch)
    uint64_t off = 0, poff = 0;
    for (uint64_t t0 = 0; t0 < n; t0 += PAIRS_MAX_TREES) {
        PairTrees Q;
        Q.count = 0;
        Q.total_threads = 0;
        for (uint64_t t = t0; t < n && t < t0 + PAIRS_MAX_TREES; ++t) {
            const uint64_t k = counts[t];
            if (!k) continue;
            PairTree& T = Q.t[Q.count++];
            T.levels = trees[t]->d_levels;
            T.elems = (const Fe*)d_codewords[t];
            T.L = trees[t]->N;
            T.logL = (uint32_t)trees[t]->logN;
            T.per_query = (uint32_t)pair_query_threads(T.logL);
            T.thread_off = Q.total_threads;
            T.idx_off = off;
            T.path_off = poff;
            Q.total_threads += k * T.per_query;
            off += k;
            poff += k * (uint64_t)trees[t]->logN;
        }
        if (!Q.count) continue;
        hipLaunchKernelGGL(fri_pairs_query_kernel, dim3((unsigned)((Q.total_threads + 255) / 256)), dim3(256), 0, g.stream, Q, (const uint64_t*)d_idx, d_pairs, d_paths);
    }
    HIPCHK(hipGetLastError());
    if (!pairs_direct) HIPCHK(hipMemcpyAsync(pairs_out, d_pairs, pair_bytes, hipMemcpyDeviceToHost, g.stream));
    if (!paths_direct) HIPCHK(hipMemcpyAsync(paths_out, d_paths, path_bytes, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return SC_OK;
}

// host only: the walk of merkle_rows.cuh over transcript.h's compression
int sc_merkle_row_leaf(const void* row, uint64_t w, uint8_t out[64]) {
    if (!row || !out || w == 0 || w > SC_MERKLE_ROWS_MAX_COLUMNS) {
        std::lock_guard<std::mutex> lk(g_mu);
        return fail(SC_ERR_BAD_ARG, "sc_merkle_row_leaf: a row of 1 .. 256 values");
    }
    struct Source {
        const uint8_t* row;
        void gate(bool) const {}
        Fe at(uint32_t c) const { Fe e; memcpy(&e, row + 16 * (size_t)c, 16); return e; }
    };
    uint64_t h[8];
    row_leaf_walk((uint32_t)w, Source{(const uint8_t*)row},
                  [](uint64_t* hh, const uint64_t* m, uint64_t t, bool last) { blake2b_compress(hh, (const uint8_t*)m, t, last); }, h);
    memcpy(out, h, 64);
    return SC_OK;
}

}  // extern "C"

// rescue_merkle.hip -- Merkle trees whose hash is the Rescue-Prime sponge (csrc/rescue_merkle.cuh): build over the rows of a
// coalesced matrix, all levels kept in HBM; root, openings, level copies; batched verification of authentication paths, and the
// traces of such walks for membership proofs.
#include "core.h"
#include "rescue_merkle.cuh"

struct sc_rescue_tree {
    Fe* d_levels = nullptr;     // level j (N >> j nodes of d elements, element e of node k at e * (N >> j) + k) at element rm_level_offset(N, d, j)
    size_t bytes = 0;
    uint64_t N = 0;
    int logN = 0, d = 0;
    hipEvent_t done = nullptr;  // recorded behind the build: root, openings and level copies wait for it on their own streams
};

namespace sci {

static __host__ __device__ inline uint64_t rm_level_offset(uint64_t N, int d, int level) { return (uint64_t)d * (2 * N - 2 * (N >> level)); }

// ---- wide form: one lane per node, 256 lanes, four waves per SIMD like rescue_wide_kernel (128 VGPRs at the widest state) ----------
// LEAF: node k is the digest of row k (`width` elements at in[j * ld + k]); otherwise of children 2 k, 2 k + 1 of the level `in` (2 n nodes).
template <int M, bool LEAF>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
rescue_tree_wide_kernel(const Fe* __restrict__ C, int rounds, const Fe* in, uint64_t ld, uint64_t width, int rate, int d, Fe* out, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    Fe s[M];
    if (LEAF) rm_sponge_w<M>(C, rounds, RmLeafSrc{in + k, ld}, width, rate, s);
    else rm_sponge_w<M>(C, rounds, RmNodeSrc{in + 2 * k, 2 * n, d}, 2 * (uint64_t)d, rate, s);
    SC_RP_UNROLLED
    for (int j = 0; j < M; ++j)
        if (j < d) out[(uint64_t)j * n + k] = from_mont(s[j]);
}

// ---- split form: one lane per state register.  Grouping: 64 / M nodes per wave, node g of the wave in lanes g M .. g M + M - 1; the
// 64 % M lanes behind the last node (widths 3, 5, 6, 7) and the lanes of nodes past n run along on lane 0's values, load and store
// nothing.  The exchange is a shuffle with an arbitrary source lane, so a node need not start at a power of two and no width
// gives up more than 4 lanes of 64 (M = 5, 6: 60 of 64 busy).
template <int M>
struct SplitLane {
    uint64_t node;
    int r, base;
    bool live;
    __device__ __forceinline__ explicit SplitLane(uint64_t n) {
        constexpr int PER = 64 / M;
        const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        const int lane = threadIdx.x & 63, g = lane / M;
        node = wave * PER + g;
        live = g < PER && node < n;
        r = live ? lane - g * M : 0;
        base = live ? g * M : 0;
        if (!live) node = 0;
    }
};
template <class Src>
struct SplitWord {           // a source in memory: only the lanes that want a word load
    Src src;
    __device__ __forceinline__ Fe operator()(uint64_t i, bool want) const { return want ? src(i) : fe_zero(); }
};

template <int M, bool LEAF>
__global__ void __launch_bounds__(256)
rescue_tree_split_kernel(const Fe* __restrict__ C, int rounds, const Fe* in, uint64_t ld, uint64_t width, int rate, int d, Fe* out, uint64_t n) {
    const SplitLane<M> L(n);
    Fe s;
    if (LEAF) {
        SplitWord<RmLeafSrc> word{RmLeafSrc{in + L.node, ld}};
        s = rm_sponge_split<M>(C, rounds, word, width, rate, L.r, L.base, L.live);
    } else {
        SplitWord<RmNodeSrc> word{RmNodeSrc{in + 2 * L.node, 2 * n, d}};
        s = rm_sponge_split<M>(C, rounds, word, 2 * (uint64_t)d, rate, L.r, L.base, L.live);
    }
    if (L.live && L.r < d) out[(uint64_t)L.r * n + L.node] = from_mont(s);
}

// ---- openings: one launch gathers all k paths.  Thread (t, j, e): element e of node (index_t >> j) ^ 1 of level j.
__global__ void __launch_bounds__(256) rescue_tree_open_kernel(const Fe* __restrict__ levels, uint64_t N, int logN, int d, const uint64_t* __restrict__ idx, uint64_t total, Fe* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const uint64_t e = g % d, tj = g / d, j = tj % logN, t = tj / logN;
    const uint64_t w = N >> j;
    out[g] = levels[rm_level_offset(N, d, (int)j) + e * w + ((idx[t] >> j) ^ 1)];
}

// ---- verification: an item's whole walk (depth + 1 sponges in sequence) inside one launch.  Item-major host layouts, see the header.
struct VerifyArgs {
    const Fe* roots;
    const uint64_t* idx;
    const Fe* paths;
    const Fe* rows;
    Fe* pair;               // wide form: the message of the node a walk reaches next, element i (of 2 d) of item t at pair[i * k + t]
    uint8_t* verdicts;
    uint64_t k, width;
    int depth, d, rate, rounds;
};

// wide: one lane per item (rm_verify_w)
template <int M>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
rescue_tree_verify_wide_kernel(const Fe* __restrict__ C, const VerifyArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.k) return;
    a.verdicts[t] = rm_verify_w<M>(C, a.rounds, a.rate, a.d, a.rows + t * a.width, a.width, a.idx[t], a.paths + t * a.depth * a.d, a.depth,
                                   a.roots + t * a.d, a.pair + t, a.k);
}

// split: one lane per register of an item's state; the digest stays in lanes 0 .. d - 1 of the item and reaches the lanes that
// absorb it by a shuffle that every lane executes
struct SplitPathWord {
    const Fe* rows;
    const Fe* sibs;         // paths + level * d
    uint64_t t, width, item_stride;
    int d, base;
    unsigned bit;
    bool leaf;
    Fe own;                 // this lane's element of the digest reached so far (lanes 0 .. d - 1 of the item), canonical
    __device__ __forceinline__ Fe operator()(uint64_t i, bool want) const {
        const uint32_t du = (uint32_t)d, iu = (uint32_t)(i < 2ull * du ? i : 0);
        const uint32_t child = iu >= du, e = iu - child * du;                    // e below d for every lane, wanted or not
        const Fe mine = rm_shfl(own, base + (int)e);                             // every lane, before any masking
        if (!want) return fe_zero();
        // a word is loaded either way (the sibling's is there and harmless where the walk's own digest is wanted) and the choice is
        // made between VALUES: a choice between the load and `mine` makes the compiler park `mine` in scratch to select an address
        const Fe x = leaf ? rows[t * width + i] : sibs[t * item_stride + e];
        const bool walk = !leaf && child == bit;
        return Fe{walk ? mine.lo : x.lo, walk ? mine.hi : x.hi};
    }
};
template <int M>
__global__ void __launch_bounds__(256)
rescue_tree_verify_split_kernel(const Fe* __restrict__ C, const VerifyArgs a) {
    const SplitLane<M> L(a.k);
    const uint64_t index = L.live ? a.idx[L.node] : 0;
    Fe own = fe_zero();
    SC_RP_ROLLED
    for (int lvl = -1; lvl < a.depth; ++lvl) {
        const bool leaf = lvl < 0;
        const SplitPathWord word{a.rows, a.paths + (leaf ? 0 : lvl) * (uint64_t)a.d, L.node, a.width, (uint64_t)a.depth * a.d, a.d, L.base,
                                 leaf ? 0u : (unsigned)((index >> lvl) & 1), leaf, own};
        own = from_mont(rm_sponge_split<M>(C, a.rounds, word, leaf ? a.width : 2 * (uint64_t)a.d, a.rate, L.r, L.base, L.live));
    }
    const bool differs = L.live && L.r < a.d && !fe_eq(own, rp_reduce(a.roots[L.node * a.d + L.r]));
    const unsigned long long bad = __ballot(differs);                              // every lane
    if (L.live && L.r == 0) a.verdicts[L.node] = ((bad >> L.base) & ((1ull << M) - 1)) == 0;
}

// ---- the trace of a path: every state of an item's walk (depth permutations in sequence) inside one launch.  Item t's W = M + d + 1
// columns of T rows lie one behind the other at out + W T t (rescue_merkle.cuh: the layout).
struct TraceArgs {
    const Fe* leaves;       // item-major: leaves[t * d + e]
    const uint64_t* idx;
    const Fe* paths;        // paths[((t * depth) + j) * d + e]
    Fe* out;
    uint64_t k, T;
    int depth, d, rounds;
};
// wide: one lane per item (rm_path_trace_w)
template <int M>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
rescue_path_trace_wide_kernel(const Fe* __restrict__ C, const TraceArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.k) return;
    rm_path_trace_w<M>(C, a.rounds, a.d, a.leaves + t * a.d, a.idx[t], a.paths + t * a.depth * a.d, a.depth, a.out + (uint64_t)(M + a.d + 1) * a.T * t, a.T);
}
// split: one lane per register of an item's state (rm_path_trace_split), 64 / M items per wave
template <int M>
__global__ void __launch_bounds__(256)
rescue_path_trace_split_kernel(const Fe* __restrict__ C, const TraceArgs a) {
    const SplitLane<M> L(a.k);
    const uint64_t index = L.live ? a.idx[L.node] : 0;
    rm_path_trace_split<M>(C, a.rounds, a.d, a.leaves + L.node * a.d, index, a.paths + L.node * a.depth * a.d, a.depth,
                           a.out + (uint64_t)(M + a.d + 1) * a.T * L.node, a.T, L.r, L.base, L.live);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
struct Shape {
    uint64_t m, rate, d, rounds;
};
static int check_shape(const std::string& what, const Shape& s, const void* params) {
    if (s.m < 2 || s.m > (uint64_t)RP_MAX_M) return fail(SC_ERR_BAD_ARG, what + "a state width of 2 .. 8 expected");
    if (s.rate < 2 || s.rate >= s.m) return fail(SC_ERR_BAD_ARG, what + "a rate of 2 .. m - 1 expected");
    if (s.d == 0 || s.d > s.rate) return fail(SC_ERR_BAD_ARG, what + "a digest length of 1 .. rate expected");
    if (s.rounds == 0 || s.rounds > (uint64_t)RP_MAX_ROUNDS) return fail(SC_ERR_BAD_ARG, what + "1 .. 27 rounds expected");
    if (!params) return fail(SC_ERR_BAD_ARG, what + "null parameters");
    return SC_OK;
}
constexpr size_t MAX_CONSTANTS = RP_MAX_M * RP_MAX_M + 2 * RP_MAX_M * RP_MAX_ROUNDS;
// the constants in Montgomery form (host[MAX_CONSTANTS]); returns their number, 0 when one is not below p
static uint64_t constants_to_mont(const Shape& s, const void* params, Fe* host) {
    const uint64_t count = s.m * s.m + 2 * s.m * s.rounds;
    const Fe* h = (const Fe*)params;
    for (uint64_t i = 0; i < count; ++i) {
        const Fe v{h[i].lo, h[i].hi};
        if (fe_ge_p(v)) return 0;
        host[i] = to_mont(v);
    }
    return count;
}
// Which form a level of `nodes` nodes (a batch of `nodes` paths) takes: sc_set_tuning("rescue_tree_split_max_nodes").  The default
// is measured (tools/rescue_merkle_timing.py, profiles/rescue_merkle): the largest power-of-two level width of the sweep 2^0 .. 2^18
// at which the split form's median is below the wide form's by more than the spread of the repetitions at EVERY state width
// measured (m = 3, 4, 8); a difference inside the spread is a tie and goes to the wide form.  Up to 2^14 nodes a level is one
// lane's instruction stream and the split form takes a half (m = 3, 4) to a quarter (m = 8) of the wide form's time; from 2^16
// on the two close in on each other, and at 2^17 and 2^18 m = 3 and m = 4 are ties (m = 8 still gains 0.5 to 1.3 ms there).
constexpr int SPLIT_MAX_NODES_DEFAULT = 1 << 16;
static bool split_wanted(uint64_t nodes) {
    int key = g.rescue_tree_split_max_nodes;
    if (key < 0) key = SPLIT_MAX_NODES_DEFAULT;
    return key == INT32_MAX || (key > 0 && nodes <= (uint64_t)key);
}
static unsigned wide_grid(uint64_t n) { return (unsigned)((n + 255) / 256); }
static unsigned split_grid(uint64_t n, uint64_t m) {
    const uint64_t per = 64 / m, waves = (n + per - 1) / per;
    return (unsigned)((waves + 3) / 4);
}

template <int M>
static void level_enqueue(bool split, bool leaf, const Fe* C, const Shape& s, const Fe* in, uint64_t ld, uint64_t width, Fe* out, uint64_t n, hipStream_t st) {
    const int rounds = (int)s.rounds, rate = (int)s.rate, d = (int)s.d;
    if (split) {
        const dim3 grid(split_grid(n, M));
        if (leaf) hipLaunchKernelGGL((rescue_tree_split_kernel<M, true>), grid, dim3(256), 0, st, C, rounds, in, ld, width, rate, d, out, n);
        else hipLaunchKernelGGL((rescue_tree_split_kernel<M, false>), grid, dim3(256), 0, st, C, rounds, in, ld, width, rate, d, out, n);
    } else {
        const dim3 grid(wide_grid(n));
        if (leaf) hipLaunchKernelGGL((rescue_tree_wide_kernel<M, true>), grid, dim3(256), 0, st, C, rounds, in, ld, width, rate, d, out, n);
        else hipLaunchKernelGGL((rescue_tree_wide_kernel<M, false>), grid, dim3(256), 0, st, C, rounds, in, ld, width, rate, d, out, n);
    }
}
template <int M>
static void verify_enqueue(bool split, const Fe* C, const VerifyArgs& a, hipStream_t st) {
    if (split) hipLaunchKernelGGL((rescue_tree_verify_split_kernel<M>), dim3(split_grid(a.k, M)), dim3(256), 0, st, C, a);
    else hipLaunchKernelGGL((rescue_tree_verify_wide_kernel<M>), dim3(wide_grid(a.k)), dim3(256), 0, st, C, a);
}
template <int M>
static void trace_enqueue(bool split, const Fe* C, const TraceArgs& a, hipStream_t st) {
    if (split) hipLaunchKernelGGL((rescue_path_trace_split_kernel<M>), dim3(split_grid(a.k, M)), dim3(256), 0, st, C, a);
    else hipLaunchKernelGGL((rescue_path_trace_wide_kernel<M>), dim3(wide_grid(a.k)), dim3(256), 0, st, C, a);
}
#define RM_DISPATCH(m, call, ...)                  \
    switch (m) {                               \
        case 3: call<3>(__VA_ARGS__); break;                \
        case 4: call<4>(__VA_ARGS__); break;                \
        case 5: call<5>(__VA_ARGS__); break;                \
        case 6: call<6>(__VA_ARGS__); break;                \
        case 7: call<7>(__VA_ARGS__); break;                \
        default: call<8>(__VA_ARGS__); break;               \
    }

}  // namespace sci

int sc_rescue_merkle_build_dev(const void* d_rows, uint64_t ld, uint64_t width, uint64_t N, uint64_t digest_len, uint64_t m, uint64_t rate,
                               const void* params, uint64_t rounds, sc_rescue_tree_t** tree, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    const std::string what = "rescue merkle build: ";
    const Shape s{m, rate, digest_len, rounds};
    SCCHK(check_shape(what, s, params));
    if (!d_rows || !tree) return fail(SC_ERR_BAD_ARG, what + "null argument");
    if (width == 0) return fail(SC_ERR_BAD_ARG, what + "rows of at least one element expected");
    if (!is_pow2(N)) return fail(SC_ERR_BAD_ARG, what + "length must be power of two");
    if (ld < N) return fail(SC_ERR_BAD_ARG, what + "a stride below N");
    // the bytes read and the bytes of the tree (128-bit sums: no stride or width can wrap them)
    const u128 in_bytes = (((u128)width - 1) * ld + N) * sizeof(Fe);
    const u128 tree_bytes = (u128)digest_len * (2 * (u128)N - 1) * sizeof(Fe);
    if ((in_bytes >> 64) || (tree_bytes >> 63) || (u128)(uintptr_t)d_rows + in_bytes > ((u128)1 << 64)) return fail(SC_ERR_BAD_ARG, what + "the byte counts wrap");
    if ((N + 255) / 256 > 0x7FFFFFFFull || (N + 7) / 8 > 4 * 0x7FFFFFFFull) return fail(SC_ERR_BAD_ARG, what + "too many leaves for one launch");
    Fe host[MAX_CONSTANTS];
    const uint64_t count = constants_to_mont(s, params, host);
    if (!count) return fail(SC_ERR_BAD_ARG, what + "a constant is not below p");

    hipStream_t st = pick_stream(stream);
    PoolTmpAsync block;                               // the constants: this call's own, for every level
    SCCHK(block.get(sizeof host));
    sc_rescue_tree* t = new sc_rescue_tree;
    t->bytes = (size_t)tree_bytes;
    t->N = N;
    t->logN = ilog2(N);
    t->d = (int)digest_len;
    hipError_t e = pool_alloc((void**)&t->d_levels, t->bytes);
    if (e != hipSuccess) { delete t; return fail(SC_ERR_HIP, hipGetErrorString(e)); }
    auto drop = [&](int code, const std::string& msg) {
        release_after_streams(t->d_levels, t->bytes);
        if (t->done) g_event_pool.push_back(t->done);
        delete t;
        return fail(code, what + msg);
    };
    if (!upload_small(block.p, host, count * sizeof(Fe), st)) return drop(SC_ERR_HIP, "the constants could not be enqueued");
    for (int j = 0; j <= t->logN; ++j) {
        const uint64_t n = N >> j;
        const Fe* in = j ? t->d_levels + rm_level_offset(N, t->d, j - 1) : (const Fe*)d_rows;
        Fe* out = t->d_levels + rm_level_offset(N, t->d, j);
        RM_DISPATCH(m, level_enqueue, split_wanted(n), j == 0, block.fe(), s, in, ld, width, out, n, st);
    }
    if (hipGetLastError() != hipSuccess) return drop(SC_ERR_HIP, "a level could not be enqueued");
    t->done = event_get();
    if (!t->done || hipEventRecord(t->done, st) != hipSuccess) return drop(SC_ERR_HIP, "no event behind the build");
    *tree = t;
    return SC_OK;
}

int sc_rescue_merkle_root(sc_rescue_tree_t* tree, void* root_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !root_out) return fail(SC_ERR_BAD_ARG, "rescue merkle root: null argument");
    HIPCHK(hipStreamWaitEvent(g.stream, tree->done, 0));
    return download(root_out, tree->d_levels + rm_level_offset(tree->N, tree->d, tree->logN), (size_t)tree->d * sizeof(Fe), g.stream);
}

int sc_rescue_merkle_open_batch(const sc_rescue_tree_t* tree, const uint64_t* indices, uint64_t k, void* paths_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    const std::string what = "rescue merkle open: ";
    if (!tree) return fail(SC_ERR_BAD_ARG, what + "null tree");
    if (k && !indices) return fail(SC_ERR_BAD_ARG, what + "null indices");
    // what depends on k alone comes before the scan of the indices: an absurd k is refused without a look at the arrays
    const u128 total128 = (u128)k * tree->logN * tree->d;
    if ((total128 * sizeof(Fe)) >> 63 || ((u128)k * 8) >> 63) return fail(SC_ERR_BAD_ARG, what + "the byte counts wrap");
    const uint64_t total = (uint64_t)total128;
    if ((total + 255) / 256 > 0x7FFFFFFFull) return fail(SC_ERR_BAD_ARG, what + "too many openings for one launch");
    for (uint64_t i = 0; i < k; ++i) if (indices[i] >= tree->N) return fail(SC_ERR_BAD_ARG, what + "cannot open invalid index");
    if (total == 0) return SC_OK;                   // no opening, or a tree of one leaf: the path is empty
    if (!paths_out) return fail(SC_ERR_BAD_ARG, what + "null output");
    PoolTmpAsync d_idx, d_out;
    SCCHK(d_idx.get(k * 8));
    SCCHK(d_out.get(total * sizeof(Fe)));
    HIPCHK(hipStreamWaitEvent(g.stream, tree->done, 0));
    SCCHK(upload(d_idx.p, indices, k * 8, g.stream));
    hipLaunchKernelGGL(rescue_tree_open_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, g.stream, tree->d_levels, tree->N, tree->logN, tree->d,
                       (const uint64_t*)d_idx.p, total, d_out.fe());
    HIPCHK(hipGetLastError());
    return download(paths_out, d_out.p, total * sizeof(Fe), g.stream);
}

int sc_rescue_merkle_level_copy_dev(const sc_rescue_tree_t* tree, uint64_t level, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !d_out) return fail(SC_ERR_BAD_ARG, "rescue merkle level copy: null argument");
    if (level > (uint64_t)tree->logN) return fail(SC_ERR_BAD_ARG, "rescue merkle level copy: level out of range");
    hipStream_t st = pick_stream(stream);
    HIPCHK(hipStreamWaitEvent(st, tree->done, 0));
    HIPCHK(hipMemcpyAsync(d_out, tree->d_levels + rm_level_offset(tree->N, tree->d, (int)level), (size_t)tree->d * (tree->N >> level) * sizeof(Fe), hipMemcpyDeviceToDevice, st));
    return SC_OK;
}

int sc_rescue_merkle_verify_batch(const void* roots, const uint64_t* indices, const void* paths, const void* rows, uint64_t k, uint64_t depth,
                                  uint64_t width, uint64_t digest_len, uint64_t m, uint64_t rate, const void* params, uint64_t rounds, uint8_t* verdicts_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    const std::string what = "rescue merkle verify: ";
    const Shape s{m, rate, digest_len, rounds};
    SCCHK(check_shape(what, s, params));
    if (width == 0) return fail(SC_ERR_BAD_ARG, what + "rows of at least one element expected");
    if (depth > 63) return fail(SC_ERR_BAD_ARG, what + "a depth of at most 63 expected");
    if (k && (!roots || !indices || !rows || !verdicts_out || (depth && !paths))) return fail(SC_ERR_BAD_ARG, what + "null argument");
    // What depends on k alone comes before the scan of the indices: an absurd k is refused without a look at the arrays.
    // One block: [constants][roots][paths][rows][the walks' next messages][indices][verdicts], every part a multiple of 16 bytes but the last.
    const u128 rows128 = (u128)k * width;              // below 2^128; times 16 it would not be
    const u128 root_b = (u128)k * digest_len * sizeof(Fe), path_b = root_b * depth, row_b = (rows128 >> 58) ? ~(u128)0 >> 1 : rows128 * sizeof(Fe), idx_b = ((u128)k * 8 + 15) & ~(u128)15;
    const u128 all = (u128)MAX_CONSTANTS * sizeof(Fe) + 3 * root_b + path_b + idx_b + k;
    if (row_b >> 62 || (all + row_b) >> 62 || (k + 255) / 256 > 0x7FFFFFFFull || (k + 7) / 8 > 4 * 0x7FFFFFFFull) return fail(SC_ERR_BAD_ARG, what + "the byte counts wrap");
    for (uint64_t i = 0; i < k; ++i) if (indices[i] >> depth) return fail(SC_ERR_BAD_ARG, what + "cannot verify invalid index");
    Fe host[MAX_CONSTANTS];
    const uint64_t count = constants_to_mont(s, params, host);
    if (!count) return fail(SC_ERR_BAD_ARG, what + "a constant is not below p");
    if (k == 0) return SC_OK;
    hipStream_t st = g.stream;
    PoolTmpAsync block;
    SCCHK(block.get((size_t)(all + row_b)));
    char* p = (char*)block.p;
    const Fe* C = (const Fe*)p;               p += sizeof host;
    VerifyArgs a;
    a.roots = (const Fe*)p;                   p += (size_t)root_b;
    a.paths = (const Fe*)p;                   p += (size_t)path_b;
    a.rows = (const Fe*)p;                    p += (size_t)row_b;
    a.pair = (Fe*)p;                          p += 2 * (size_t)root_b;
    a.idx = (const uint64_t*)p;               p += (size_t)idx_b;
    a.verdicts = (uint8_t*)p;
    a.k = k; a.width = width; a.depth = (int)depth; a.d = (int)digest_len; a.rate = (int)rate; a.rounds = (int)rounds;
    if (!upload_small((void*)C, host, count * sizeof(Fe), st)) return fail(SC_ERR_HIP, what + "the constants could not be enqueued");
    SCCHK(upload((void*)a.roots, roots, (size_t)root_b, st));
    SCCHK(upload((void*)a.paths, paths, (size_t)path_b, st));
    SCCHK(upload((void*)a.rows, rows, (size_t)row_b, st));
    SCCHK(upload((void*)a.idx, indices, k * 8, st));
    RM_DISPATCH(m, verify_enqueue, split_wanted(k), C, a, st);
    HIPCHK(hipGetLastError());
    return download(verdicts_out, a.verdicts, k, st);
}

int sc_rescue_merkle_path_trace_dev(const void* leaves, const uint64_t* indices, const void* paths, uint64_t k, uint64_t depth, uint64_t digest_len,
                                    uint64_t m, uint64_t rate, const void* params, uint64_t rounds, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    const std::string what = "rescue merkle path trace: ";
    const Shape s{m, rate, digest_len, rounds};
    SCCHK(check_shape(what, s, params));
    if (2 * digest_len >= rate) return fail(SC_ERR_BAD_ARG, what + "a node of one permutation expected: 2 * digest_len < rate");
    if (depth == 0 || depth > 63) return fail(SC_ERR_BAD_ARG, what + "a depth of 1 .. 63 expected");
    if (k && (!leaves || !indices || !paths || !d_out)) return fail(SC_ERR_BAD_ARG, what + "null argument");
    // What depends on k alone comes before the scan of the indices: an absurd k is refused without a look at the arrays.
    // One block of the call's own: [constants][leaves][paths][indices], every part a multiple of 16 bytes.
    const uint64_t W = m + digest_len + 1, T = depth * (rounds + 1) + 1;                  // at most 12 registers, 1765 rows
    const u128 leaf_b = (u128)k * digest_len * sizeof(Fe), path_b = leaf_b * depth, idx_b = ((u128)k * 8 + 15) & ~(u128)15;
    const u128 in_b = (u128)MAX_CONSTANTS * sizeof(Fe) + leaf_b + path_b + idx_b, out_b = (u128)k * W * T * sizeof(Fe);
    if (in_b >> 62 || out_b >> 62 || (u128)(uintptr_t)d_out + out_b > ((u128)1 << 64) || (k + 255) / 256 > 0x7FFFFFFFull || (k + 7) / 8 > 4 * 0x7FFFFFFFull)
        return fail(SC_ERR_BAD_ARG, what + "the byte counts wrap");
    for (uint64_t i = 0; i < k; ++i) if (indices[i] >> depth) return fail(SC_ERR_BAD_ARG, what + "cannot trace invalid index");
    Fe host[MAX_CONSTANTS];
    const uint64_t count = constants_to_mont(s, params, host);
    if (!count) return fail(SC_ERR_BAD_ARG, what + "a constant is not below p");
    if (k == 0) return SC_OK;
    hipStream_t st = pick_stream(stream);
    PoolTmpAsync block;
    SCCHK(block.get((size_t)in_b));
    char* p = (char*)block.p;
    const Fe* C = (const Fe*)p;               p += sizeof host;
    TraceArgs a;
    a.leaves = (const Fe*)p;                  p += (size_t)leaf_b;
    a.paths = (const Fe*)p;                   p += (size_t)path_b;
    a.idx = (const uint64_t*)p;
    a.out = (Fe*)d_out;
    a.k = k; a.T = T; a.depth = (int)depth; a.d = (int)digest_len; a.rounds = (int)rounds;
    if (!upload_small((void*)C, host, count * sizeof(Fe), st)) return fail(SC_ERR_HIP, what + "the constants could not be enqueued");
    // The inputs are the caller's pageable memory.  Few of them travel as kernel arguments and nothing is waited for; otherwise they
    // are copied and the copies -- nothing behind them -- are waited for before the call returns.
    const bool small = upload_small((void*)a.leaves, leaves, (size_t)leaf_b, st) && upload_small((void*)a.paths, paths, (size_t)path_b, st) &&
                       upload_small((void*)a.idx, indices, k * 8, st);
    if (!small) {
        (void)hipGetLastError();
        SCCHK(upload((void*)a.leaves, leaves, (size_t)leaf_b, st));
        SCCHK(upload((void*)a.paths, paths, (size_t)path_b, st));
        SCCHK(upload((void*)a.idx, indices, k * 8, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    switch (m) {
        case 4: trace_enqueue<4>(split_wanted(k), C, a, st); break;
        case 5: trace_enqueue<5>(split_wanted(k), C, a, st); break;
        case 6: trace_enqueue<6>(split_wanted(k), C, a, st); break;
        case 7: trace_enqueue<7>(split_wanted(k), C, a, st); break;
        default: trace_enqueue<8>(split_wanted(k), C, a, st); break;
    }
    HIPCHK(hipGetLastError());
    return SC_OK;
}

uint64_t sc_rescue_merkle_leaves(const sc_rescue_tree_t* tree) { return tree ? tree->N : 0; }

int sc_rescue_merkle_free(sc_rescue_tree_t* tree) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!tree) return SC_OK;
    release_after_streams(tree->d_levels, tree->bytes);
    if (tree->done) g_event_pool.push_back(tree->done);
    delete tree;
    return SC_OK;
}

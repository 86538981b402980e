// core.h -- what the translation units of libstarkcore.so share: the host state (one context per process), the device-memory pool,
// error plumbing, the table caches and the entry points of the transform planner.  Nothing here is part of the C ABI
// (include/starkcore.h is); everything lives in namespace sci and is hidden from the shared object's export table.
//
//   core.hip          state, pool, streams, tables, planner + pass launches, vectors / randomness / transforms / pointwise entries
//   merkle_fri.hip    Merkle trees and forests of them, the FRI fold and commit loop, the Fiat-Shamir transcript, openings
//   merkle_rows.hip   row commitments: one Merkle tree over the rows of a matrix of codewords (csrc/merkle_rows.cuh); the climb is merkle_fri.hip's
//   polytree_geo.hip  subproduct trees and geometric progressions (fast_zerofier / fast_evaluate / fast_interpolate)
//   fourstep.hip      batched transforms, the sharded four-step plan, the RCCL communicator, the direct-store corner turn
//   rescue.hip        the Rescue-Prime permutation (hash and trace; permutation, sponge and states at any width 2 .. 8) over many inputs
//   rescue_merkle.hip Merkle trees over the Rescue-Prime sponge: build, root, openings, batched path verification (csrc/rescue_merkle.cuh)
//   polyeval.hip      polynomials in HBM evaluated at a list of points directly (csrc/polyeval.cuh)
//   columns.hip       division, combination and one deferred verdict over a matrix of polynomial columns (csrc/columns.cuh); the
//                     verifier's combination at the opened points as rows (csrc/combination.cuh)
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cerrno>
#include <thread>
#include <sys/random.h>
#include <deque>
#include <functional>
#include <future>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/starkcore.h"
#pragma GCC visibility pop
#include "ntt_plan.h"

namespace sc { struct FoldIn; struct ForestFold; }          // merkle.cuh, merkle_forest.cuh (their kernels belong to merkle_fri.hip alone)
using namespace sc;

struct sc_vec {
    Fe* d;
    uint64_t n;
    bool owned = true;    // false: a view of memory somebody else owns (sc_vec_wrap: a torch tensor's storage) -- sc_vec_free leaves it alone
};
struct sc_later {           // a few words a kernel will write to a pinned slot (deferred checks: include/starkcore.h sc_later_t)
    int slot;
    uint64_t seq;
    hipStream_t st;
};
struct sc_merkle {
    uint64_t* d_levels;   // (2N-1) digests of 8 x u64
    uint64_t N;
    int logN;
    // asynchronous builds (sc_merkle_build_async_dev, sc_fri_fold_commit_dev): the root is on its way to a pinned host slot;
    // sc_merkle_root waits for `st` once and moves it to `root`
    int slot = -1;
    uint64_t seq = 0;
    hipStream_t st = nullptr;
    bool have_root = false;
    bool lazy = false;    // built "enqueue only" (BUILD_NOROOT): no slot, no publish kernel; the root is copied out if ever asked for
    uint8_t root[64] = {};
};

struct sc_merkle_forest {   // count trees of N leaves, tree-major (csrc/merkle_forest.cuh)
    uint64_t* d_levels;   // count blocks of 2N digests
    uint64_t N, count;
    int logN;
    uint64_t* h_roots = nullptr;   // pinned (the pool of sc_host_alloc): 64 bytes per tree, written by the launch that reaches the roots; behind them the fold's staged c_m
    Fe* d_cm = nullptr;            // the fused fold's per-tree constants (pool), or null
    hipEvent_t done = nullptr;     // recorded behind the build
    hipStream_t st = nullptr;
    bool have_roots = false;
};

namespace sci {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct PlanKey {
    int logn;
    uint64_t lo, hi;
    bool operator<(const PlanKey& o) const { return std::tie(logn, lo, hi) < std::tie(o.logn, o.lo, o.hi); }
};
struct PlanTables {      // power tables of one root of order n = 2^logn
    Fe* mt = nullptr;
    int mt_log = 0;
    Fe* tl = nullptr;
    Fe* th = nullptr;
    Fe* th_ninv = nullptr;   // th * n^-1 (built on first inverse use)
    // direct four-step twiddle tables built so far (direct_twiddles), one per (logA, logR, scaled) of ntt_plan.h's DirectTable:
    // the column passes of plain and batched plans of every digit split share them
    struct Direct { int logA, logR; bool scaled; Fe* d; };
    std::vector<Direct> direct;
    uint64_t last_use = 0;   // lookup tick (eviction order; see evict_tables)
};
struct OuterKey {        // direct outer-twiddle table of one rank's slab (multi-GPU column stage)
    uint64_t lo, hi, order, len, batch, col_base;
    int ninv;
    bool operator<(const OuterKey& o) const { return std::tie(lo, hi, order, len, batch, col_base, ninv) < std::tie(o.lo, o.hi, o.order, o.len, o.batch, o.col_base, o.ninv); }
};
struct OuterTable {
    Fe* d = nullptr;
    uint64_t last_use = 0;
};
struct PowKey {
    uint64_t lo, hi, hi_count;
    bool operator<(const PowKey& o) const { return std::tie(lo, hi, hi_count) < std::tie(o.lo, o.hi, o.hi_count); }
};
struct PowTables {
    Fe* lo = nullptr;
    Fe* hi = nullptr;
    uint64_t last_use = 0;
};

struct Ctx {
    bool init = false;
    int device = -1;
    hipStream_t stream = nullptr;
    std::string err;
    NttTuning tuning;
    std::map<PlanKey, PlanTables> plans;
    std::map<PowKey, PowTables> pows;
    std::map<OuterKey, OuterTable> outers;
    uint64_t tick = 0;       // bumped by every table lookup
    bool foreign_streams = false;   // a caller-owned stream has been used (see pick_stream)
    int small_divisor_direct = 1;    // coset_divide_core evaluates a divisor of <= 8 coefficients point by point instead of transforming it (sc_set_tuning("small_divisor_direct", 0): A/B and tests)
    int div_cols_launch_log = 26;    // sc_coset_divide_columns_later_dev: log2 of the values one set of launches takes (COLS_ELEMS_PER_LAUNCH); smaller: a test hook for the chunk loop
    int tree_cols_launch_log = 26;   // sc_polytree_*_columns_dev: log2 of the elements one temporary of a set of columns holds (COLS_ELEMS_PER_LAUNCH); smaller: a test hook for the set loop
    int eval_chunk_log = 8;          // sc_poly_eval_points_dev: log2 of the coefficients one workgroup takes at least (csrc/polyeval.hip); a test hook that decides how many chunks a small input goes through
    int eval_points_across_min = 32; // sc_poly_eval_points_dev: the number of points (of a call, of a last part-wave) from which the points-across-lanes form is taken ...
    int eval_across_min_products_log = 26;   // ... in calls of at least 2^this many modular products (0: in every call)
    int rescue_tree_split_max_nodes = -1;    // sc_rescue_merkle_*: a level (a batch of paths) of at most this many nodes runs one lane per state register; 0: never, INT32_MAX: always, -1: the measured default (csrc/rescue_merkle.hip SPLIT_MAX_NODES_DEFAULT)
    int grind_window = -1;           // sc_grind*: trials per launch and member; -1: the measured default (csrc/grind.hip GRIND_WINDOW_DEFAULT)
    int grind_unrolled = 0;          // sc_grind*: 1 = the kernel with rounds 1 .. 22 fully unrolled instead of one loop over them (A/B, csrc/grind.cuh)
    int div_cols_chunk = 0;          // columns that share one batch inversion in pointwise_div_cols_kernel; 0: chosen by shape (columns.hip div_cols_chunk_for)
    std::vector<hipStream_t> seen_streams;   // those streams, most recent last (at most SEEN_STREAMS; more: device-wide waits)
    DevBuf scratch[8];       // 0: ntt work, 1..3: poly temporaries, 4: misc small, 5: merkle staging, 6: uploaded operands, 7: degree / exactness flag
    std::map<hipStream_t, DevBuf> ntt_work;   // the work buffer of a multi-pass transform, one per stream: transforms on DIFFERENT streams may be in flight together
    int fast_fixups = 1;     // eight-element kernels: 1 = self-repairing top-limb corrections, 0 = exact arithmetic on every tile, 2 = both kernels on every tile (tests)
    int num_cus = 256;
    int xcd_remap = 1;
    int fixed_shapes = 1;    // use the geometry-specialised kernel instantiations where one matches
    int prio_balance = -1;   // -1: 1 for launches of at most one workgroup per CU, 2 for long grids (>= 8 workgroups per CU; >= 2 of 2^10 x 4 tiles), else 0; 0 / 1 / 2: force (PassParams::prio_balance)
    int wave_local = 1;      // wave-level fences instead of workgroup barriers once a tile's exchanges stay inside one wave
    unsigned long long* trace = nullptr;   // diagnostics: phase stamps of the next fixed-shape pass launches (sc_debug_trace)
    int forest_four_lane_wgs = 256;  // a forest launch of at most this many workgroups runs its narrow levels four lanes per compression (0: never)
    int merkle_big_nlev = 2; // levels fused per launch for Merkle levels wider than FUSE_MAX_W (0: one level kernel per level)
    int fri_tail = -1;       // the persistent tail kernel of Fri.commit (csrc/fri_tail.cuh): -1 = environment STARKCORE_FRI_TAIL (default on), 0 / 1
    int fri_tail_stall = -1; // tests: the host withholds the challenge of this round of the tail kernel (its wait then times out: the abort path)
    size_t verify_stage_bytes = 64ull << 20;   // sc_merkle_verify_batch / sc_fri_colinearity_batch: the pinned staging buffer and its device twin (sc_set_tuning("verify_stage_kb"))
    uint8_t* root_slots = nullptr;        // pinned host memory: roots of asynchronously built Merkle trees in flight
    uint8_t* later_words = nullptr;       // device memory: the flag and degree words of each deferred check, LATER_WORD_BYTES per pinned slot
    uint64_t root_seq = 0;
    std::vector<int> free_root_slots;
};
constexpr int ROOT_SLOTS = 256;
constexpr size_t ROOT_SLOT_BYTES = 128;   // 64-byte root, then the 8-byte sequence number that says it has landed
constexpr size_t LATER_WORD_BYTES = 128;  // a deferred check's device words: DEGREE_SLOTS degree words (64 bytes), then the zero-divisor flag
constexpr long SPIN_POLLS = 40000000;     // ~ tens of milliseconds of polling before the blocking wait

// Frees never wait.  A buffer handed back while a stream may still be using it (the *_dev entries take raw device pointers on
// caller streams, so the library cannot know which) is parked with one event per stream in use -- recorded at the moment of the
// free, i.e. behind everything enqueued so far -- and returns to the pool once those events have completed; that is checked
// when the next buffer is allocated or freed (a query per event, no blocking).
struct PendingFree {
    void* p;
    size_t bytes;
    std::vector<hipEvent_t> evs;
};
#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return fail(SC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
    } while (0)

#define SCCHK(expr)              \
    do {                         \
        int _rc = (expr);        \
        if (_rc != SC_OK) return _rc; \
    } while (0)

struct NttOpts {
    uint64_t in_limit = ~0ull;
    const PowTables* coset = nullptr;
    uint32_t cols = 1;       // independent transforms in one set of launches, column c at element c * n of in / out (NttIo::cols)
    uint64_t col_stride_in = 0;   // ... of `in` at c * col_stride_in instead (0 = n)
};
// elements one set of column launches covers at most (sc_ntt_columns_dev, sc_coset_evaluate_columns_dev, sc_geodomain_interpolate_columns_dev)
constexpr uint64_t COLS_ELEMS_PER_LAUNCH = 1ull << 26;
// a divisor of at most this many coefficients is evaluated point by point on the coset instead of being transformed (small_divisor_direct)
constexpr uint64_t SMALL_DIVISOR = 8;

// Climb from level `lvl` (already in the tree, `N >> lvl` nodes) to the root.  Levels wider than FUSE_MAX_W nodes are
// throughput-bound: launches that fuse merkle_big_nlev (2) levels -- a workgroup's 256 -> 128 -> 64 nodes keep every active
// wave full, and the intermediate levels are not re-read from HBM.  Below FUSE_MAX_W the chain of dependent launches is pure
// latency: fused 8-level subtree launches (most threads idle on the upper levels, which is fine there), then the
// one-workgroup tail.  Measured (tools/merkle_timing.py, profiles/r01/merkle_timing.txt): at 2^24 leaves 2 fused levels
// 2.09 ms, 1 level per launch 2.46 ms, 4 levels 2.50 ms, 8 levels 4.5 ms.
constexpr uint64_t FUSE_MAX_W = 1ull << 17;

enum BuildMode { BUILD_SYNC = 0, BUILD_ASYNC = 1, BUILD_NOROOT = 2 };

// ---- shared host state (defined in core.hip)
extern Ctx g;
extern std::mutex g_mu;
extern hipStream_t g_comm_stream_for_free;      // the library's communication stream once it exists (sc_fourstep_run_dev)
extern std::future<void> g_rand_worker;         // a draw of kernel randomness started ahead of time (sc_urandom_prefetch) ...
extern size_t g_rand_prefetched;                // ... and its size in bytes (0: none in flight)
extern std::multimap<size_t, void*> g_pool;
extern size_t g_pool_bytes, g_pool_cap;
extern std::deque<PendingFree> g_pending;
extern std::vector<hipEvent_t> g_event_pool;

// ---- core.hip: pool, errors, streams, tables, the transform planner
void reap_pending(bool block);
hipError_t pool_alloc(void** p, size_t bytes);
void pool_free(void* p, size_t bytes);
void pool_clear();
hipEvent_t event_get();
int fail(int code, const std::string& msg);
int ensure_init();
int grow_buffer(DevBuf& b, size_t bytes, void** out);
inline int scratch(int slot, size_t bytes, void** out) { return grow_buffer(g.scratch[slot], bytes, out); }
int check_root(Fe root, uint64_t n);
int build_pow_table(Fe** out, uint64_t count, Fe base_m, uint64_t step, Fe scale_m, hipStream_t st);
void free_plans();
int evict_outer_tables();
int get_plan(Fe root, int logn, bool need_ninv, hipStream_t st, PlanTables** out);
inline NttTables tables_of(const PlanTables& t) {
    NttTables tb;
    tb.mt = t.mt; tb.mt_log = t.mt_log; tb.tl = t.tl; tb.th = t.th;
    return tb;
}
int get_pow(Fe base, uint64_t count, hipStream_t st, PowTables** out);
int plan_batched_direct(NttPlanDesc& d, BatchKind kind, int loglen, int logbatch, PlanTables* pt, const Fe* in, Fe* work, Fe* out, BatchExtras ex, hipStream_t st, bool* ok);
int run_plan(NttPlanDesc& d, hipStream_t st);
int ntt_device(const Fe* d_in, Fe* d_out, int logn, Fe root, bool inverse_scale, const NttOpts& o, hipStream_t st);
Fe root_inverse(Fe root, uint64_t n);
int ntt_any(const Fe* d_in, Fe* d_out, uint64_t n, Fe root, bool inverse, const NttOpts& o, hipStream_t st);
int upload(void* d, const void* h, size_t bytes, hipStream_t st);
int download(void* h, const void* d, size_t bytes, hipStream_t st);
int pointwise_div_device(const Fe* a, const Fe* b, Fe* out, uint64_t n, hipStream_t st);
int pointwise_div_enqueue(const Fe* a, const Fe* b, Fe* out, uint64_t n, hipStream_t st, uint32_t* flag);
int gather_device(const Fe* v, const uint64_t* d_idx, uint64_t k, Fe* d_out, hipStream_t st);
int read_small_polled(const void* d_src, size_t bytes, hipStream_t st, void* host_out);
bool upload_small(void* d_dst, const void* host, size_t bytes, hipStream_t st);

// ---- merkle_fri.hip
int merkle_climb(uint64_t* levels, uint64_t N, int lvl, hipStream_t st, volatile uint64_t* host = nullptr, uint64_t seq = 0, bool* published = nullptr);
int merkle_finish(uint64_t* levels, uint64_t width, hipStream_t st);
int root_slot_get();
// A leaf stage other than the decimal one of merkle.cuh (merkle_rows.hip: rows of several columns): called once by merkle_build_device to
// enqueue level 0 of `levels` on `st` -- nlev < 0: that level alone (fewer than 256 leaves); otherwise the leaves and the first nlev
// levels of every 256-leaf subtree in one launch of merkle_subtree_kernel<true, four_lane, ...>.
using LeafStage = std::function<void(uint64_t* levels, uint64_t N, int nlev, bool four_lane, hipStream_t st)>;
int merkle_build_device(const Fe* d_elems, uint64_t N, uint8_t root_out[64], sc_merkle** tree, hipStream_t st, BuildMode mode = BUILD_SYNC, const FoldIn* fold = nullptr,
                        const LeafStage* leaves = nullptr);
// The same for a forest (merkle_rows.hip: a forest whose leaves are rows): called once by forest_build to enqueue the launch that starts
// at level 0 -- `wgs` workgroups of forest_climb_kernel<true, four_lane, false, Rows>, which climb nlev levels and, when that reaches
// the roots, write them to `roots` (else NULL).  forest_args: the shape rules every forest entry shares (N a power of two >= min_n,
// count >= 1, count * N <= SC_FOREST_MAX_LEAVES).  Callers hold g_mu.
using ForestLeafStage = std::function<void(uint64_t* levels, uint64_t N, uint64_t count, int nlev, bool four_lane, unsigned wgs, uint64_t* roots, hipStream_t st)>;
int forest_build(const Fe* d_elems, uint64_t N, uint64_t count, const ForestFold* fold, const std::vector<Fe>* cm, sc_merkle_forest** out, hipStream_t st,
                 const ForestLeafStage* leaves = nullptr);
int forest_args(uint64_t N, uint64_t count, uint64_t min_n);
int wait_polled(std::unique_lock<std::mutex>* lk, hipEvent_t ev);
int merkle_root_wait(sc_merkle* t, bool from_free = false);
void root_poll_unlocked(std::unique_lock<std::mutex>& lk, const sc_merkle* t);
int fold_prepare(const Fe* d_in, uint64_t N, Fe alpha, Fe offset, Fe omega, Fe* d_out, hipStream_t st, FoldIn* f);
int fold_device(const Fe* d_in, uint64_t N, Fe alpha, Fe offset, Fe omega, Fe* d_out, hipStream_t st);
int fold_and_build(const Fe* d_in, uint64_t N, Fe alpha, Fe offset, Fe omega, Fe* d_out, sc_merkle** tree, hipStream_t st);
int fold_constants(uint64_t N, Fe offset, Fe omega, hipStream_t st, PowTables** pw_out, Fe* i2o_m_out);
int host_pool_get(size_t bytes, void** out);
int host_pool_put(void* p);
bool host_pool_holds(const void* p, size_t bytes);
int verify_stage_buffer(size_t bytes, uint8_t** out);   // the batched verifier's pinned staging buffer, grown to `bytes` (one per process; callers hold g_mu)

// ---- merkle_rows.hip: pair leaves for FRI (csrc/fri_pairs.cuh) for a caller that holds g_mu -- the commit phase of sc_fri_prove_pairs_dev
// pair_tree_start: the pair tree of a codeword of n >= 2 elements (n / 2 leaves), enqueued, the root on its way to a pinned slot;
// fold_pairs_and_build: what sc_fri_fold_pairs_commit_dev enqueues (N >= 4)
int pair_tree_start(const Fe* d_codeword, uint64_t n, sc_merkle** tree, hipStream_t st);
int fold_pairs_and_build(const Fe* d_in, uint64_t N, Fe alpha, Fe offset, Fe omega, Fe* d_out, sc_merkle** tree, hipStream_t st);

// ---- grind.hip
// sc_grind_batch for a caller that holds g_mu (and keeps it: sc_fri_prove_grind_dev searches in the middle of its own call)
int grind_seeds_locked(const std::string& what, const void* seeds, uint64_t count, int bits, uint64_t start, uint64_t max_nonces, uint64_t* nonces_out,
                       uint8_t* found_out, void* stream);

// ---- polytree_geo.hip
Fe canonical_root(int logn);
Fe ninv_scaled(int logn, int j);
int ntt_cols(const Fe* in, Fe* out, int loglen, int logbatch, bool inverse, hipStream_t st);

// A caller stream (the *_dev entries take one; sharded.py passes torch's) may still be reading a pooled buffer when it is
// freed: once any foreign stream has been seen, frees wait for the whole device instead of the library stream only.
constexpr size_t SEEN_STREAMS = 8;
inline hipStream_t pick_stream(void* s) {
    if (s && (hipStream_t)s != g.stream) {
        g.foreign_streams = true;
        hipStream_t st = (hipStream_t)s;
        if (g.seen_streams.size() <= SEEN_STREAMS && std::find(g.seen_streams.begin(), g.seen_streams.end(), st) == g.seen_streams.end())
            g.seen_streams.push_back(st);
    }
    return s ? (hipStream_t)s : g.stream;
}
// A buffer goes back to the pool when nothing can still be using it: an event is recorded on the library stream and on every
// caller stream seen so far, and the buffer is parked until they have completed (reap_pending).  A stream that no longer takes
// an event (destroyed by its owner: its work is done) is forgotten; more streams than are tracked: wait for the whole device.
inline void release_after_streams(void* p, size_t bytes) {
    if (!p) return;
    if (g.seen_streams.size() > SEEN_STREAMS) {
        (void)hipDeviceSynchronize();
        g.seen_streams.clear();
        pool_free(p, bytes);
        return;
    }
    PendingFree f{p, bytes, {}};
    auto mark = [&](hipStream_t st) -> bool {
        if (hipStreamQuery(st) == hipSuccess) return true;          // idle: nothing of it can still touch the buffer
        (void)hipGetLastError();
        hipEvent_t e = event_get();
        if (!e) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); return true; }
        if (hipEventRecord(e, st) != hipSuccess) { (void)hipGetLastError(); g_event_pool.push_back(e); return false; }
        f.evs.push_back(e);
        return true;
    };
    if (g.stream) (void)mark(g.stream);
    if (g_comm_stream_for_free) (void)mark(g_comm_stream_for_free);
    for (size_t i = 0; i < g.seen_streams.size();) {
        if (mark(g.seen_streams[i])) ++i;
        else g.seen_streams.erase(g.seen_streams.begin() + i);      // stale handle
    }
    if (f.evs.empty()) { pool_free(p, bytes); return; }
    g_pending.push_back(std::move(f));
    reap_pending(false);
}
inline Fe fe_from(const uint64_t v[2]) { return Fe{v[0], v[1]}; }
inline bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }
inline int ilog2(uint64_t n) { int l = 0; while ((1ull << l) < n) ++l; return l; }

// small RAII holder for pool temporaries
struct PoolTmp {
    void* p = nullptr;
    size_t bytes = 0;
    ~PoolTmp() { if (p) pool_free(p, bytes); }
    int get(size_t b) {
        bytes = b;
        HIPCHK(pool_alloc(&p, b));
        return SC_OK;
    }
    Fe* fe() const { return (Fe*)p; }
};

// pool temporary whose memory goes back once the streams that may still read it have passed this point (nothing here waits)
struct PoolTmpAsync {
    void* p = nullptr;
    size_t bytes = 0;
    ~PoolTmpAsync() { if (p) release_after_streams(p, bytes); }
    int get(size_t b) {
        bytes = b ? b : sizeof(Fe);
        HIPCHK(pool_alloc(&p, bytes));
        return SC_OK;
    }
    Fe* fe() const { return (Fe*)p; }
};

}  // namespace sci
using namespace sci;

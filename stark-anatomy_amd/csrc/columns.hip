// columns.hip -- the kernels of csrc/columns.cuh and their entries: the division of a matrix of polynomial columns (pointwise and on
// a coset, code/ntt.py:159-176 for every column at once), the nonlinear combination of code/fast_stark.py:130-145 in one pass, and ONE
// deferred verdict for all columns of a call (the scheme of sc_coset_divide_later_dev: a one-wave kernel behind the work writes the
// words to a pinned slot, then a sequence number).  Also the verifier's combination at the opened points (csrc/combination.cuh,
// sc_stark_combination_batch), which runs the AIR through mpoly_eval_columns_kernel here.
#include "core.h"
#include "columns.cuh"
#include "mpoly_plan.h"
#include "combination_plan.h"

namespace sci {

static_assert(sizeof(CombineTerm) == sizeof(sc_combine_term_t), "the device term table is the ABI's term array");

__global__ void __launch_bounds__(256) pointwise_div_cols_kernel(const DivCols D) {
    div_cols_thread<DIV_COLS_K>(D, blockIdx.x, blockIdx.y, threadIdx.x, gridDim.x);
}

__global__ void __launch_bounds__(256) short_poly_coset_cols_kernel(const Fe* __restrict__ b, uint64_t ld_b, uint32_t nb, Fe off_m, const Fe* __restrict__ tl,
                                                                   const Fe* __restrict__ th, Fe* __restrict__ out, uint64_t order) {
    short_poly_cols_thread(b, ld_b, nb, off_m, tl, th, out, order, blockIdx.y, (uint64_t)blockIdx.x * COLS_WG + threadIdx.x);
}

// grid (position blocks) x (columns): a wave lies inside one column, so its highest non-zero coefficient above the quotient is one
// atomic (the lanes are in index order: the highest lane that reports holds the highest index)
__global__ void __launch_bounds__(256) unscale_cols_kernel(const UnscaleCols U) {
    const long long r = unscale_cols_thread(U, blockIdx.y, (uint64_t)blockIdx.x * COLS_WG + threadIdx.x);
    const unsigned long long lanes = __ballot(r >= 0);
    if (lanes && (threadIdx.x & 63u) == (unsigned)(63 - __clzll((long long)lanes))) cols_word_max(U.rem + blockIdx.y, r);
}

__global__ void __launch_bounds__(256) combine_cols_kernel(const CombineTerm* __restrict__ terms, uint32_t nterms, const Fe* __restrict__ w_m, Fe* __restrict__ out,
                                                           uint64_t n_out, uint64_t ld_out) {
    const uint64_t i = (uint64_t)blockIdx.x * COLS_WG + threadIdx.x;
    if (i < n_out) out[blockIdx.y * ld_out + i] = combine_cols_elem(terms, nterms, w_m, blockIdx.y, i);
}

// grid (point blocks) x (pairs of member and constraint): the pair is uniform in a workgroup, the tables are read with scalar loads
__global__ void __launch_bounds__(256) mpoly_eval_columns_kernel(const MpolyCols D) {
    mpoly_cols_thread(D, blockIdx.x, blockIdx.y, threadIdx.x);
}

// the verifier's combination rows (csrc/combination.cuh): grid (row blocks) x (variables of the point), and (row blocks); the shared
// description travels as a kernel argument, the verdicts are plain byte stores
__global__ void __launch_bounds__(256) combination_point_kernel(const CombShared S) {
    combination_point_thread(S, blockIdx.x, blockIdx.y, threadIdx.x);
}
__global__ void __launch_bounds__(256) combination_sum_kernel(const CombShared S) {
    combination_sum_thread(S, blockIdx.x, threadIdx.x);
}

__global__ void __launch_bounds__(256) scale_cols_kernel(const Fe* in, uint64_t ld_in, Fe* out, uint64_t ld_out, uint64_t n,
                                                         const Fe* __restrict__ lo, const Fe* __restrict__ hi) {
    scale_cols_thread(in, ld_in, out, ld_out, n, lo, hi, blockIdx.y, (uint64_t)blockIdx.x * COLS_WG + threadIdx.x);
}

// grid (position blocks) x (columns of the batch): one thread per element of the randomized trace matrix
__global__ void __launch_bounds__(256) randomized_cols_kernel(const RandomizedCols D) {
    randomized_cols_thread(D, blockIdx.x, blockIdx.y, threadIdx.x);
}

// one wave: the per-column words -> the words of one pinned slot, published like divide_flags_publish_kernel
__global__ void __launch_bounds__(64) columns_verdict_kernel(const uint32_t* __restrict__ zero, const long long* __restrict__ rem, uint64_t cols,
                                                            volatile uint64_t* host, uint64_t seq) {
    __shared__ long long firsts[64];
    __shared__ uint64_t counts[64];
    verdict_lane(zero, rem, cols, threadIdx.x, &firsts[threadIdx.x], &counts[threadIdx.x]);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t words[4];
        verdict_words(zero, rem, firsts, counts, words);
        for (int k = 0; k < 4; ++k) host[k] = words[k];
        __threadfence_system();
        host[8] = seq;
    }
}

// Columns per workgroup row of the division with a shared divisor.  A thread's batch inversion costs about 190 + 3 * 15 = 235
// products and every column of its chunk 16 more, so a chunk of c columns costs (235 + 16 c) / (16 c) products per element: 15.7 at
// c = 1, 2.8 at c = 8, 1.9 at c = 16, 1.5 at c = 32 -- against one product per 32 bytes moved at which the kernel would be bound by
// memory, gains flatten past 16.  Short columns need the opposite: a 2^10-point column is ONE workgroup of positions, and only the
// chunk rows spread it over the CUs.  So: the largest chunk up to 16 that still leaves two workgroups per CU, else the largest that
// leaves as many workgroups as the columns allow.  (Reasoned, not measured; sc_set_tuning("div_cols_chunk", c > 0) forces c.)
static uint32_t div_cols_chunk_for(uint64_t n, uint64_t cols) {
    if (g.div_cols_chunk > 0) return (uint32_t)g.div_cols_chunk;
    const uint64_t gx = div_cols_grid_x(n), want = 2ull * (uint64_t)g.num_cus;
    uint32_t chunk = 16;
    while (chunk > 1 && gx * ((cols + chunk - 1) / chunk) < want) chunk >>= 1;
    return chunk;
}

static int div_cols_enqueue(const Fe* a, uint64_t ld_a, const Fe* b, uint64_t ld_b, Fe* out, uint64_t ld_out, uint64_t n, uint64_t cols, uint32_t* zero, hipStream_t st) {
    uint64_t chunk = ld_b == 0 ? div_cols_chunk_for(n, cols) : 1;
    if (chunk > cols) chunk = cols;
    while ((cols + chunk - 1) / chunk > 65535) chunk *= 2;               // (grid.y)
    const DivCols D{a, ld_a, b, ld_b, out, ld_out, n, cols, (uint32_t)chunk, zero};
    hipLaunchKernelGGL(pointwise_div_cols_kernel, dim3(div_cols_grid_x(n), (unsigned)((cols + chunk - 1) / chunk)), dim3(COLS_WG), 0, st, D);
    HIPCHK(hipGetLastError());
    return SC_OK;
}

// the per-column device words of one call: cols remainder words (preset to -1), then cols zero-divisor words (preset to 0); they go
// back to the pool behind the streams in use once the call has enqueued its publish kernel
struct ColumnWords {
    PoolTmpAsync mem;
    long long* rem = nullptr;
    uint32_t* zero = nullptr;
    int get(uint64_t cols) {
        SCCHK(mem.get(cols * (sizeof(long long) + sizeof(uint32_t))));
        rem = (long long*)mem.p;
        zero = (uint32_t*)(rem + cols);
        return SC_OK;
    }
    int preset(uint64_t cols, hipStream_t st) {
        HIPCHK(hipMemsetAsync(rem, 0xFF, cols * sizeof(long long), st));
        HIPCHK(hipMemsetAsync(zero, 0, cols * sizeof(uint32_t), st));
        return SC_OK;
    }
};
static int columns_verdict_later(int slot, const ColumnWords& w, bool with_rem, uint64_t cols, hipStream_t st, sc_later** out) {
    const uint64_t seq = ++g.root_seq;
    volatile uint64_t* host = (volatile uint64_t*)(g.root_slots + ROOT_SLOT_BYTES * slot);
    hipLaunchKernelGGL(columns_verdict_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)w.zero, with_rem ? (const long long*)w.rem : nullptr, cols, host, seq);
    HIPCHK(hipGetLastError());
    *out = new sc_later{slot, seq, st};
    return SC_OK;
}
// a deferred entry that failed after reserving its slot: nothing enqueued may still write the slot when it is reused
static int columns_abandon(int slot, hipStream_t st, int rc) {
    (void)hipStreamSynchronize(st);
    g.free_root_slots.push_back(slot);
    return rc;
}
// host words -> device memory of the call's own: as kernel arguments when few (nothing to wait for), else by a copy that is waited for
static int upload_words(void* d_dst, const void* host, size_t bytes, hipStream_t st) {
    if (upload_small(d_dst, host, bytes, st)) return SC_OK;
    (void)hipGetLastError();
    SCCHK(upload(d_dst, host, bytes, st));
    HIPCHK(hipStreamSynchronize(st));
    return SC_OK;
}


// the plan's tables as mpoly_eval_columns_kernel reads them -- coefficients (16-byte elements first), variables, constraints, drops,
// exponent words -- in device memory of the call's own, and the launches over them
struct MpolyTables {
    PoolTmpAsync mem;
    size_t o_coef = 0, o_vars = 0, o_cons = 0, o_drop = 0, o_exps = 0;
    uint32_t nvw = 0;
    int put(const MpolyPlan& P, const std::vector<MpolyVar>& vars, hipStream_t st) {
        const size_t b_coef = P.coef.size() * sizeof(Fe), b_vars = vars.size() * sizeof(MpolyVar), b_cons = P.cons.size() * sizeof(MpolyCons),
                     b_drop = P.drop.size() * sizeof(uint32_t), b_exps = P.exps.size() * sizeof(uint32_t);
        std::vector<uint8_t> table(b_coef + b_vars + b_cons + b_drop + b_exps);
        uint8_t* at = table.data();
        auto add = [&](const void* src, size_t bytes) { if (bytes) memcpy(at, src, bytes); at += bytes; return (size_t)(at - bytes - table.data()); };
        o_coef = add(P.coef.data(), b_coef); o_vars = add(vars.data(), b_vars); o_cons = add(P.cons.data(), b_cons); o_drop = add(P.drop.data(), b_drop);
        o_exps = add(P.exps.data(), b_exps);
        nvw = P.nvw;
        SCCHK(mem.get(table.size() + 8));
        return upload_words(mem.p, table.data(), table.size(), st);
    }
    int launch(const Fe* vals, uint64_t n, uint64_t members, uint64_t ncons, Fe* out, uint64_t ld_out, hipStream_t st) const {
        const uint8_t* T = (const uint8_t*)mem.p;
        const uint64_t pairs = members * ncons;
        for (uint64_t pair0 = 0; pair0 < pairs; pair0 += COLS_GRID_ROWS) {
            const uint64_t rows = pairs - pair0 < COLS_GRID_ROWS ? pairs - pair0 : COLS_GRID_ROWS;
            const MpolyCols D{vals, (const MpolyVar*)(T + o_vars), (const MpolyCons*)(T + o_cons), (const Fe*)(T + o_coef), (const uint32_t*)(T + o_drop),
                              (const uint32_t*)(T + o_exps), nvw, (uint32_t)ncons, n, out, ld_out, (uint32_t)pair0};
            hipLaunchKernelGGL(mpoly_eval_columns_kernel, dim3((unsigned)((n + COLS_WG - 1) / COLS_WG), (unsigned)rows), dim3(COLS_WG), 0, st, D);
            HIPCHK(hipGetLastError());
        }
        return SC_OK;
    }
};

}  // namespace sci

int sc_pointwise_div_columns_later_dev(const void* d_a, uint64_t ld_a, const void* d_b, uint64_t ld_b, void* d_out, uint64_t ld_out, uint64_t n, uint64_t cols,
                                       sc_later_t** later, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!later || !d_a || !d_b || !d_out || !n || !cols) return fail(SC_ERR_BAD_ARG, "null argument");
    if (ld_a < n || ld_out < n || (ld_b != 0 && ld_b < n)) return fail(SC_ERR_BAD_ARG, "a column stride below the column length");
    if (d_out == d_a && ld_out != ld_a && cols > 1) return fail(SC_ERR_BAD_ARG, "in place needs the numerator's column stride");
    hipStream_t st = pick_stream(stream);
    const int slot = root_slot_get();
    if (slot < 0) return fail(SC_ERR_UNSUPPORTED, "no pinned slot free for a deferred check (nothing enqueued)");
    ColumnWords w;
    if (int rc = w.get(cols)) { g.free_root_slots.push_back(slot); return rc; }      // (nothing enqueued yet)
    const int rc = [&]() -> int {
        SCCHK(w.preset(cols, st));
        SCCHK(div_cols_enqueue((const Fe*)d_a, ld_a, (const Fe*)d_b, ld_b, (Fe*)d_out, ld_out, n, cols, w.zero, st));
        return columns_verdict_later(slot, w, false, cols, st, later);
    }();
    return rc == SC_OK ? SC_OK : columns_abandon(slot, st, rc);
}

int sc_coset_divide_columns_later_dev(const void* d_a, uint64_t na, uint64_t ld_a, const void* d_b, uint64_t nb, uint64_t ld_b, uint64_t cols,
                                      const uint64_t offset[2], const uint64_t root[2], uint64_t order, void* d_out, const uint64_t* n_out, uint64_t ld_out,
                                      sc_later_t** later, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!later || !d_a || !d_b || !n_out || !cols || !offset || !root) return fail(SC_ERR_BAD_ARG, "null argument");
    if (!is_pow2(order) || order < 2) return fail(SC_ERR_NOT_POW2, "cannot compute ntt of non-power-of-two sequence");
    if (na > order || nb > order || na == 0 || nb == 0) return fail(SC_ERR_BAD_ARG, "operand longer than the transform order");
    if (ld_a < na || (ld_b != 0 && ld_b < nb)) return fail(SC_ERR_BAD_ARG, "a column stride below the column length");
    uint64_t longest = 0;
    for (uint64_t c = 0; c < cols; ++c) {
        if (n_out[c] > order) return fail(SC_ERR_BAD_ARG, "operand longer than the transform order");
        longest = n_out[c] > longest ? n_out[c] : longest;
    }
    if (ld_out < longest || (longest && !d_out)) return fail(SC_ERR_BAD_ARG, "a column stride below the column length");
    const Fe rt = fe_from(root), off = fe_from(offset);
    SCCHK(check_root(rt, order));
    if (fe_is_zero(off) || fe_ge_p(off)) return fail(SC_ERR_BAD_ARG, "bad coset offset");
    hipStream_t st = pick_stream(stream);
    const int slot = root_slot_get();
    if (slot < 0) return fail(SC_ERR_UNSUPPORTED, "no pinned slot free for a deferred check (nothing enqueued)");
    // one set of launches takes COLS_ELEMS_PER_LAUNCH values (and grid.y 65 535 columns): more columns go in chunks that report into
    // the same per-column words.  The value matrices are this call's own.  (sc_set_tuning("div_cols_launch_log") lowers the limit so
    // that a test reaches the chunk loop with small matrices.)
    static_assert(COLS_ELEMS_PER_LAUNCH == 1ull << 26, "div_cols_launch_log's default and upper end");
    const bool shared = ld_b == 0;
    uint64_t per = (1ull << g.div_cols_launch_log) / order;
    if (per < 1) per = 1;
    if (per > 65535) per = 65535;
    if (per > cols) per = cols;
    ColumnWords w;
    PoolTmpAsync va, vb, vd, keep;
    const int got = [&]() -> int {
        SCCHK(w.get(cols));
        SCCHK(va.get(per * order * sizeof(Fe)));
        SCCHK(vb.get(per * order * sizeof(Fe)));
        SCCHK(vd.get((shared ? 1 : per) * order * sizeof(Fe)));
        return keep.get(cols * sizeof(uint64_t));
    }();
    if (got != SC_OK) { g.free_root_slots.push_back(slot); return got; }           // (nothing enqueued yet)
    const int rc = [&]() -> int {
        const int logn = ilog2(order);
        SCCHK(w.preset(cols, st));
        SCCHK(upload_words(keep.p, n_out, cols * sizeof(uint64_t), st));
        PowTables *pw, *pinv;
        SCCHK(get_pow(off, order, st, &pw));
        SCCHK(get_pow(from_mont(mont_inv(to_mont(off))), order, st, &pinv));       // unscale by offset^-1 (ntt.py:176)
        const bool direct = nb <= SMALL_DIVISOR && g.small_divisor_direct;
        PlanTables* pt = nullptr;
        if (direct) SCCHK(get_plan(rt, logn, false, st, &pt));
        const unsigned xblocks = (unsigned)((order + COLS_WG - 1) / COLS_WG);
        // the divisors' values on the coset: `k` rows from `b` (a shared divisor: one row, once)
        auto divisor_values = [&](const Fe* b, uint64_t k) -> int {
            if (direct) {
                hipLaunchKernelGGL(short_poly_coset_cols_kernel, dim3(xblocks, (unsigned)k), dim3(COLS_WG), 0, st, b, ld_b, (uint32_t)nb, to_mont(off), (const Fe*)pt->tl,
                                   (const Fe*)pt->th, vd.fe(), order);
                HIPCHK(hipGetLastError());
                return SC_OK;
            }
            NttOpts o;
            o.coset = pw;
            o.in_limit = nb;
            o.cols = (uint32_t)k;
            o.col_stride_in = ld_b;
            return ntt_device(b, vd.fe(), logn, rt, false, o, st);
        };
        if (shared) SCCHK(divisor_values((const Fe*)d_b, 1));
        for (uint64_t done = 0; done < cols; done += per) {
            const uint64_t k = cols - done < per ? cols - done : per;
            NttOpts o;
            o.coset = pw;
            o.in_limit = na;
            o.cols = (uint32_t)k;
            o.col_stride_in = ld_a;
            SCCHK(ntt_device((const Fe*)d_a + done * ld_a, va.fe(), logn, rt, false, o, st));
            if (!shared) SCCHK(divisor_values((const Fe*)d_b + done * ld_b, k));
            SCCHK(div_cols_enqueue(va.fe(), order, vd.fe(), shared ? 0 : order, va.fe(), order, order, k, w.zero + done, st));
            NttOpts back;
            back.cols = (uint32_t)k;
            SCCHK(ntt_device(va.fe(), vb.fe(), logn, root_inverse(rt, order), true, back, st));
            const UnscaleCols U{vb.fe(), order, (Fe*)d_out + done * ld_out, ld_out, (const uint64_t*)keep.p + done, pinv->lo, pinv->hi, w.rem + done};
            hipLaunchKernelGGL(unscale_cols_kernel, dim3(xblocks, (unsigned)k), dim3(COLS_WG), 0, st, U);
            HIPCHK(hipGetLastError());
        }
        return columns_verdict_later(slot, w, true, cols, st, later);
    }();
    return rc == SC_OK ? SC_OK : columns_abandon(slot, st, rc);
}

int sc_combine_columns_dev(const sc_combine_term_t* terms, uint64_t nterms, const void* weights, uint64_t cols, void* d_out, uint64_t n_out, uint64_t ld_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (cols == 0 || n_out == 0) return SC_OK;
    if (!terms || !weights || !d_out || nterms == 0 || nterms > 0xFFFFFFFFull) return fail(SC_ERR_BAD_ARG, nterms ? "null argument" : "a combination of no terms");
    if (ld_out < n_out || cols > 65535) return fail(SC_ERR_BAD_ARG, cols > 65535 ? "more than 65 535 columns" : "a column stride below the column length");
    hipStream_t st = pick_stream(stream);
    const uintptr_t out_lo = (uintptr_t)d_out, out_hi = out_lo + ((cols - 1) * ld_out + n_out) * sizeof(Fe);
    // the table as the kernel reads it: the terms, then the weights in Montgomery form
    const size_t tbytes = nterms * sizeof(CombineTerm), wbytes = cols * nterms * sizeof(Fe);
    std::vector<uint8_t> table(tbytes + wbytes);
    CombineTerm* T = (CombineTerm*)table.data();
    Fe* W = (Fe*)(table.data() + tbytes);
    for (uint64_t t = 0; t < nterms; ++t) {
        const sc_combine_term_t& s = terms[t];
        if (s.shift + s.n > n_out || s.shift + s.n < s.shift) return fail(SC_ERR_BAD_ARG, "shifted term does not fit the output");
        if (s.n) {
            if (!s.d_src || s.ld < s.n) return fail(SC_ERR_BAD_ARG, s.d_src ? "a column stride below the column length" : "null argument");
            const uintptr_t lo = (uintptr_t)s.d_src, hi = lo + ((cols - 1) * s.ld + s.n) * sizeof(Fe);
            if (lo < out_hi && out_lo < hi) return fail(SC_ERR_BAD_ARG, "the output may not alias a source");
        }
        T[t] = CombineTerm{(const Fe*)s.d_src, s.ld, s.n, s.shift};
    }
    const Fe* w = (const Fe*)weights;
    for (uint64_t k = 0; k < cols * nterms; ++k) {
        if (fe_ge_p(w[k])) return fail(SC_ERR_BAD_ARG, "weight is not a canonical residue");
        W[k] = to_mont(w[k]);
    }
    PoolTmpAsync d_table;
    SCCHK(d_table.get(table.size() + 8));
    SCCHK(upload_words(d_table.p, table.data(), table.size(), st));
    hipLaunchKernelGGL(combine_cols_kernel, dim3((unsigned)((n_out + COLS_WG - 1) / COLS_WG), (unsigned)cols), dim3(COLS_WG), 0, st,
                       (const CombineTerm*)d_table.p, (uint32_t)nterms, (const Fe*)((const uint8_t*)d_table.p + tbytes), (Fe*)d_out, n_out, ld_out);
    HIPCHK(hipGetLastError());
    return SC_OK;
}

// MPolynomial.evaluate_symbolic in the value domain for `members` point sets and `ncons` constraints in one launch
int sc_mpoly_eval_columns_dev(const void* d_vals, uint64_t nvars, uint64_t n, uint64_t members, const uint64_t* var_base, const uint64_t* var_ld, const uint32_t* var_src,
                              const uint64_t* var_rot, uint64_t ncons, const uint64_t* nterms, const uint8_t* exps, const void* coefs, void* d_out, uint64_t ld_out,
                              void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (members == 0 || ncons == 0) return SC_OK;
    if (!d_vals || !d_out || !var_base || !var_ld || !nterms) return fail(SC_ERR_BAD_ARG, "null argument");
    if ((var_src == nullptr) != (var_rot == nullptr)) return fail(SC_ERR_BAD_ARG, "var_src and var_rot come together");
    if (nvars == 0 || nvars > 255) return fail(SC_ERR_BAD_ARG, "between 1 and 255 variables");
    if (ld_out < n) return fail(SC_ERR_BAD_ARG, "a column stride below the column length");
    if (members > 0xFFFFFFFFull / ncons) return fail(SC_ERR_BAD_ARG, "more than 2^32 - 1 results");
    uint64_t total = 0;
    for (uint64_t c = 0; c < ncons; ++c) total += nterms[c];
    if (total && (!exps || !coefs)) return fail(SC_ERR_BAD_ARG, "null argument");
    MpolyPlan P;
    if (const char* what = mpoly_plan_build((uint32_t)nvars, ncons, nterms, exps, (const Fe*)coefs, P)) return fail(SC_ERR_BAD_ARG, what);
    std::vector<MpolyVar> vars;
    const char* what = nullptr;
    if (const int bad = mpoly_vars_resolve((uint32_t)nvars, n, var_base, var_ld, var_src, var_rot, P.used, vars, &what)) return fail(bad == 2 ? SC_ERR_NOT_POW2 : SC_ERR_BAD_ARG, what);
    if (n == 0) return SC_OK;
    const uint64_t pairs = members * ncons;
    const uintptr_t out_lo = (uintptr_t)d_out, out_hi = out_lo + ((pairs - 1) * ld_out + n) * sizeof(Fe);
    for (uint64_t j = 0; j < nvars; ++j) {
        if (!P.used[j]) continue;
        const uintptr_t lo = (uintptr_t)d_vals + vars[j].base * sizeof(Fe), hi = lo + ((members - 1) * vars[j].ld + n) * sizeof(Fe);
        if (lo < out_hi && out_lo < hi) return fail(SC_ERR_BAD_ARG, "the output may not overlap the values");
    }
    hipStream_t st = pick_stream(stream);
    MpolyTables tables;
    SCCHK(tables.put(P, vars, st));
    return tables.launch((const Fe*)d_vals, n, members, ncons, (Fe*)d_out, ld_out, st);
}

// FastStark.verify_batch's combination check at the opened points (csrc/combination.cuh): per chunk of staged rows the point matrix,
// the AIR under the plan above (members = 1, n = the chunk's rows: ONE launch for all constraints) and the weighted sum, on the
// library stream with one wait.  What every chunk reads -- weights, coefficient pool, the members' lists, shifts, the plan -- is
// uploaded once; the chunks' rows and verdicts go through the bounded pinned buffer of the other two verifier entries.
int sc_stark_combination_batch(const sc_combination_t* shared, const void* rows, uint64_t n, uint8_t* verdicts_out) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (n == 0) return SC_OK;
    if (!shared || !rows || !verdicts_out) return fail(SC_ERR_BAD_ARG, "null argument");
    const sc_combination_t& c = *shared;
    CombTables T;
    if (const char* what = combination_prepare(c, rows, n, T)) return fail(SC_ERR_BAD_ARG, what);
    if (T.undecided) {
        memset(verdicts_out, CB_UNDECIDED, n);
        return SC_OK;
    }
    const uint32_t w = (uint32_t)c.registers, ncons = (uint32_t)c.ncons, nvars = 1 + 2 * w;
    const uint64_t stride = comb_row_bytes(w);
    const size_t cap = g.verify_stage_bytes;
    const uint64_t fit = combination_chunk_rows(cap, w), per = n < fit ? n : fit;
    auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t rows_b = align(per * stride);
    uint8_t* stage;
    SCCHK(verify_stage_buffer(cap, &stage));
    hipStream_t st = g.stream;
    // [weights][pool][lists][shifts][member flags]: 16-byte elements first
    const size_t b_w = T.weights_m.size() * sizeof(Fe), b_pool = c.pool_len * sizeof(Fe), b_polys = 2 * c.members * w * sizeof(CombPoly),
                 b_shifts = T.shifts.size() * sizeof(uint64_t), b_bad = c.members;
    std::vector<uint8_t> table(b_w + b_pool + b_polys + b_shifts + b_bad);
    memcpy(table.data(), T.weights_m.data(), b_w);
    if (b_pool) memcpy(table.data() + b_w, c.pool, b_pool);
    memcpy(table.data() + b_w + b_pool, c.polys, b_polys);
    memcpy(table.data() + b_w + b_pool + b_polys, T.shifts.data(), b_shifts);
    memcpy(table.data() + b_w + b_pool + b_polys + b_shifts, T.member_bad.data(), b_bad);
    PoolTmpAsync d_table, d_stage, d_vals;
    SCCHK(d_table.get(table.size() + 8));
    SCCHK(d_stage.get(rows_b + align(per)));
    SCCHK(d_vals.get((size_t)(nvars + ncons) * per * sizeof(Fe)));
    SCCHK(upload_words(d_table.p, table.data(), table.size(), st));
    MpolyTables plan;
    if (ncons) SCCHK(plan.put(T.plan, combination_vars(w, per), st));
    const uint8_t* D = (const uint8_t*)d_table.p;
    uint8_t* d_rows = (uint8_t*)d_stage.p;
    Fe* vals = d_vals.fe();
    Fe* tq = vals + (size_t)nvars * per;
    for (uint64_t i = 0; i < n; i += per) {
        const uint64_t count = n - i < per ? n - i : per;
        memcpy(stage, (const uint8_t*)rows + i * stride, count * stride);
        HIPCHK(hipMemcpyAsync(d_rows, stage, count * stride, hipMemcpyHostToDevice, st));
        const CombShared S{d_rows, count, w, ncons, T.generator_m, T.omega_m, c.domain_length - 1, c.step, (const CombPoly*)(D + b_w + b_pool),
                           (const Fe*)(D + b_w), (const Fe*)D, D + b_w + b_pool + b_polys + b_shifts, (const uint64_t*)(D + b_w + b_pool + b_polys),
                           vals, per, tq, d_rows + rows_b};
        const unsigned gx = (unsigned)((count + COLS_WG - 1) / COLS_WG);
        hipLaunchKernelGGL(combination_point_kernel, dim3(gx, nvars), dim3(COLS_WG), 0, st, S);
        HIPCHK(hipGetLastError());
        if (ncons) SCCHK(plan.launch(vals, count, 1, ncons, tq, per, st));
        hipLaunchKernelGGL(combination_sum_kernel, dim3(gx), dim3(COLS_WG), 0, st, S);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(stage + rows_b, d_rows + rows_b, count, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        memcpy(verdicts_out + i, stage + rows_b, count);
    }
    return SC_OK;
}

// Polynomial.scale for the rows of a matrix: out[c][i] = in[c][i] * factor^i
int sc_scale_columns_dev(const void* d_in, uint64_t ld_in, void* d_out, uint64_t ld_out, uint64_t n, uint64_t cols, const uint64_t factor[2], void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (n == 0 || cols == 0) return SC_OK;
    if (!d_in || !d_out || !factor) return fail(SC_ERR_BAD_ARG, "null argument");
    if (ld_in < n || ld_out < n) return fail(SC_ERR_BAD_ARG, "a column stride below the column length");
    if (d_out == d_in && ld_out != ld_in && cols > 1) return fail(SC_ERR_BAD_ARG, "in place needs the input's column stride");
    if (fe_ge_p(fe_from(factor))) return fail(SC_ERR_BAD_ARG, "factor is not a canonical residue");
    hipStream_t st = pick_stream(stream);
    PowTables* pw;
    SCCHK(get_pow(fe_from(factor), n, st, &pw));
    for (uint64_t done = 0; done < cols; done += COLS_GRID_ROWS) {
        const uint64_t k = cols - done < COLS_GRID_ROWS ? cols - done : COLS_GRID_ROWS;
        hipLaunchKernelGGL(scale_cols_kernel, dim3((unsigned)((n + COLS_WG - 1) / COLS_WG), (unsigned)k), dim3(COLS_WG), 0, st, (const Fe*)d_in + done * ld_in, ld_in,
                           (Fe*)d_out + done * ld_out, ld_out, n, (const Fe*)pw->lo, (const Fe*)pw->hi);
        HIPCHK(hipGetLastError());
    }
    return SC_OK;
}

// the randomized trace matrix of a batch of proofs: every member's trace columns with the randomizer rows sampled behind them
int sc_randomized_columns_dev(const void* d_trace, uint64_t rows, uint64_t ld_trace, uint64_t members, uint64_t registers, const void* draws, uint64_t draws_stride,
                              uint64_t extra, uint32_t width, void* d_out, uint64_t ld_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (members == 0 || registers == 0 || (rows == 0 && extra == 0)) return SC_OK;
    if (width == 0 || width > 32) return fail(SC_ERR_BAD_ARG, "byte strings of 1..32 bytes expected");
    if (rows + extra < rows || ld_out < rows + extra || ld_trace < rows) return fail(SC_ERR_BAD_ARG, "a column stride below the column length");
    if (!d_out || (rows && !d_trace) || (extra && !draws)) return fail(SC_ERR_BAD_ARG, "null argument");
    if (members > (1ull << 32) / registers || extra > (1ull << 40) / (registers * width)) return fail(SC_ERR_BAD_ARG, "more than 2^32 columns or 2^40 bytes of draws per member");
    const uint64_t block = extra * registers * width, cols = members * registers, n = rows + extra;
    if (members > 1 && draws_stride < block) return fail(SC_ERR_BAD_ARG, "the members' draws overlap");
    if (rows) {
        const uintptr_t out_lo = (uintptr_t)d_out, out_hi = out_lo + ((cols - 1) * ld_out + n) * sizeof(Fe);
        const uintptr_t lo = (uintptr_t)d_trace, hi = lo + ((cols - 1) * ld_trace + rows) * sizeof(Fe);
        if (lo < out_hi && out_lo < hi) return fail(SC_ERR_BAD_ARG, "the output may not overlap the trace");
    }
    hipStream_t st = pick_stream(stream);
    // the draws as the kernel reads them: the members' blocks one behind the other (pooled scratch, like sc_sample_bytes_dev)
    void* buf = nullptr;
    std::vector<uint8_t> packed;
    if (block) {
        SCCHK(scratch(6, members * block + 256, &buf));
        const uint8_t* src = (const uint8_t*)draws;
        if (members > 1 && draws_stride != block) {
            packed.resize(members * block);
            for (uint64_t m = 0; m < members; ++m) memcpy(packed.data() + m * block, src + m * draws_stride, block);
            src = packed.data();
        }
        SCCHK(upload(buf, src, members * block, st));
    }
    for (uint64_t done = 0; done < cols; done += COLS_GRID_ROWS) {
        const uint64_t k = cols - done < COLS_GRID_ROWS ? cols - done : COLS_GRID_ROWS;
        const RandomizedCols D{(const Fe*)d_trace, rows, ld_trace, registers, (const uint8_t*)buf, block, extra, width, (Fe*)d_out, ld_out, done};
        hipLaunchKernelGGL(randomized_cols_kernel, dim3((unsigned)((n + COLS_WG - 1) / COLS_WG), (unsigned)k), dim3(COLS_WG), 0, st, D);
        HIPCHK(hipGetLastError());
    }
    if (block) HIPCHK(hipStreamSynchronize(st));    // `draws` is the caller's host memory
    return SC_OK;
}

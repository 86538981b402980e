// polytree_geo.hip -- fast_zerofier / fast_evaluate / fast_interpolate (code/ntt.py:66-130): the subproduct tree over arbitrary points
// (polytree.cuh) and the closed forms on geometric progressions (geoseq.cuh), resident in HBM.
#include "core.h"
#include "polytree.cuh"
#include "geoseq.cuh"
#include "polydiv.cuh"
#include "polymul.cuh"

namespace sci {

// ============================================================================ subproduct tree (polytree.cuh)

// primitive 2^logn-th root the tree's internal transforms use: Field.primitive_nth_root (algebra.py:104-111), i.e. the
// order-2^119 constant squared 119 - logn times.  The results of sc_polytree_* do not depend on which roots are used.
Fe canonical_root(int logn) {
    static Fe cache[120];
    static bool have[120] = {false};
    if (!have[logn]) {
        Fe r = to_mont(Fe{0xb5038f9c18f6f7d1ull, 0x4040fbed12ee470full});
        for (int i = 119; i > logn; --i) r = mont_mul(r, r);
        cache[logn] = from_mont(r);
        have[logn] = true;
    }
    return cache[logn];
}

// c * R^j (mod p) for c = (2^logn)^-1: the constant a pointwise kernel multiplies by to apply the inverse transform's n^-1
// and cancel the R^-1 factors of its j Montgomery products
Fe ninv_scaled(int logn, int j) {
    Fe c = from_mont(mont_inv(to_mont(Fe{1ull << logn, 0})));
    for (int i = 0; i < j; ++i) c = to_mont(c);
    return c;
}

inline unsigned pt_blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

// transform along axis 0 of a [2^loglen][2^logbatch] array (natural order, out != in); the inverse uses root^-1 and does NOT
// scale by n^-1 (the pointwise kernel in front of it does)
int ntt_cols(const Fe* in, Fe* out, int loglen, int logbatch, bool inverse, hipStream_t st) {
    const uint64_t len = 1ull << loglen, B = 1ull << logbatch;
    if (loglen == 0) {
        if (in != out) HIPCHK(hipMemcpyAsync(out, in, B * sizeof(Fe), hipMemcpyDeviceToDevice, st));
        return SC_OK;
    }
    Fe rt = canonical_root(loglen);
    if (inverse) rt = root_inverse(rt, len);
    if (logbatch == 0) return ntt_device(in, out, loglen, rt, false, NttOpts(), st);
    PlanTables* pt;
    SCCHK(get_plan(rt, loglen, false, st, &pt));
    void* w;
    SCCHK(scratch(0, len * B * sizeof(Fe), &w));
    NttPlanDesc d;
    bool planned = false;
    SCCHK(plan_batched_direct(d, BATCH_COLS, loglen, logbatch, pt, in, (Fe*)w, out, BatchExtras(), st, &planned));
    if (planned) return run_plan(d, st);
    // columns longer than the batched plans take (only the top few levels of a big tree, a handful of columns each)
    void *a, *b;
    SCCHK(scratch(1, len * sizeof(Fe), &a));
    SCCHK(scratch(2, len * sizeof(Fe), &b));
    for (uint64_t c = 0; c < B; ++c) {
        hipLaunchKernelGGL(pt_col_gather_kernel, dim3(pt_blocks(len)), dim3(256), 0, st, in, len, B, c, (Fe*)a);
        SCCHK(ntt_device((const Fe*)a, (Fe*)b, loglen, rt, false, NttOpts(), st));
        hipLaunchKernelGGL(pt_col_scatter_kernel, dim3(pt_blocks(len)), dim3(256), 0, st, (const Fe*)b, len, B, c, out);
    }
    HIPCHK(hipGetLastError());
    return SC_OK;
}

}  // namespace sci

struct sc_polytree {
    uint64_t k, K;
    int L;
    Fe* zc;        // (L+1) levels of K entries: level l at zc + l*K, [2^l][K >> l], monic top coefficient implicit
    Fe* zf;        // L levels of 2K entries: level l at zf + l*2K, [2^(l+1)][K >> l] = transforms of level l at twice its size
    Fe* invg_f;    // size-2K transform of rev(Z)^-1 mod y^K (built by the first evaluation)
    size_t zc_bytes, zf_bytes;
    Fe* winv_m = nullptr;   // k: 1 / Z'(d_i) as Montgomery forms, Z = the zerofier of the k real points (built by the first column interpolation)
    Fe* winv0_m = nullptr;  // k: inv0(Z'(d_i)), 0 where the derivative is (built by the first Lagrange interpolation); IS winv_m where that existed already
};

namespace {

int polytree_build(const Fe* d_points, uint64_t k, sc_polytree** out, hipStream_t st) {
    if (k == 0) return fail(SC_ERR_BAD_ARG, "empty domain");
    int L = 0;
    while ((1ull << L) < k) ++L;
    if (L > 30) return fail(SC_ERR_UNSUPPORTED, "domain too large");
    const uint64_t K = 1ull << L;
    sc_polytree* t = new sc_polytree{k, K, L, nullptr, nullptr, nullptr, (size_t)(L + 1) * K * sizeof(Fe), (size_t)(L ? L : 1) * 2 * K * sizeof(Fe)};
    hipError_t e = pool_alloc((void**)&t->zc, t->zc_bytes);
    if (e == hipSuccess) e = pool_alloc((void**)&t->zf, t->zf_bytes);
    if (e != hipSuccess) {
        if (t->zc) pool_free(t->zc, t->zc_bytes);
        delete t;
        return fail(SC_ERR_HIP, hipGetErrorString(e));
    }
    auto cleanup = [&](int rc) { pool_free(t->zc, t->zc_bytes); pool_free(t->zf, t->zf_bytes); delete t; return rc; };
    PoolTmp buf, buf2;
    int rc = buf.get(2 * K * sizeof(Fe));
    if (rc == SC_OK) rc = buf2.get(K * sizeof(Fe));
    if (rc != SC_OK) return cleanup(rc);
    hipLaunchKernelGGL(pt_leaves_kernel, dim3(pt_blocks(K)), dim3(256), 0, st, d_points, k, t->zc, K);
    for (int l = 0; l < L && rc == SC_OK; ++l) {
        const uint64_t B = K >> l;
        Fe* zcl = t->zc + (uint64_t)l * K;
        Fe* zfl = t->zf + (uint64_t)l * 2 * K;
        hipLaunchKernelGGL(pt_expand_kernel, dim3(pt_blocks(2 * K)), dim3(256), 0, st, (const Fe*)zcl, buf.fe(), K, B, (uint64_t)1);
        rc = ntt_cols(buf.fe(), zfl, l + 1, L - l, false, st);
        if (rc != SC_OK) break;
        hipLaunchKernelGGL(pt_mul_pairs_kernel, dim3(pt_blocks(K)), dim3(256), 0, st, (const Fe*)zfl, buf2.fe(), K, ninv_scaled(l + 1, 2));
        rc = ntt_cols(buf2.fe(), zcl + K, l + 1, L - l - 1, true, st);
        if (rc != SC_OK) break;
        hipLaunchKernelGGL(pt_sub_one_kernel, dim3(pt_blocks(B / 2)), dim3(256), 0, st, zcl + K, B / 2);
    }
    if (rc == SC_OK && hipGetLastError() != hipSuccess) rc = fail(SC_ERR_HIP, "polytree build launch failed");
    if (rc == SC_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(SC_ERR_HIP, "polytree build failed");
    if (rc != SC_OK) return cleanup(rc);
    *out = t;
    return SC_OK;
}

// rev(Z)^-1 mod y^K by Newton iteration (h <- h (2 - G h), precision doubling), kept as its size-2K transform
int polytree_inverse_series(sc_polytree* t, hipStream_t st) {
    if (t->invg_f || t->L == 0) return SC_OK;
    const uint64_t K = t->K;
    const int L = t->L;
    PoolTmp G, h, H, T;
    SCCHK(G.get(K * sizeof(Fe)));
    SCCHK(h.get(2 * K * sizeof(Fe)));
    SCCHK(H.get(2 * K * sizeof(Fe)));
    SCCHK(T.get(2 * K * sizeof(Fe)));
    hipLaunchKernelGGL(pt_rev_monic_kernel, dim3(pt_blocks(K)), dim3(256), 0, st, (const Fe*)(t->zc + (uint64_t)L * K), G.fe(), K);
    const Fe one{1, 0};
    HIPCHK(hipMemcpyAsync(h.p, &one, sizeof(Fe), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                    // `one` is a stack temporary
    for (int lm = 0; lm < L; ++lm) {                      // m = 2^lm known coefficients -> 2m
        const int logn = lm + 2;
        const uint64_t n = 1ull << logn, m = 1ull << lm;
        Fe rt = canonical_root(logn);
        NttOpts o;
        o.in_limit = m;
        SCCHK(ntt_device(h.fe(), H.fe(), logn, rt, false, o, st));
        o.in_limit = 2 * m;
        SCCHK(ntt_device(G.fe(), T.fe(), logn, rt, false, o, st));
        hipLaunchKernelGGL(pt_newton_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, H.fe(), (const Fe*)T.fe(), n, ninv_scaled(logn, 3));
        SCCHK(ntt_device(H.fe(), h.fe(), logn, root_inverse(rt, n), false, NttOpts(), st));
    }
    Fe* f = nullptr;
    HIPCHK(pool_alloc((void**)&f, 2 * K * sizeof(Fe)));
    NttOpts o;
    o.in_limit = K;
    int rc = ntt_device(h.fe(), f, L + 1, canonical_root(L + 1), false, o, st);
    if (rc == SC_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(SC_ERR_HIP, "inverse series failed");
    if (rc != SC_OK) { pool_free(f, 2 * K * sizeof(Fe)); return rc; }
    t->invg_f = f;
    return SC_OK;
}

// values of the polynomial d_coeffs[0..m), m <= K, at all K leaves (the k real points first); d_out holds K entries.
// bx, by: caller's temporaries of 2K entries each, tk: K entries.
int polytree_evaluate_all(sc_polytree* t, const Fe* d_coeffs, uint64_t m, Fe* d_out, Fe* bx, Fe* by, Fe* tk, hipStream_t st) {
    const uint64_t K = t->K;
    const int L = t->L;
    if (L == 0) {
        if (m) HIPCHK(hipMemcpyAsync(d_out, d_coeffs, sizeof(Fe), hipMemcpyDeviceToDevice, st));
        else HIPCHK(hipMemsetAsync(d_out, 0, sizeof(Fe), st));
        return SC_OK;
    }
    SCCHK(polytree_inverse_series(t, st));
    // root: c = first K coefficients of f/Z in 1/x = rev_K(f) * rev(Z)^-1 mod y^K
    hipLaunchKernelGGL(pt_rev_poly_kernel, dim3(pt_blocks(2 * K)), dim3(256), 0, st, d_coeffs, m, by, K, 2 * K);
    SCCHK(ntt_cols(by, bx, L + 1, 0, false, st));
    hipLaunchKernelGGL(pt_mul_scaled_kernel, dim3(pt_blocks(2 * K)), dim3(256), 0, st, (const Fe*)bx, (const Fe*)t->invg_f, bx, 2 * K, ninv_scaled(L + 1, 2));
    SCCHK(ntt_cols(bx, by, L + 1, 0, true, st));
    // down: cur = by[0..K) holds the series of the level-l nodes, [2^l][K >> l]
    for (int l = L; l >= 1; --l) {
        const uint64_t n = 1ull << l;
        const int logB = L - l;
        SCCHK(ntt_cols(by, tk, l, logB, false, st));
        hipLaunchKernelGGL(pt_corr_kernel, dim3(pt_blocks(2 * K)), dim3(256), 0, st, (const Fe*)tk, (const Fe*)(t->zf + (uint64_t)(l - 1) * 2 * K), bx, n, logB + 1,
                           ninv_scaled(l, 2));
        SCCHK(ntt_cols(bx, by, l, logB + 1, true, st));     // rows < n/2 = the first K entries = next level's series
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d_out, by, K * sizeof(Fe), hipMemcpyDeviceToDevice, st));
    return SC_OK;
}

// d_points: the k points again (only read when m > K, for the chunk powers x^K)
int polytree_evaluate(sc_polytree* t, const Fe* d_coeffs, uint64_t m, const Fe* d_points, Fe* d_out, hipStream_t st) {
    const uint64_t K = t->K, k = t->k;
    PoolTmp bx, by, tk, all;
    SCCHK(bx.get(2 * K * sizeof(Fe)));
    SCCHK(by.get(2 * K * sizeof(Fe)));
    SCCHK(tk.get(K * sizeof(Fe)));
    SCCHK(all.get(K * sizeof(Fe)));
    if (m <= K) {
        SCCHK(polytree_evaluate_all(t, d_coeffs, m, all.fe(), bx.fe(), by.fe(), tk.fe(), st));
        HIPCHK(hipMemcpyAsync(d_out, all.p, k * sizeof(Fe), hipMemcpyDeviceToDevice, st));
    } else {
        if (!d_points) return fail(SC_ERR_BAD_ARG, "polynomial longer than the padded domain needs the points for chunked evaluation");
        PoolTmp y;
        SCCHK(y.get(k * sizeof(Fe)));
        hipLaunchKernelGGL(pt_pow2_kernel, dim3(pt_blocks(k)), dim3(256), 0, st, d_points, k, t->L, y.fe());
        const uint64_t chunks = (m + K - 1) / K;
        for (uint64_t j = chunks; j-- > 0;) {
            const uint64_t len = (j == chunks - 1) ? m - j * K : K;
            SCCHK(polytree_evaluate_all(t, d_coeffs + j * K, len, all.fe(), bx.fe(), by.fe(), tk.fe(), st));
            if (j == chunks - 1) HIPCHK(hipMemcpyAsync(d_out, all.p, k * sizeof(Fe), hipMemcpyDeviceToDevice, st));
            else hipLaunchKernelGGL(pt_horner_kernel, dim3(pt_blocks(k)), dim3(256), 0, st, d_out, (const Fe*)y.fe(), (const Fe*)all.fe(), k);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));
    return SC_OK;
}

int polytree_interpolate(sc_polytree* t, const Fe* d_values, Fe* d_out, hipStream_t st) {
    const uint64_t K = t->K, k = t->k, pad = K - k;
    const int L = t->L;
    if (L == 0) {
        HIPCHK(hipMemcpyAsync(d_out, d_values, sizeof(Fe), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return SC_OK;
    }
    PoolTmp bx, by, tk, p;
    SCCHK(bx.get(2 * K * sizeof(Fe)));
    SCCHK(by.get(2 * K * sizeof(Fe)));
    SCCHK(tk.get(K * sizeof(Fe)));
    SCCHK(p.get(K * sizeof(Fe)));
    const Fe* top = t->zc + (uint64_t)L * K;
    // weights w_i = v_i / Z_real'(d_i); padding leaves get weight 0
    hipLaunchKernelGGL(pt_deriv_kernel, dim3(pt_blocks(K)), dim3(256), 0, st, top, K, pad, k, p.fe());
    SCCHK(polytree_evaluate_all(t, p.fe(), k, tk.fe(), bx.fe(), by.fe(), p.fe(), st));     // p doubles as the K-entry temporary: its content is consumed first
    HIPCHK(hipMemsetAsync(p.p, 0, K * sizeof(Fe), st));
    SCCHK(pointwise_div_device(d_values, tk.fe(), p.fe(), k, st));
    // up: P = P_L * Z_R + P_R * Z_L
    Fe* cur = p.fe();
    Fe* nxt = tk.fe();
    for (int l = 0; l < L; ++l) {
        const uint64_t B = K >> l;
        hipLaunchKernelGGL(pt_expand_kernel, dim3(pt_blocks(2 * K)), dim3(256), 0, st, (const Fe*)cur, bx.fe(), K, B, (uint64_t)0);
        SCCHK(ntt_cols(bx.fe(), by.fe(), l + 1, L - l, false, st));
        hipLaunchKernelGGL(pt_comb_kernel, dim3(pt_blocks(K)), dim3(256), 0, st, (const Fe*)by.fe(), (const Fe*)(t->zf + (uint64_t)l * 2 * K), bx.fe(), K, ninv_scaled(l + 1, 2));
        SCCHK(ntt_cols(bx.fe(), nxt, l + 1, L - l - 1, true, st));
        Fe* s = cur; cur = nxt; nxt = s;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d_out, cur + pad, k * sizeof(Fe), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return SC_OK;
}

// ---- many columns per call (the *_cols kernels of polytree.cuh): a set of C' = 2^logC columns, column index innermost ----------
// Columns per set: 2K * C' elements per temporary within the launch budget (sc_set_tuning("tree_cols_launch_log"), 2^26 by
// default), and no more lanes than the power of two that holds all columns
int polytree_set_log(const sc_polytree* t, uint64_t cols) {
    const int budget = g.tree_cols_launch_log - (t->L + 1);
    int logC = 0;
    while (logC < budget && (1ull << logC) < cols) ++logC;
    return logC;
}
// lanes of a set that holds `nc` real columns: the power of two >= nc (the padding lanes compute on zeros and are never stored)
inline int lanes_log(uint64_t nc) { return ilog2(nc); }

// polytree_evaluate_all for nc <= 2^logC columns at pitch ld_in: the values at all K leaves are left INTERLEAVED in by[0 .. K << logC).
// bx, by: 2K << logC entries each, tk: K << logC.
int polytree_evaluate_all_cols(sc_polytree* t, const Fe* d_coeffs, uint64_t m, uint64_t ld_in, uint64_t nc, int logC, Fe* bx, Fe* by, Fe* tk, hipStream_t st) {
    const uint64_t K = t->K;
    const int L = t->L;
    if (L == 0) {
        hipLaunchKernelGGL(pt_rev_poly_cols_kernel, dim3(pt_blocks(K << logC)), dim3(256), 0, st, d_coeffs, m, ld_in, nc, by, K, logC, K << logC);
        HIPCHK(hipGetLastError());
        return SC_OK;
    }
    const uint64_t wide = (2 * K) << logC;
    hipLaunchKernelGGL(pt_rev_poly_cols_kernel, dim3(pt_blocks(wide)), dim3(256), 0, st, d_coeffs, m, ld_in, nc, by, K, logC, wide);
    SCCHK(ntt_cols(by, bx, L + 1, logC, false, st));
    hipLaunchKernelGGL(pt_mul_tab_cols_kernel, dim3(pt_blocks(wide)), dim3(256), 0, st, (const Fe*)bx, (const Fe*)t->invg_f, bx, wide, logC, ninv_scaled(L + 1, 2));
    SCCHK(ntt_cols(bx, by, L + 1, logC, true, st));
    for (int l = L; l >= 1; --l) {
        const uint64_t n = 1ull << l;
        const int logB = L - l;
        SCCHK(ntt_cols(by, tk, l, logB + logC, false, st));
        hipLaunchKernelGGL(pt_corr_cols_kernel, dim3(pt_blocks(wide)), dim3(256), 0, st, (const Fe*)tk, (const Fe*)(t->zf + (uint64_t)(l - 1) * 2 * K), bx, n, logB + 1, logC,
                           ninv_scaled(l, 2));
        SCCHK(ntt_cols(bx, by, l, logB + 1 + logC, true, st));     // rows < n/2 = the first K << logC entries = next level's series
    }
    HIPCHK(hipGetLastError());
    return SC_OK;
}

// polytree_evaluate for `cols` columns: column c's m coefficients at d_coeffs + c * ld_in, its k values to d_out + c * ld_out.  Every
// step is issued once per set of columns; nothing waits (but the first use of a tree builds its inverse series, which does).
int polytree_evaluate_columns(sc_polytree* t, const Fe* d_coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, const Fe* d_points, Fe* d_out, uint64_t ld_out,
                              hipStream_t st) {
    const uint64_t K = t->K, k = t->k;
    SCCHK(polytree_inverse_series(t, st));
    const uint64_t per = 1ull << polytree_set_log(t, cols);
    const int logP = ilog2(per);
    PoolTmpAsync bx, by, tk, y;
    SCCHK(bx.get(((2 * K) << logP) * sizeof(Fe)));
    SCCHK(by.get(((2 * K) << logP) * sizeof(Fe)));
    SCCHK(tk.get((K << logP) * sizeof(Fe)));
    if (m > K) {
        SCCHK(y.get(k * sizeof(Fe)));
        hipLaunchKernelGGL(pt_pow2_kernel, dim3(pt_blocks(k)), dim3(256), 0, st, d_points, k, t->L, y.fe());
    }
    const uint64_t chunks = m > K ? (m + K - 1) / K : 1;
    for (uint64_t done = 0; done < cols; done += per) {
        const uint64_t nc = cols - done < per ? cols - done : per;
        const int logC = lanes_log(nc);
        const Fe* src = d_coeffs + done * ld_in;
        Fe* dst = d_out + done * ld_out;
        for (uint64_t j = chunks; j-- > 0;) {
            const uint64_t len = (j == chunks - 1) ? m - j * K : K;
            SCCHK(polytree_evaluate_all_cols(t, src + j * K, len, ld_in, nc, logC, bx.fe(), by.fe(), tk.fe(), st));
            if (j == chunks - 1) hipLaunchKernelGGL(pt_store_cols_kernel, dim3(pt_blocks(k * nc)), dim3(256), 0, st, (const Fe*)by.fe(), logC, (uint64_t)0, k, k * nc, dst, ld_out);
            else hipLaunchKernelGGL(pt_horner_cols_kernel, dim3(pt_blocks(k * nc)), dim3(256), 0, st, dst, ld_out, (const Fe*)y.fe(), (const Fe*)by.fe(), logC, k, k * nc);
        }
        HIPCHK(hipGetLastError());
    }
    return SC_OK;
}

// 1 / Z'(d_i) for the k real points, once per tree: the derivative of the zerofier at all leaves and one division of ones.  A zero
// derivative (a repeated point) fails with what sc_polytree_interpolate_dev reports, and nothing is kept.
int polytree_weights(sc_polytree* t, hipStream_t st) {
    if (t->winv_m || t->L == 0) return SC_OK;
    const uint64_t K = t->K, k = t->k;
    PoolTmpAsync bx, by, tk, p, ones;
    SCCHK(bx.get(2 * K * sizeof(Fe)));
    SCCHK(by.get(2 * K * sizeof(Fe)));
    SCCHK(tk.get(K * sizeof(Fe)));
    SCCHK(p.get(K * sizeof(Fe)));
    SCCHK(ones.get(k * sizeof(Fe)));
    hipLaunchKernelGGL(pt_deriv_kernel, dim3(pt_blocks(K)), dim3(256), 0, st, (const Fe*)(t->zc + (uint64_t)t->L * K), K, K - k, k, p.fe());
    SCCHK(polytree_evaluate_all(t, p.fe(), k, tk.fe(), bx.fe(), by.fe(), p.fe(), st));
    hipLaunchKernelGGL(pt_fill_kernel, dim3(pt_blocks(k)), dim3(256), 0, st, ones.fe(), k, fe_mont_one());
    HIPCHK(hipGetLastError());
    Fe* w = nullptr;
    HIPCHK(pool_alloc((void**)&w, k * sizeof(Fe)));
    int rc = pointwise_div_device(ones.fe(), tk.fe(), w, k, st);     // R / Z'(d_i): the Montgomery form of the inverse; waits for the verdict
    if (rc != SC_OK) { release_after_streams(w, k * sizeof(Fe)); return rc; }
    t->winv_m = w;
    return SC_OK;
}

// inv0(Z'(d_i)) for the k real points, once per tree (pt_inv0_kernel): the derivative of the zerofier at all leaves and one inversion
// per point that keeps a zero.  Only enqueues (but the tree's inverse series is built on first use, which waits).  A table winv_m
// that exists was built without a zero derivative and is the same table: it is shared.  The table is published as soon as its kernel
// is enqueued (polytree_weights waits, for its verdict): valid in the order of `st`, which is the trees' one-stream rule.  Nothing here touches winv_m, so the
// entries that answer a repeated point with SC_ERR_DIV_ZERO go on doing so.
int polytree_weights_inv0(sc_polytree* t, hipStream_t st) {
    if (t->winv0_m || t->L == 0) return SC_OK;
    if (t->winv_m) { t->winv0_m = t->winv_m; return SC_OK; }
    const uint64_t K = t->K, k = t->k;
    PoolTmpAsync bx, by, tk, p;
    SCCHK(bx.get(2 * K * sizeof(Fe)));
    SCCHK(by.get(2 * K * sizeof(Fe)));
    SCCHK(tk.get(K * sizeof(Fe)));
    SCCHK(p.get(K * sizeof(Fe)));
    hipLaunchKernelGGL(pt_deriv_kernel, dim3(pt_blocks(K)), dim3(256), 0, st, (const Fe*)(t->zc + (uint64_t)t->L * K), K, K - k, k, p.fe());
    SCCHK(polytree_evaluate_all(t, p.fe(), k, tk.fe(), bx.fe(), by.fe(), p.fe(), st));
    Fe* w = nullptr;
    HIPCHK(pool_alloc((void**)&w, k * sizeof(Fe)));
    hipLaunchKernelGGL(pt_inv0_kernel, dim3(pt_blocks(k)), dim3(256), 0, st, (const Fe*)tk.fe(), w, k);
    if (hipGetLastError() != hipSuccess) { release_after_streams(w, k * sizeof(Fe)); return fail(SC_ERR_HIP, "weight table launch failed"); }
    t->winv0_m = w;
    return SC_OK;
}

// polytree_interpolate for `cols` columns: column c's k values at d_values + c * ld_in, its k coefficients to d_out + c * ld_out.
// lagrange: the weights inv0(Z'(d_i)) instead of 1 / Z'(d_i) -- Polynomial.interpolate_domain's result for ANY points (a repeated
// point drops its terms, code/univariate.py:107-121) where the other table fails the call; everything behind the weights is the same.
int polytree_interpolate_columns(sc_polytree* t, const Fe* d_values, uint64_t ld_in, uint64_t cols, Fe* d_out, uint64_t ld_out, bool lagrange, hipStream_t st) {
    const uint64_t K = t->K, k = t->k, pad = K - k;
    const int L = t->L;
    SCCHK(lagrange ? polytree_weights_inv0(t, st) : polytree_weights(t, st));
    const Fe* winv = lagrange ? t->winv0_m : t->winv_m;
    const uint64_t per = 1ull << polytree_set_log(t, cols);
    const int logP = ilog2(per);
    PoolTmpAsync bx, by, tk, p;
    SCCHK(bx.get(((2 * K) << logP) * sizeof(Fe)));
    SCCHK(by.get(((2 * K) << logP) * sizeof(Fe)));
    SCCHK(tk.get((K << logP) * sizeof(Fe)));
    SCCHK(p.get((K << logP) * sizeof(Fe)));
    for (uint64_t done = 0; done < cols; done += per) {
        const uint64_t nc = cols - done < per ? cols - done : per;
        const int logC = lanes_log(nc);
        const uint64_t half = K << logC;
        const Fe* src = d_values + done * ld_in;
        Fe* cur = p.fe();
        Fe* nxt = tk.fe();
        if (L == 0) hipLaunchKernelGGL(pt_rev_poly_cols_kernel, dim3(pt_blocks(half)), dim3(256), 0, st, src, (uint64_t)1, ld_in, nc, cur, K, logC, half);   // one point: the value itself
        else hipLaunchKernelGGL(pt_weights_cols_kernel, dim3(pt_blocks(half)), dim3(256), 0, st, src, ld_in, nc, winv, k, cur, logC, half);
        // up: P = P_L * Z_R + P_R * Z_L
        for (int l = 0; l < L; ++l) {
            hipLaunchKernelGGL(pt_expand_cols_kernel, dim3(pt_blocks(2 * half)), dim3(256), 0, st, (const Fe*)cur, bx.fe(), half);
            SCCHK(ntt_cols(bx.fe(), by.fe(), l + 1, L - l + logC, false, st));
            hipLaunchKernelGGL(pt_comb_cols_kernel, dim3(pt_blocks(half)), dim3(256), 0, st, (const Fe*)by.fe(), (const Fe*)(t->zf + (uint64_t)l * 2 * K), bx.fe(), half, logC,
                               ninv_scaled(l + 1, 2));
            SCCHK(ntt_cols(bx.fe(), nxt, l + 1, L - l - 1 + logC, true, st));
            Fe* s = cur; cur = nxt; nxt = s;
        }
        hipLaunchKernelGGL(pt_store_cols_kernel, dim3(pt_blocks(k * nc)), dim3(256), 0, st, (const Fe*)cur, logC, pad, k, k * nc, d_out + done * ld_out, ld_out);
        HIPCHK(hipGetLastError());
    }
    return SC_OK;
}

}  // namespace

// ============================================================================ geometric progressions (geoseq.cuh)

struct sc_geodomain {
    uint64_t n, M;
    int logM;
    Fe c, q, c_inv;        // first point, ratio, 1 / first point (canonical)
    bool unit;             // c == 1: no scaling by powers of c anywhere
    Fe* tinv_m;            // n:  q^-(j(j-1)/2)
    Fe* wden_m;            // n:  1 / (Z'(q^i) t_i)
    Fe* Bf;                // M:  transform of t_0 .. t_(M-1)
    Fe* ZRf;               // M:  transform of the reversed zerofier's first n coefficients
    Fe* zr;                // n + 1: reversed zerofier of {q^i}, canonical
};

namespace {

// inclusive prefix products of n Montgomery forms, in place (reduce per workgroup, scan the totals, apply)
int scan_products(Fe* a, uint64_t n, hipStream_t st) {
    if (n == 0) return SC_OK;
    const uint64_t nb = (n + GS_BLOCK - 1) / GS_BLOCK;
    if (nb == 1) {
        hipLaunchKernelGGL(gs_apply_kernel, dim3(1), dim3(GS_T), 0, st, a, n, (const Fe*)nullptr);
        HIPCHK(hipGetLastError());
        return SC_OK;
    }
    PoolTmpAsync tot;
    SCCHK(tot.get(nb * sizeof(Fe)));
    hipLaunchKernelGGL(gs_totals_kernel, dim3((unsigned)nb), dim3(GS_T), 0, st, (const Fe*)a, n, tot.fe());
    SCCHK(scan_products(tot.fe(), nb, st));
    hipLaunchKernelGGL(gs_apply_kernel, dim3((unsigned)nb), dim3(GS_T), 0, st, a, n, (const Fe*)tot.fe());
    HIPCHK(hipGetLastError());
    return SC_OK;
}

void geodomain_release(sc_geodomain* d) {
    if (!d) return;
    if (d->tinv_m) release_after_streams(d->tinv_m, d->n * sizeof(Fe));
    if (d->wden_m) release_after_streams(d->wden_m, d->n * sizeof(Fe));
    if (d->Bf) release_after_streams(d->Bf, d->M * sizeof(Fe));
    if (d->ZRf) release_after_streams(d->ZRf, d->M * sizeof(Fe));
    if (d->zr) release_after_streams(d->zr, (d->n + 1) * sizeof(Fe));
    delete d;
}

int geodomain_create(Fe c, Fe q, uint64_t n, sc_geodomain** out, hipStream_t st) {
    if (n < 2) return fail(SC_ERR_UNSUPPORTED, "a progression of fewer than two points");
    if (fe_ge_p(c) || fe_ge_p(q) || fe_is_zero(c) || fe_is_zero(q)) return fail(SC_ERR_UNSUPPORTED, "first point and ratio must be non-zero residues");
    const int logM = ilog2(2 * n - 1);
    if (logM > 28) return fail(SC_ERR_UNSUPPORTED, "progression too long");
    const uint64_t M = 1ull << logM;
    sc_geodomain* d = new sc_geodomain{n, M, logM, c, q, Fe{0, 0}, fe_eq(c, fe_one()), nullptr, nullptr, nullptr, nullptr, nullptr};
    auto bail = [&](int rc) { geodomain_release(d); return rc; };
    auto alloc = [&](Fe** p, uint64_t count) -> int {
        hipError_t e = pool_alloc((void**)p, count * sizeof(Fe));
        return e == hipSuccess ? SC_OK : fail(SC_ERR_HIP, hipGetErrorString(e));
    };
    int rc = alloc(&d->tinv_m, n);
    if (rc == SC_OK) rc = alloc(&d->wden_m, n);
    if (rc == SC_OK) rc = alloc(&d->Bf, M);
    if (rc == SC_OK) rc = alloc(&d->ZRf, M);
    if (rc == SC_OK) rc = alloc(&d->zr, n + 1);
    if (rc != SC_OK) return bail(rc);
    const Fe q_m = to_mont(q);
    const Fe qinv = from_mont(mont_inv(q_m));
    d->c_inv = from_mont(mont_inv(to_mont(c)));
    PoolTmpAsync tt, A, rev;
    if ((rc = tt.get(M * sizeof(Fe))) != SC_OK || (rc = A.get(n * sizeof(Fe))) != SC_OK || (rc = rev.get(n * sizeof(Fe))) != SC_OK) return bail(rc);
    PowTables *pq, *pqi, *pg;
    if ((rc = get_pow(q, M, st, &pq)) != SC_OK) return bail(rc);
    if ((rc = get_pow(qinv, n, st, &pqi)) != SC_OK) return bail(rc);
    // t_j (M of them), 1 / t_j (n), A_(j+1) (n), S_(n-2-j) (n - 1): one fill and one scan each
    hipLaunchKernelGGL(geo_fill_kernel, dim3(pt_blocks(M)), dim3(256), 0, st, tt.fe(), M, 0, n, (const Fe*)pq->lo, (const Fe*)pq->hi);
    if ((rc = scan_products(tt.fe(), M, st)) != SC_OK) return bail(rc);
    hipLaunchKernelGGL(geo_fill_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, d->tinv_m, n, 0, n, (const Fe*)pqi->lo, (const Fe*)pqi->hi);
    if ((rc = scan_products(d->tinv_m, n, st)) != SC_OK) return bail(rc);
    hipLaunchKernelGGL(geo_fill_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, A.fe(), n, 1, n, (const Fe*)pq->lo, (const Fe*)pq->hi);
    if ((rc = scan_products(A.fe(), n, st)) != SC_OK) return bail(rc);
    hipLaunchKernelGGL(geo_fill_kernel, dim3(pt_blocks(n - 1)), dim3(256), 0, st, rev.fe(), n - 1, 2, n, (const Fe*)pq->lo, (const Fe*)pq->hi);
    if ((rc = scan_products(rev.fe(), n - 1, st)) != SC_OK) return bail(rc);
    // scan[j] = A_(j+1).  A_(n-1) and A_n decide: a zero A_(n-1) means q^m = 1 for some m < n, i.e. the points repeat
    Fe tail[2];
    if (hipMemcpyAsync(tail, A.fe() + (n - 2), 2 * sizeof(Fe), hipMemcpyDeviceToHost, st) != hipSuccess) return bail(fail(SC_ERR_HIP, "copy of the scan's tail failed"));
    if (hipStreamSynchronize(st) != hipSuccess) return bail(fail(SC_ERR_HIP, "progression tables failed"));
    const Fe an1_m = tail[0], an_m = tail[1];
    if (fe_is_zero(an1_m)) return bail(fail(SC_ERR_UNSUPPORTED, "the points of the progression are not distinct"));
    const Fe ia_m = mont_inv(an1_m);
    const Fe k1_m = mont_mul(ia_m, ia_m);
    const Fe k2_m = mont_mul(an_m, k1_m);
    const Fe g = from_mont(mont_pow(to_mont(qinv), n - 2));
    if ((rc = get_pow(g, n, st, &pg)) != SC_OK) return bail(rc);
    hipLaunchKernelGGL(geo_wden_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, d->wden_m, n, (const Fe*)rev.fe(), k1_m, (const Fe*)pg->lo, (const Fe*)pg->hi);
    hipLaunchKernelGGL(geo_zr_kernel, dim3(pt_blocks(n + 1)), dim3(256), 0, st, d->zr, n, (const Fe*)rev.fe(), (const Fe*)tt.fe(), k2_m);
    hipLaunchKernelGGL(geo_from_mont_kernel, dim3(pt_blocks(M)), dim3(256), 0, st, tt.fe(), M);
    if (hipGetLastError() != hipSuccess) return bail(fail(SC_ERR_HIP, "progression table launch failed"));
    const Fe rt = canonical_root(logM);
    if ((rc = ntt_device(tt.fe(), d->Bf, logM, rt, false, NttOpts(), st)) != SC_OK) return bail(rc);
    NttOpts o;
    o.in_limit = n;
    if ((rc = ntt_device(d->zr, d->ZRf, logM, rt, false, o, st)) != SC_OK) return bail(rc);
    *out = d;
    return SC_OK;
}

const PowTables* geo_cpow(const sc_geodomain* d, Fe base, uint64_t count, hipStream_t st, int* rc) {
    if (d->unit) { *rc = SC_OK; return nullptr; }
    PowTables* pw = nullptr;
    *rc = get_pow(base, count, st, &pw);
    return pw;
}

// values at all n points of the polynomial p[0..len), len <= n; bx, by: M entries each
int geodomain_evaluate_chunk(const sc_geodomain* d, const Fe* p, uint64_t len, Fe* dst, Fe* bx, Fe* by, hipStream_t st) {
    const uint64_t n = d->n, M = d->M;
    if (len == 0) { HIPCHK(hipMemsetAsync(dst, 0, n * sizeof(Fe), st)); return SC_OK; }
    int rc;
    const PowTables* pc = geo_cpow(d, d->c, n, st, &rc);
    SCCHK(rc);
    hipLaunchKernelGGL(geo_eval_in_kernel, dim3(pt_blocks(len)), dim3(256), 0, st, p, len, pc ? (const Fe*)pc->lo : nullptr, pc ? (const Fe*)pc->hi : nullptr, (const Fe*)d->tinv_m, bx);
    const Fe rt = canonical_root(d->logM);
    NttOpts o;
    o.in_limit = len;
    SCCHK(ntt_device(bx, by, d->logM, rt, false, o, st));
    hipLaunchKernelGGL(geo_corr_kernel, dim3(pt_blocks(M)), dim3(256), 0, st, (const Fe*)by, (const Fe*)d->Bf, bx, M, ninv_scaled(d->logM, 2));
    SCCHK(ntt_device(bx, by, d->logM, root_inverse(rt, M), false, NttOpts(), st));
    hipLaunchKernelGGL(geo_mul_tab_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, (const Fe*)by, (const Fe*)d->tinv_m, dst, n);
    HIPCHK(hipGetLastError());
    return SC_OK;
}

int geodomain_evaluate(const sc_geodomain* d, const Fe* coeffs, uint64_t m, Fe* out, hipStream_t st) {
    const uint64_t n = d->n, M = d->M;
    PoolTmpAsync bx, by;
    SCCHK(bx.get(M * sizeof(Fe)));
    SCCHK(by.get(M * sizeof(Fe)));
    if (m <= n) return geodomain_evaluate_chunk(d, coeffs, m, out, bx.fe(), by.fe(), st);
    // longer polynomials: Horner over chunks of n coefficients, y_i = x_i^n = c^n (q^n)^i
    PoolTmpAsync y, vals;
    SCCHK(y.get(n * sizeof(Fe)));
    SCCHK(vals.get(n * sizeof(Fe)));
    const Fe cn_m = mont_pow(to_mont(d->c), n);
    const Fe qn = from_mont(mont_pow(to_mont(d->q), n));
    PowTables* py;
    SCCHK(get_pow(qn, n, st, &py));
    hipLaunchKernelGGL(geo_chunk_power_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, y.fe(), n, cn_m, (const Fe*)py->lo, (const Fe*)py->hi);
    const uint64_t chunks = (m + n - 1) / n;
    for (uint64_t j = chunks; j-- > 0;) {
        const uint64_t len = (j == chunks - 1) ? m - j * n : n;
        if (j == chunks - 1) { SCCHK(geodomain_evaluate_chunk(d, coeffs + j * n, len, out, bx.fe(), by.fe(), st)); continue; }
        SCCHK(geodomain_evaluate_chunk(d, coeffs + j * n, len, vals.fe(), bx.fe(), by.fe(), st));
        hipLaunchKernelGGL(pt_horner_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, out, (const Fe*)y.fe(), (const Fe*)vals.fe(), n);
    }
    HIPCHK(hipGetLastError());
    return SC_OK;
}

// is d_points[i + 1] == d_points[i] * ratio for all i < n - 1, with ratio = points[1] / points[0]?  (one small kernel, one sync)
int geodomain_detect(const Fe* d_points, uint64_t n, Fe* first, Fe* ratio, bool* is_geometric, hipStream_t st) {
    *is_geometric = false;
    if (n < 2) return SC_OK;
    Fe head[2];
    SCCHK(read_small_polled(d_points, 2 * sizeof(Fe), st, head));
    if (fe_is_zero(head[0]) || fe_is_zero(head[1]) || fe_ge_p(head[0]) || fe_ge_p(head[1])) return SC_OK;
    const Fe r_m = mont_mul(to_mont(head[1]), mont_inv(to_mont(head[0])));
    void* fl;
    SCCHK(scratch(7, 64, &fl));
    HIPCHK(hipMemsetAsync(fl, 0, 4, st));
    hipLaunchKernelGGL(geo_detect_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, d_points, n, r_m, (uint32_t*)fl);
    HIPCHK(hipGetLastError());
    uint64_t bad = 1;
    SCCHK(read_small_polled(fl, 8, st, &bad));
    if ((uint32_t)bad) return SC_OK;
    *first = head[0];
    *ratio = from_mont(r_m);
    *is_geometric = true;
    return SC_OK;
}

// the progression tables of device points if they are a progression of at least two distinct points, else *out = nullptr
int geodomain_of_points(const Fe* d_points, uint64_t n, sc_geodomain** out, hipStream_t st) {
    *out = nullptr;
    Fe first, ratio;
    bool is = false;
    SCCHK(geodomain_detect(d_points, n, &first, &ratio, &is, st));
    if (!is) return SC_OK;
    int rc = geodomain_create(first, ratio, n, out, st);
    if (rc == SC_ERR_UNSUPPORTED) { *out = nullptr; return SC_OK; }
    return rc;
}

int geodomain_interpolate(const sc_geodomain* d, const Fe* values, Fe* out, hipStream_t st) {
    const uint64_t n = d->n, M = d->M;
    PoolTmpAsync bx, by;
    SCCHK(bx.get(M * sizeof(Fe)));
    SCCHK(by.get(M * sizeof(Fe)));
    int rc;
    const PowTables* pi = geo_cpow(d, d->c_inv, n, st, &rc);
    SCCHK(rc);
    const Fe rt = canonical_root(d->logM), rti = root_inverse(rt, M);
    const Fe c_m2 = ninv_scaled(d->logM, 2);
    NttOpts o;
    o.in_limit = n;
    // s_m = sum_i (v_i / Z'(q^i)) q^(i m): weights, correlation with t, division by t_m
    hipLaunchKernelGGL(geo_mul_tab_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, values, (const Fe*)d->wden_m, bx.fe(), n);
    SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rt, false, o, st));
    hipLaunchKernelGGL(geo_corr_kernel, dim3(pt_blocks(M)), dim3(256), 0, st, (const Fe*)by.fe(), (const Fe*)d->Bf, bx.fe(), M, c_m2);
    SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rti, false, NttOpts(), st));
    hipLaunchKernelGGL(geo_mul_tab_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, (const Fe*)by.fe(), (const Fe*)d->tinv_m, bx.fe(), n);
    // rev(P) = rev(Z) * S mod y^n
    SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rt, false, o, st));
    hipLaunchKernelGGL(pt_mul_scaled_kernel, dim3(pt_blocks(M)), dim3(256), 0, st, (const Fe*)by.fe(), (const Fe*)d->ZRf, bx.fe(), M, c_m2);
    SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rti, false, NttOpts(), st));
    hipLaunchKernelGGL(geo_rev_scale_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, (const Fe*)by.fe(), n, pi ? (const Fe*)pi->lo : nullptr, pi ? (const Fe*)pi->hi : nullptr, out);
    HIPCHK(hipGetLastError());
    return SC_OK;
}

// geodomain_interpolate for `cols` columns: column c's n values at values + c * ld_in, its n coefficients at out + c * ld_out.
// The same nine steps, each issued ONCE for a set of columns: the four transforms through the column form of ntt_device
// (NttOpts::cols on [cols][M] work buffers, zero padding above n per column), the five elementwise steps over a flat grid of
// cols * len threads.  A set holds at most COLS_ELEMS_PER_LAUNCH / M and at most 65 536 columns (as sc_ntt_columns_dev splits),
// which bounds the two temporaries at 1 GiB each.  Nothing waits.
int geodomain_interpolate_columns(const sc_geodomain* d, const Fe* values, uint64_t ld_in, uint64_t cols, Fe* out, uint64_t ld_out, hipStream_t st) {
    const uint64_t n = d->n, M = d->M;
    uint64_t per = COLS_ELEMS_PER_LAUNCH / M;
    if (per < 1) per = 1;
    if (per > 65536) per = 65536;
    if (per > cols) per = cols;
    PoolTmpAsync bx, by;
    SCCHK(bx.get(per * M * sizeof(Fe)));
    SCCHK(by.get(per * M * sizeof(Fe)));
    const Fe rt = canonical_root(d->logM), rti = root_inverse(rt, M);
    const Fe c_m2 = ninv_scaled(d->logM, 2);
    for (uint64_t done = 0; done < cols; done += per) {
        const uint64_t k = cols - done < per ? cols - done : per;
        const Fe* v = values + done * ld_in;
        Fe* o = out + done * ld_out;
        int rc;
        const PowTables* pi = geo_cpow(d, d->c_inv, n, st, &rc);       // (looked up per set: a table in use is a recent lookup)
        SCCHK(rc);
        NttOpts padded, whole;
        padded.cols = whole.cols = (uint32_t)k;
        padded.in_limit = n;
        hipLaunchKernelGGL(geo_mul_tab_cols_kernel, dim3(pt_blocks(k * n)), dim3(256), 0, st, v, ld_in, (const Fe*)d->wden_m, bx.fe(), M, n, k * n);
        SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rt, false, padded, st));
        hipLaunchKernelGGL(geo_corr_cols_kernel, dim3(pt_blocks(k * M)), dim3(256), 0, st, (const Fe*)by.fe(), (const Fe*)d->Bf, bx.fe(), d->logM, k * M, c_m2);
        SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rti, false, whole, st));
        hipLaunchKernelGGL(geo_mul_tab_cols_kernel, dim3(pt_blocks(k * n)), dim3(256), 0, st, (const Fe*)by.fe(), M, (const Fe*)d->tinv_m, bx.fe(), M, n, k * n);
        SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rt, false, padded, st));
        hipLaunchKernelGGL(geo_mul_scaled_cols_kernel, dim3(pt_blocks(k * M)), dim3(256), 0, st, (const Fe*)by.fe(), (const Fe*)d->ZRf, bx.fe(), d->logM, k * M, c_m2);
        SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rti, false, whole, st));
        hipLaunchKernelGGL(geo_rev_scale_cols_kernel, dim3(pt_blocks(k * n)), dim3(256), 0, st, (const Fe*)by.fe(), M, n, k * n, pi ? (const Fe*)pi->lo : nullptr,
                           pi ? (const Fe*)pi->hi : nullptr, o, ld_out);
        HIPCHK(hipGetLastError());
    }
    return SC_OK;
}

// geodomain_evaluate for `cols` columns: column c's m coefficients at coeffs + c * ld_in, its n values at out + c * ld_out.  The five
// steps of geodomain_evaluate_chunk, each issued ONCE for a set of columns ([cols][M] work buffers, NttOpts::cols; sets as
// geodomain_interpolate_columns makes them); polynomials longer than n go through the same Horner over chunks of n coefficients,
// the chunk powers shared by the columns.  Nothing waits.
int geodomain_evaluate_columns(const sc_geodomain* d, const Fe* coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, Fe* out, uint64_t ld_out, hipStream_t st) {
    const uint64_t n = d->n, M = d->M;
    if (m == 0) {
        hipLaunchKernelGGL(geo_zero_cols_kernel, dim3(pt_blocks(cols * n)), dim3(256), 0, st, out, ld_out, n, cols * n);
        HIPCHK(hipGetLastError());
        return SC_OK;
    }
    uint64_t per = COLS_ELEMS_PER_LAUNCH / M;
    if (per < 1) per = 1;
    if (per > 65536) per = 65536;
    if (per > cols) per = cols;
    PoolTmpAsync bx, by, y, vals;
    SCCHK(bx.get(per * M * sizeof(Fe)));
    SCCHK(by.get(per * M * sizeof(Fe)));
    const Fe rt = canonical_root(d->logM), rti = root_inverse(rt, M);
    const Fe c_m2 = ninv_scaled(d->logM, 2);
    const uint64_t chunks = (m + n - 1) / n;
    if (chunks > 1) {                                                       // y_i = x_i^n = c^n (q^n)^i
        SCCHK(y.get(n * sizeof(Fe)));
        SCCHK(vals.get(per * n * sizeof(Fe)));
        const Fe cn_m = mont_pow(to_mont(d->c), n);
        const Fe qn = from_mont(mont_pow(to_mont(d->q), n));
        PowTables* py;
        SCCHK(get_pow(qn, n, st, &py));
        hipLaunchKernelGGL(geo_chunk_power_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, y.fe(), n, cn_m, (const Fe*)py->lo, (const Fe*)py->hi);
    }
    for (uint64_t done = 0; done < cols; done += per) {
        const uint64_t k = cols - done < per ? cols - done : per;
        Fe* o = out + done * ld_out;
        for (uint64_t j = chunks; j-- > 0;) {
            const uint64_t len = (j == chunks - 1) ? m - j * n : n;
            const Fe* p = coeffs + done * ld_in + j * n;
            const bool top = j == chunks - 1;
            int rc;
            const PowTables* pc = geo_cpow(d, d->c, n, st, &rc);           // (looked up per use: a table in use is a recent lookup)
            SCCHK(rc);
            NttOpts padded, whole;
            padded.cols = whole.cols = (uint32_t)k;
            padded.in_limit = len;
            hipLaunchKernelGGL(geo_eval_in_cols_kernel, dim3(pt_blocks(k * len)), dim3(256), 0, st, p, ld_in, len, k * len, pc ? (const Fe*)pc->lo : nullptr,
                               pc ? (const Fe*)pc->hi : nullptr, (const Fe*)d->tinv_m, bx.fe(), M);
            SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rt, false, padded, st));
            hipLaunchKernelGGL(geo_corr_cols_kernel, dim3(pt_blocks(k * M)), dim3(256), 0, st, (const Fe*)by.fe(), (const Fe*)d->Bf, bx.fe(), d->logM, k * M, c_m2);
            SCCHK(ntt_device(bx.fe(), by.fe(), d->logM, rti, false, whole, st));
            hipLaunchKernelGGL(geo_mul_tab_cols_kernel, dim3(pt_blocks(k * n)), dim3(256), 0, st, (const Fe*)by.fe(), M, (const Fe*)d->tinv_m, top ? o : vals.fe(), top ? ld_out : n,
                               n, k * n);
            if (!top) hipLaunchKernelGGL(geo_horner_cols_kernel, dim3(pt_blocks(k * n)), dim3(256), 0, st, o, ld_out, (const Fe*)y.fe(), (const Fe*)vals.fe(), n, n, k * n);
        }
        HIPCHK(hipGetLastError());
    }
    return SC_OK;
}

}  // namespace

// ============================================================================ division with remainder (polydiv.cuh)

namespace {

// a of na, b of nb coefficients: m quotient and nr remainder coefficients, and the transforms of the three steps
struct PolyDivShape {
    uint64_t na, nb, m, nr;
    uint64_t g;            // coefficients of rev(b) that matter: min(nb, m)
    int logP;              // Newton runs to P = 2^logP >= m coefficients (its largest transform: 2P)
    int log2, log3;        // rev(a) h at n2 = 2^log2 >= 2m - 1;  q b mod (x^n3 - 1) at n3 = 2^log3 >= nb   (both at least 2)
};

inline bool pd_overlap(const void* x, uint64_t nx, const void* y, uint64_t ny) {
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + nx * sizeof(Fe), y0 = (uintptr_t)y, y1 = y0 + ny * sizeof(Fe);
    return x && y && nx && ny && x0 < y1 && y0 < x1;
}

// everything sc_poly_divmod* refuses before anything is enqueued (the leading coefficient is looked at by polydiv_columns)
int polydiv_args(const void* d_a, uint64_t na, uint64_t ld_a, uint64_t cols, const void* d_b, uint64_t nb, const void* d_q, uint64_t ld_q, const void* d_r, uint64_t ld_r,
                 PolyDivShape* out) {
    if (!d_a || !d_b) return fail(SC_ERR_BAD_ARG, "null argument");
    if (!d_q && !d_r) return fail(SC_ERR_BAD_ARG, "neither quotient nor remainder asked for");
    if (nb == 0) return fail(SC_ERR_BAD_ARG, "empty divisor");
    if (na < nb) return fail(SC_ERR_BAD_ARG, "numerator shorter than the divisor");
    PolyDivShape s;
    s.na = na; s.nb = nb; s.m = na - nb + 1; s.nr = nb - 1;
    s.g = nb < s.m ? nb : s.m;
    if (na > (1ull << 31)) return fail(SC_ERR_BAD_ARG, "operand longer than the transforms take");
    s.logP = ilog2(s.m);
    s.log2 = std::max(1, ilog2(2 * s.m - 1));
    s.log3 = std::max(1, ilog2(nb));
    if (s.logP + 1 > 32 || s.log2 > 32 || s.log3 > 32) return fail(SC_ERR_BAD_ARG, "operand longer than the transforms take");
    if (ld_a < na || (d_q && ld_q < s.m) || (d_r && ld_r < s.nr)) return fail(SC_ERR_BAD_ARG, "a column stride below the column length");
    if (cols) {
        const uint64_t ea = (cols - 1) * ld_a + na, eq = (cols - 1) * ld_q + s.m, er = (cols - 1) * ld_r + s.nr;
        if (pd_overlap(d_q, eq, d_a, ea) || pd_overlap(d_q, eq, d_b, nb) || pd_overlap(d_r, er, d_a, ea) || pd_overlap(d_r, er, d_b, nb) || pd_overlap(d_q, eq, d_r, er))
            return fail(SC_ERR_BAD_ARG, "the outputs may not overlap the operands or each other");
    }
    *out = s;
    return SC_OK;
}

// h = rev(b)^-1 mod y^m in hbuf (2P entries, P >= m of them valid; one entry for a constant divisor): b[nb-1]^-1, then logP
// Newton steps, step lm at transform size 4 * 2^lm like polytree_inverse_series.  G, H, T: min(nb, m) and 2P and 2P entries.
int polydiv_inverse_series(const Fe* d_b, const PolyDivShape& s, Fe lead_inv, Fe* G, Fe* hbuf, Fe* H, Fe* T, hipStream_t st) {
    hipLaunchKernelGGL(pt_fill_kernel, dim3(1), dim3(256), 0, st, hbuf, (uint64_t)1, lead_inv);
    if (s.nb == 1) return SC_OK;                          // a constant: its inverse is the whole series
    if (s.logP) hipLaunchKernelGGL(pd_rev_kernel, dim3(pt_blocks(s.g)), dim3(256), 0, st, d_b, (uint64_t)0, s.nb - 1, s.g, G, (uint64_t)0);
    for (int lm = 0; lm < s.logP; ++lm) {                 // 2^lm known coefficients -> 2^(lm+1)
        const int logn = lm + 2;
        const uint64_t n = 1ull << logn, have = 1ull << lm;
        const Fe rt = canonical_root(logn);
        NttOpts o;
        o.in_limit = have;
        SCCHK(ntt_device(hbuf, H, logn, rt, false, o, st));
        o.in_limit = 2 * have < s.g ? 2 * have : s.g;
        SCCHK(ntt_device(G, T, logn, rt, false, o, st));
        hipLaunchKernelGGL(pt_newton_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, H, (const Fe*)T, n, ninv_scaled(logn, 3));
        SCCHK(ntt_device(H, hbuf, logn, root_inverse(rt, n), false, NttOpts(), st));
    }
    HIPCHK(hipGetLastError());
    return SC_OK;
}

// the three steps for `cols` columns and ONE divisor: the series and the two tables once, every transform and every kernel once
// per set of columns (div_cols_launch_log values per temporary, at most 65 535 columns: grid.y).  Temporaries are the call's own.
int polydiv_columns(const Fe* d_a, uint64_t ld_a, uint64_t cols, const Fe* d_b, Fe* d_q, uint64_t ld_q, Fe* d_r, uint64_t ld_r, const PolyDivShape& s, hipStream_t st) {
    Fe lead;
    SCCHK(read_small_polled(d_b + (s.nb - 1), sizeof(Fe), st, &lead));
    if (fe_is_zero(lead)) return fail(SC_ERR_DIV_ZERO, "divide by zero");
    if (fe_ge_p(lead)) return fail(SC_ERR_BAD_ARG, "leading coefficient is not a canonical residue");
    const Fe lead_inv = from_mont(mont_inv(to_mont(lead)));
    const bool with_r = d_r && s.nr;
    if (!with_r && !d_q) return SC_OK;                    // the remainder of a division by a constant: no coefficients
    const uint64_t n2 = 1ull << s.log2, n3 = 1ull << s.log3, P = 1ull << s.logP, wide = with_r && n3 > n2 ? n3 : n2;
    uint64_t per = (1ull << g.div_cols_launch_log) / wide;
    if (per < 1) per = 1;
    if (per > 65535) per = 65535;
    if (per > cols) per = cols;
    PoolTmpAsync G, hbuf, H, T, Hf, Bf, X, Y;
    SCCHK(G.get(s.g * sizeof(Fe)));
    SCCHK(hbuf.get(2 * P * sizeof(Fe)));
    SCCHK(H.get(2 * P * sizeof(Fe)));
    SCCHK(T.get(2 * P * sizeof(Fe)));
    SCCHK(Hf.get(n2 * sizeof(Fe)));
    if (with_r) SCCHK(Bf.get(n3 * sizeof(Fe)));
    SCCHK(X.get(per * wide * sizeof(Fe)));
    SCCHK(Y.get(per * wide * sizeof(Fe)));
    SCCHK(polydiv_inverse_series(d_b, s, lead_inv, G.fe(), hbuf.fe(), H.fe(), T.fe(), st));
    const Fe rt2 = canonical_root(s.log2), rt3 = canonical_root(s.log3);
    NttOpts o;
    o.in_limit = s.nb == 1 ? 1 : s.m;
    SCCHK(ntt_device(hbuf.fe(), Hf.fe(), s.log2, rt2, false, o, st));
    if (with_r) {
        o.in_limit = s.nb;
        SCCHK(ntt_device(d_b, Bf.fe(), s.log3, rt3, false, o, st));
    }
    for (uint64_t done = 0; done < cols; done += per) {
        const unsigned k = (unsigned)(cols - done < per ? cols - done : per);
        const Fe* a = d_a + done * ld_a;
        Fe* q = d_q ? d_q + done * ld_q : nullptr;
        // rev(q) = rev(a)[0..m) h mod y^m: columns of X at pitch n2
        hipLaunchKernelGGL(pd_rev_kernel, dim3(pt_blocks(s.m), k), dim3(256), 0, st, a, ld_a, s.na - 1, s.m, X.fe(), n2);
        NttOpts oc;
        oc.cols = k;
        oc.in_limit = s.m;
        SCCHK(ntt_device(X.fe(), Y.fe(), s.log2, rt2, false, oc, st));
        hipLaunchKernelGGL(pd_mul_tab_kernel, dim3(pt_blocks(n2), k), dim3(256), 0, st, Y.fe(), n2, (const Fe*)Hf.fe(), n2, ninv_scaled(s.log2, 2));
        oc.in_limit = ~0ull;
        SCCHK(ntt_device(Y.fe(), X.fe(), s.log2, root_inverse(rt2, n2), false, oc, st));
        if (!with_r) {
            hipLaunchKernelGGL(pd_rev_kernel, dim3(pt_blocks(s.m), k), dim3(256), 0, st, (const Fe*)X.fe(), n2, s.m - 1, s.m, q, ld_q);
            HIPCHK(hipGetLastError());
            continue;
        }
        // r = a - q b mod (x^n3 - 1): q folded into Y at pitch n3 (and stored), the product back in Y
        const uint64_t nf = s.m < n3 ? s.m : n3;
        hipLaunchKernelGGL(pd_fold_rev_kernel, dim3(pt_blocks(nf), k), dim3(256), 0, st, (const Fe*)X.fe(), n2, s.m, n3, Y.fe(), n3, q, ld_q);
        oc.in_limit = nf;
        SCCHK(ntt_device(Y.fe(), X.fe(), s.log3, rt3, false, oc, st));
        hipLaunchKernelGGL(pd_mul_tab_kernel, dim3(pt_blocks(n3), k), dim3(256), 0, st, X.fe(), n3, (const Fe*)Bf.fe(), n3, ninv_scaled(s.log3, 2));
        oc.in_limit = ~0ull;
        SCCHK(ntt_device(X.fe(), Y.fe(), s.log3, root_inverse(rt3, n3), false, oc, st));
        hipLaunchKernelGGL(pd_remainder_kernel, dim3(pt_blocks(s.nr), k), dim3(256), 0, st, a, ld_a, s.na, (const Fe*)Y.fe(), n3, n3, d_r + done * ld_r, ld_r, s.nr);
        HIPCHK(hipGetLastError());
    }
    return SC_OK;
}

}  // namespace

// ============================================================================ products, powers, products of many (polymul.cuh)

namespace {

// the largest result the transforms take: 2^32 coefficients, as for the division
constexpr uint64_t PM_MAX_LEN = 1ull << 32;

// transform size of a result of `len` coefficients: the smallest power of two that holds it, at least 2
inline int pm_log(uint64_t len) { return std::max(1, ilog2(len)); }

// extent in elements of `rows` rows of n elements at pitch ld; false: it does not fit 64 bits of bytes
inline bool pm_extent(uint64_t rows, uint64_t ld, uint64_t n, uint64_t* out) {
    const unsigned __int128 e = (unsigned __int128)(rows - 1) * ld + n;
    if (e > (~0ull) / sizeof(Fe)) return false;
    *out = (uint64_t)e;
    return true;
}

// columns of one set: div_cols_launch_log values per temporary, at most 65 535 (grid.y), at least `least`
inline uint64_t pm_per_set(uint64_t n, uint64_t least) {
    uint64_t per = (1ull << g.div_cols_launch_log) / n;
    if (per > 65535) per = 65535;
    return per < least ? least : per;
}

// everything sc_poly_mul_dev / sc_poly_mul_columns_dev refuse before anything is enqueued
int polymul_args(const void* d_a, uint64_t na, uint64_t ld_a, uint64_t cols, const void* d_b, uint64_t nb, uint64_t ld_b, const void* d_out, uint64_t ld_out, uint64_t* n_out) {
    if (!d_a || !d_b || !d_out) return fail(SC_ERR_BAD_ARG, "null argument");
    if (na == 0 || nb == 0) return fail(SC_ERR_BAD_ARG, "empty operand");
    if (na > PM_MAX_LEN || nb > PM_MAX_LEN || na + nb - 1 > PM_MAX_LEN) return fail(SC_ERR_BAD_ARG, "result longer than the transforms take");
    const uint64_t len = na + nb - 1;
    if (ld_a < na || (ld_b && ld_b < nb) || ld_out < len) return fail(SC_ERR_BAD_ARG, "a column stride below the column length");
    if (cols) {
        uint64_t ea, eb, eo;
        if (!pm_extent(cols, ld_a, na, &ea) || !pm_extent(ld_b ? cols : 1, ld_b, nb, &eb) || !pm_extent(cols, ld_out, len, &eo))
            return fail(SC_ERR_BAD_ARG, "matrix larger than the address space");
        if (pd_overlap(d_out, eo, d_a, ea) || pd_overlap(d_out, eo, d_b, eb)) return fail(SC_ERR_BAD_ARG, "the output may not overlap an operand");
    }
    *n_out = len;
    return SC_OK;
}

// out[c] = a[c] * b[c] (ld_b == 0: a[c] * b) for `cols` columns: the shared multiplicand's transform once, every other transform
// and every kernel once per set of columns.  square: b IS a (one column); it is transformed once.  Temporaries are the call's own.
int polymul_columns(const Fe* d_a, uint64_t na, uint64_t ld_a, uint64_t cols, const Fe* d_b, uint64_t nb, uint64_t ld_b, Fe* d_out, uint64_t ld_out, bool square,
                    hipStream_t st) {
    const uint64_t len = na + nb - 1;
    const int logn = pm_log(len);
    const uint64_t n = 1ull << logn;
    uint64_t per = pm_per_set(n, 1);
    if (per > cols) per = cols;
    const bool shared = ld_b == 0 && !square;
    PoolTmpAsync Bf, X, Y;
    if (shared) SCCHK(Bf.get(n * sizeof(Fe)));
    SCCHK(X.get(per * n * sizeof(Fe)));
    SCCHK(Y.get(per * n * sizeof(Fe)));
    const Fe rt = canonical_root(logn), rti = root_inverse(rt, n), c_m2 = ninv_scaled(logn, 2);
    if (shared) {
        NttOpts o;
        o.in_limit = nb;
        SCCHK(ntt_device(d_b, Bf.fe(), logn, rt, false, o, st));
    }
    for (uint64_t done = 0; done < cols; done += per) {
        const unsigned k = (unsigned)(cols - done < per ? cols - done : per);
        NttOpts oc;
        oc.cols = k;
        oc.in_limit = na;
        oc.col_stride_in = ld_a;
        SCCHK(ntt_device(d_a + done * ld_a, X.fe(), logn, rt, false, oc, st));
        const Fe* bf = shared ? Bf.fe() : X.fe();
        if (!shared && !square) {
            oc.in_limit = nb;
            oc.col_stride_in = ld_b;
            SCCHK(ntt_device(d_b + done * ld_b, Y.fe(), logn, rt, false, oc, st));
            bf = Y.fe();
        }
        hipLaunchKernelGGL(pm_mul_kernel, dim3(pt_blocks(n), k), dim3(256), 0, st, (const Fe*)X.fe(), n, bf, shared ? (uint64_t)0 : n, X.fe(), n, n, c_m2);
        NttOpts oi;
        oi.cols = k;
        SCCHK(ntt_device(X.fe(), Y.fe(), logn, rti, false, oi, st));
        hipLaunchKernelGGL(pm_store_kernel, dim3(pt_blocks(len), k), dim3(256), 0, st, (const Fe*)Y.fe(), n, d_out + done * ld_out, ld_out, len);
        HIPCHK(hipGetLastError());
    }
    return SC_OK;
}

// a^e: exponent 0 is the constant 1, exponent 1 a copy, anything else one forward transform at the result's size, the pointwise
// power and one inverse transform
int polypow(const Fe* d_a, uint64_t na, uint64_t e, Fe* d_out, uint64_t len, hipStream_t st) {
    if (e == 0) {
        hipLaunchKernelGGL(pt_fill_kernel, dim3(1), dim3(256), 0, st, d_out, (uint64_t)1, Fe{1, 0});
        HIPCHK(hipGetLastError());
        return SC_OK;
    }
    if (e == 1) {
        HIPCHK(hipMemcpyAsync(d_out, d_a, na * sizeof(Fe), hipMemcpyDeviceToDevice, st));
        return SC_OK;
    }
    const int logn = pm_log(len);
    const uint64_t n = 1ull << logn;
    PoolTmpAsync X, Y;
    SCCHK(X.get(n * sizeof(Fe)));
    SCCHK(Y.get(n * sizeof(Fe)));
    const Fe rt = canonical_root(logn);
    NttOpts o;
    o.in_limit = na;
    SCCHK(ntt_device(d_a, X.fe(), logn, rt, false, o, st));
    hipLaunchKernelGGL(pm_pow_kernel, dim3(pt_blocks(n)), dim3(256), 0, st, X.fe(), n, n, e, ninv_scaled(logn, 0));
    SCCHK(ntt_device(X.fe(), Y.fe(), logn, root_inverse(rt, n), false, NttOpts(), st));
    HIPCHK(hipMemcpyAsync(d_out, Y.fe(), len * sizeof(Fe), hipMemcpyDeviceToDevice, st));
    return SC_OK;
}

// one level of the product tree: `rows` rows of `len` coefficients -> (rows + 1) / 2 rows of min(2 len - 1, total), at transform size n
struct PolyProductLevel {
    uint64_t rows, len, out_len, n;
    int logn;
};

// the product of `count` rows of n0 coefficients at pitch ld: a balanced tree whose levels live in two buffers in turn (the first
// level reads the caller's rows).  Per level and set of rows: one columns transform, the pairwise products, one inverse columns
// transform; an odd last row is carried up as it is, zero-extended to the level's length.  No product of any level is longer than
// the result, so no level needs a transform above the result's size.
int polyproduct(const Fe* d_rows, uint64_t n0, uint64_t ld, uint64_t count, Fe* d_out, uint64_t total, hipStream_t st) {
    if (count == 1) {
        HIPCHK(hipMemcpyAsync(d_out, d_rows, n0 * sizeof(Fe), hipMemcpyDeviceToDevice, st));
        return SC_OK;
    }
    std::vector<PolyProductLevel> levels;
    uint64_t level_elems = 0, set_elems = 0;
    for (uint64_t rows = count, len = n0; rows > 1; rows = (rows + 1) / 2) {
        PolyProductLevel lv;
        lv.rows = rows; lv.len = len;
        lv.out_len = 2 * len - 1 < total ? 2 * len - 1 : total;
        lv.logn = pm_log(lv.out_len);
        lv.n = 1ull << lv.logn;
        levels.push_back(lv);
        level_elems = std::max(level_elems, (rows + 1) / 2 * lv.n);
        set_elems = std::max(set_elems, std::min((pm_per_set(lv.n, 2) & ~(uint64_t)1), rows & ~(uint64_t)1) * lv.n);
        len = lv.out_len;
    }
    PoolTmpAsync L0, L1, F, G;
    SCCHK(L0.get(level_elems * sizeof(Fe)));
    if (levels.size() > 1) SCCHK(L1.get(level_elems * sizeof(Fe)));
    SCCHK(F.get(set_elems * sizeof(Fe)));
    SCCHK(G.get(set_elems / 2 * sizeof(Fe)));
    const Fe* src = d_rows;
    uint64_t pitch = ld;
    for (size_t l = 0; l < levels.size(); ++l) {
        const PolyProductLevel& lv = levels[l];
        Fe* dst = (l & 1) ? L1.fe() : L0.fe();
        const uint64_t paired = lv.rows & ~(uint64_t)1, per = std::min((pm_per_set(lv.n, 2) & ~(uint64_t)1), paired);
        const Fe rt = canonical_root(lv.logn), rti = root_inverse(rt, lv.n), c_m2 = ninv_scaled(lv.logn, 2);
        for (uint64_t done = 0; done < paired; done += per) {
            const unsigned k = (unsigned)(paired - done < per ? paired - done : per);
            NttOpts oc;
            oc.cols = k;
            oc.in_limit = lv.len;
            oc.col_stride_in = pitch;
            SCCHK(ntt_device(src + done * pitch, F.fe(), lv.logn, rt, false, oc, st));
            hipLaunchKernelGGL(pm_mul_kernel, dim3(pt_blocks(lv.n), k / 2), dim3(256), 0, st, (const Fe*)F.fe(), 2 * lv.n, (const Fe*)F.fe() + lv.n, 2 * lv.n, G.fe(), lv.n, lv.n, c_m2);
            NttOpts oi;
            oi.cols = k / 2;
            SCCHK(ntt_device(G.fe(), dst + done / 2 * lv.n, lv.logn, rti, false, oi, st));
            HIPCHK(hipGetLastError());
        }
        if (lv.rows & 1) {
            Fe* up = dst + paired / 2 * lv.n;
            HIPCHK(hipMemcpyAsync(up, src + paired * pitch, lv.len * sizeof(Fe), hipMemcpyDeviceToDevice, st));
            if (lv.out_len > lv.len) HIPCHK(hipMemsetAsync(up + lv.len, 0, (lv.out_len - lv.len) * sizeof(Fe), st));
        }
        src = dst;
        pitch = lv.n;
    }
    HIPCHK(hipMemcpyAsync(d_out, src, total * sizeof(Fe), hipMemcpyDeviceToDevice, st));
    return SC_OK;
}

}  // namespace

extern "C" {

// ---- subproduct tree: fast_zerofier / fast_evaluate / fast_interpolate
int sc_polytree_build_dev(const void* d_points, uint64_t k, sc_polytree_t** tree, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !d_points) return fail(SC_ERR_BAD_ARG, "null argument");
    return polytree_build((const Fe*)d_points, k, tree, pick_stream(stream));
}
int sc_polytree_build(const void* points, uint64_t k, sc_polytree_t** tree) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !points || !k) return fail(SC_ERR_BAD_ARG, "empty domain");
    PoolTmp dp;
    SCCHK(dp.get(k * sizeof(Fe)));
    SCCHK(upload(dp.p, points, k * sizeof(Fe), g.stream));
    return polytree_build(dp.fe(), k, tree, g.stream);       // synchronises before returning: dp may go back to the pool
}
uint64_t sc_polytree_points(const sc_polytree_t* tree) { return tree ? tree->k : 0; }
int sc_polytree_zerofier_dev(const sc_polytree_t* tree, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !d_out) return fail(SC_ERR_BAD_ARG, "null argument");
    hipStream_t st = pick_stream(stream);
    hipLaunchKernelGGL(pt_zerofier_out_kernel, dim3(pt_blocks(tree->k + 1)), dim3(256), 0, st, (const Fe*)(tree->zc + (uint64_t)tree->L * tree->K), tree->K,
                       tree->K - tree->k, tree->k, (Fe*)d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return SC_OK;
}
int sc_polytree_evaluate_dev(sc_polytree_t* tree, const void* d_coeffs, uint64_t m, const void* d_points, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !d_out || (m && !d_coeffs)) return fail(SC_ERR_BAD_ARG, "null argument");
    return polytree_evaluate(tree, (const Fe*)d_coeffs, m, (const Fe*)d_points, (Fe*)d_out, pick_stream(stream));
}
int sc_polytree_interpolate_dev(sc_polytree_t* tree, const void* d_values, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !d_out || !d_values) return fail(SC_ERR_BAD_ARG, "null argument");
    return polytree_interpolate(tree, (const Fe*)d_values, (Fe*)d_out, pick_stream(stream));
}
int sc_polytree_evaluate_columns_dev(sc_polytree_t* tree, const void* d_coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, const void* d_points, void* d_out, uint64_t ld_out,
                                     void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !d_out || (m && !d_coeffs)) return fail(SC_ERR_BAD_ARG, "null argument");
    if (m > tree->K && !d_points) return fail(SC_ERR_BAD_ARG, "polynomial longer than the padded domain needs the points for chunked evaluation");
    if (cols > 1 && (ld_in < m || ld_out < tree->k)) return fail(SC_ERR_BAD_ARG, "a column stride below the column's length");
    if (cols == 0) return SC_OK;
    return polytree_evaluate_columns(tree, (const Fe*)d_coeffs, m, ld_in, cols, (const Fe*)d_points, (Fe*)d_out, ld_out, pick_stream(stream));
}
int sc_polytree_interpolate_columns_dev(sc_polytree_t* tree, const void* d_values, uint64_t ld_in, uint64_t cols, void* d_out, uint64_t ld_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !d_out || !d_values) return fail(SC_ERR_BAD_ARG, "null argument");
    if (cols > 1 && (ld_in < tree->k || ld_out < tree->k)) return fail(SC_ERR_BAD_ARG, "a column stride below the number of points");
    if (cols == 0) return SC_OK;
    return polytree_interpolate_columns(tree, (const Fe*)d_values, ld_in, cols, (Fe*)d_out, ld_out, false, pick_stream(stream));
}
int sc_polytree_interpolate_lagrange_columns_dev(sc_polytree_t* tree, const void* d_values, uint64_t ld_in, uint64_t cols, void* d_out, uint64_t ld_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!tree || !d_out || !d_values) return fail(SC_ERR_BAD_ARG, "null argument");
    if (cols > 1 && (ld_in < tree->k || ld_out < tree->k)) return fail(SC_ERR_BAD_ARG, "a column stride below the number of points");
    if (cols == 0) return SC_OK;
    return polytree_interpolate_columns(tree, (const Fe*)d_values, ld_in, cols, (Fe*)d_out, ld_out, true, pick_stream(stream));
}
int sc_polytree_free(sc_polytree_t* tree) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!tree) return SC_OK;
    release_after_streams(tree->zc, tree->zc_bytes);
    release_after_streams(tree->zf, tree->zf_bytes);
    if (tree->invg_f) release_after_streams(tree->invg_f, 2 * tree->K * sizeof(Fe));
    if (tree->winv0_m && tree->winv0_m != tree->winv_m) release_after_streams(tree->winv0_m, tree->k * sizeof(Fe));
    if (tree->winv_m) release_after_streams(tree->winv_m, tree->k * sizeof(Fe));
    delete tree;
    return SC_OK;
}

// host-buffer forms of ntt.py:66-80, :82-100, :102-130
// host points -> their progression tables (nullptr when they are not a progression of >= 2 distinct points: the tree serves those)
static int host_points_progression(const void* points, uint64_t k, sc_geodomain** gd) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    *gd = nullptr;
    if (!points) return fail(SC_ERR_BAD_ARG, "null argument");
    if (k < 2) return SC_OK;
    PoolTmp dp;
    SCCHK(dp.get(k * sizeof(Fe)));
    SCCHK(upload(dp.p, points, k * sizeof(Fe), g.stream));
    int rc = geodomain_of_points(dp.fe(), k, gd, g.stream);
    if (hipStreamSynchronize(g.stream) != hipSuccess && rc == SC_OK) rc = fail(SC_ERR_HIP, "progression tables failed");   // dp goes back to the pool
    return rc;
}

int sc_zerofier(const void* points, uint64_t k, void* out) {
    if (k == 0) return SC_OK;
    sc_geodomain* gd = nullptr;
    SCCHK(host_points_progression(points, k, &gd));
    if (gd) {
        std::lock_guard<std::mutex> lk(g_mu);
        PoolTmp d;
        int rc = d.get((k + 1) * sizeof(Fe));
        if (rc == SC_OK) {
            const PowTables* pc = geo_cpow(gd, gd->c, k + 1, g.stream, &rc);
            if (rc == SC_OK) {
                hipLaunchKernelGGL(geo_zerofier_out_kernel, dim3(pt_blocks(k + 1)), dim3(256), 0, g.stream, (const Fe*)gd->zr, k, pc ? (const Fe*)pc->lo : nullptr,
                                   pc ? (const Fe*)pc->hi : nullptr, d.fe());
                rc = download(out, d.p, (k + 1) * sizeof(Fe), g.stream);
            }
        }
        geodomain_release(gd);
        return rc;
    }
    sc_polytree_t* t = nullptr;
    SCCHK(sc_polytree_build(points, k, &t));
    int rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        PoolTmp d;
        rc = d.get((k + 1) * sizeof(Fe));
        if (rc == SC_OK) {
            hipLaunchKernelGGL(pt_zerofier_out_kernel, dim3(pt_blocks(k + 1)), dim3(256), 0, g.stream, (const Fe*)(t->zc + (uint64_t)t->L * t->K), t->K, t->K - k, k, d.fe());
            rc = download(out, d.p, (k + 1) * sizeof(Fe), g.stream);
        }
    }
    sc_polytree_free(t);
    return rc;
}
int sc_evaluate(const void* coeffs, uint64_t m, const void* points, uint64_t k, void* out) {
    if (k == 0) return SC_OK;
    sc_geodomain* gd = nullptr;
    SCCHK(host_points_progression(points, k, &gd));
    if (gd) {
        std::lock_guard<std::mutex> lk(g_mu);
        PoolTmp dc, dv;
        int rc = dc.get((m ? m : 1) * sizeof(Fe));
        if (rc == SC_OK) rc = dv.get(k * sizeof(Fe));
        if (rc == SC_OK) rc = upload(dc.p, coeffs, m * sizeof(Fe), g.stream);
        if (rc == SC_OK) rc = geodomain_evaluate(gd, dc.fe(), m, dv.fe(), g.stream);
        if (rc == SC_OK) rc = download(out, dv.p, k * sizeof(Fe), g.stream);
        else (void)hipStreamSynchronize(g.stream);
        geodomain_release(gd);
        return rc;
    }
    sc_polytree_t* t = nullptr;
    SCCHK(sc_polytree_build(points, k, &t));
    int rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        PoolTmp dc, dp, dv;
        rc = dc.get((m ? m : 1) * sizeof(Fe));
        if (rc == SC_OK) rc = dp.get(k * sizeof(Fe));
        if (rc == SC_OK) rc = dv.get(k * sizeof(Fe));
        if (rc == SC_OK) rc = upload(dc.p, coeffs, m * sizeof(Fe), g.stream);
        if (rc == SC_OK) rc = upload(dp.p, points, k * sizeof(Fe), g.stream);
        if (rc == SC_OK) rc = polytree_evaluate(t, dc.fe(), m, dp.fe(), dv.fe(), g.stream);
        if (rc == SC_OK) rc = download(out, dv.p, k * sizeof(Fe), g.stream);
    }
    sc_polytree_free(t);
    return rc;
}
int sc_interpolate(const void* points, const void* values, uint64_t k, void* out) {
    if (k == 0) return SC_OK;
    sc_geodomain* gd = nullptr;
    SCCHK(host_points_progression(points, k, &gd));
    if (gd) {
        std::lock_guard<std::mutex> lk(g_mu);
        PoolTmp dv, dout;
        int rc = dv.get(k * sizeof(Fe));
        if (rc == SC_OK) rc = dout.get(k * sizeof(Fe));
        if (rc == SC_OK) rc = upload(dv.p, values, k * sizeof(Fe), g.stream);
        if (rc == SC_OK) rc = geodomain_interpolate(gd, dv.fe(), dout.fe(), g.stream);
        if (rc == SC_OK) rc = download(out, dout.p, k * sizeof(Fe), g.stream);
        else (void)hipStreamSynchronize(g.stream);
        geodomain_release(gd);
        return rc;
    }
    sc_polytree_t* t = nullptr;
    SCCHK(sc_polytree_build(points, k, &t));
    int rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        PoolTmp dv, dout;
        rc = dv.get(k * sizeof(Fe));
        if (rc == SC_OK) rc = dout.get(k * sizeof(Fe));
        if (rc == SC_OK) rc = upload(dv.p, values, k * sizeof(Fe), g.stream);
        if (rc == SC_OK) rc = polytree_interpolate(t, dv.fe(), dout.fe(), g.stream);
        if (rc == SC_OK) rc = download(out, dout.p, k * sizeof(Fe), g.stream);
    }
    sc_polytree_free(t);
    return rc;
}

// Polynomial.interpolate_domain (code/univariate.py:107-121) on host buffers: always the tree (a progression has distinct points, for
// which this is sc_interpolate's result anyway), one column
int sc_interpolate_lagrange(const void* points, const void* values, uint64_t k, void* out) {
    if (!points || !values || !out || !k) {
        std::lock_guard<std::mutex> lk(g_mu);
        return fail(SC_ERR_BAD_ARG, k ? "null argument" : "cannot interpolate between zero points");
    }
    sc_polytree_t* t = nullptr;
    SCCHK(sc_polytree_build(points, k, &t));
    int rc;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        PoolTmp dv, dout;
        rc = dv.get(k * sizeof(Fe));
        if (rc == SC_OK) rc = dout.get(k * sizeof(Fe));
        if (rc == SC_OK) rc = upload(dv.p, values, k * sizeof(Fe), g.stream);
        if (rc == SC_OK) rc = polytree_interpolate_columns(t, dv.fe(), k, 1, dout.fe(), k, true, g.stream);
        if (rc == SC_OK) rc = download(out, dout.p, k * sizeof(Fe), g.stream);
        else (void)hipStreamSynchronize(g.stream);
    }
    sc_polytree_free(t);
    return rc;
}

// ---- geometric progressions: fast_zerofier / fast_evaluate / fast_interpolate (ntt.py:66-130) on {first * ratio^i} ------------
int sc_geodomain_create(const uint64_t first[2], const uint64_t ratio[2], uint64_t n, sc_geodomain_t** domain, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!first || !ratio || !domain) return fail(SC_ERR_BAD_ARG, "null argument");
    return geodomain_create(fe_from(first), fe_from(ratio), n, domain, pick_stream(stream));
}
uint64_t sc_geodomain_points(const sc_geodomain_t* domain) { return domain ? domain->n : 0; }
int sc_geodomain_detect_dev(const void* d_points, uint64_t n, uint64_t first[2], uint64_t ratio[2], int* is_geometric, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!d_points || !first || !ratio || !is_geometric) return fail(SC_ERR_BAD_ARG, "null argument");
    Fe f{0, 0}, r{0, 0};
    bool is = false;
    SCCHK(geodomain_detect((const Fe*)d_points, n, &f, &r, &is, pick_stream(stream)));
    *is_geometric = is ? 1 : 0;
    if (is) { first[0] = f.lo; first[1] = f.hi; ratio[0] = r.lo; ratio[1] = r.hi; }
    return SC_OK;
}
int sc_geodomain_zerofier_dev(const sc_geodomain_t* domain, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!domain || !d_out) return fail(SC_ERR_BAD_ARG, "null argument");
    hipStream_t st = pick_stream(stream);
    int rc;
    const PowTables* pc = geo_cpow(domain, domain->c, domain->n + 1, st, &rc);
    SCCHK(rc);
    hipLaunchKernelGGL(geo_zerofier_out_kernel, dim3(pt_blocks(domain->n + 1)), dim3(256), 0, st, (const Fe*)domain->zr, domain->n, pc ? (const Fe*)pc->lo : nullptr,
                       pc ? (const Fe*)pc->hi : nullptr, (Fe*)d_out);
    HIPCHK(hipGetLastError());
    return SC_OK;
}
int sc_geodomain_evaluate_dev(const sc_geodomain_t* domain, const void* d_coeffs, uint64_t m, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!domain || !d_out || (m && !d_coeffs)) return fail(SC_ERR_BAD_ARG, "null argument");
    return geodomain_evaluate(domain, (const Fe*)d_coeffs, m, (Fe*)d_out, pick_stream(stream));
}
int sc_geodomain_interpolate_dev(const sc_geodomain_t* domain, const void* d_values, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!domain || !d_values || !d_out) return fail(SC_ERR_BAD_ARG, "null argument");
    return geodomain_interpolate(domain, (const Fe*)d_values, (Fe*)d_out, pick_stream(stream));
}
int sc_geodomain_interpolate_columns_dev(const sc_geodomain_t* domain, const void* d_values, uint64_t ld_in, uint64_t cols, void* d_out, uint64_t ld_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!domain || !d_values || !d_out) return fail(SC_ERR_BAD_ARG, "null argument");
    if (ld_in < domain->n || ld_out < domain->n) return fail(SC_ERR_BAD_ARG, "a column stride below the number of points");
    if (cols == 0) return SC_OK;
    return geodomain_interpolate_columns(domain, (const Fe*)d_values, ld_in, cols, (Fe*)d_out, ld_out, pick_stream(stream));
}
int sc_geodomain_evaluate_columns_dev(const sc_geodomain_t* domain, const void* d_coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, void* d_out, uint64_t ld_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!domain || !d_out || (m && !d_coeffs)) return fail(SC_ERR_BAD_ARG, "null argument");
    if (cols > 1 && (ld_in < m || ld_out < domain->n)) return fail(SC_ERR_BAD_ARG, "a column stride below the column's length");
    if (cols == 0) return SC_OK;
    return geodomain_evaluate_columns(domain, (const Fe*)d_coeffs, m, ld_in, cols, (Fe*)d_out, ld_out, pick_stream(stream));
}
int sc_geodomain_free(sc_geodomain_t* domain) {
    std::lock_guard<std::mutex> lk(g_mu);
    geodomain_release(domain);
    return SC_OK;
}

// ---- division with remainder (polydiv.cuh): Polynomial.divide, code/univariate.py:80-97
int sc_poly_divmod_columns_dev(const void* d_a, uint64_t na, uint64_t ld_a, uint64_t cols, const void* d_b, uint64_t nb, void* d_q, uint64_t ld_q, void* d_r, uint64_t ld_r,
                               void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    PolyDivShape s;
    SCCHK(polydiv_args(d_a, na, ld_a, cols, d_b, nb, d_q, ld_q, d_r, ld_r, &s));
    if (cols == 0) return SC_OK;
    return polydiv_columns((const Fe*)d_a, ld_a, cols, (const Fe*)d_b, (Fe*)d_q, ld_q, (Fe*)d_r, ld_r, s, pick_stream(stream));
}
int sc_poly_divmod_dev(const void* d_a, uint64_t na, const void* d_b, uint64_t nb, void* d_q, void* d_r, void* stream) {
    return sc_poly_divmod_columns_dev(d_a, na, na, 1, d_b, nb, d_q, na - nb + 1, d_r, nb ? nb - 1 : 0, stream);
}
int sc_poly_divmod(const void* a, uint64_t na, const void* b, uint64_t nb, void* q, void* r) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!a || !b || (!q && !r)) return fail(SC_ERR_BAD_ARG, "null argument");
    if (nb == 0 || na < nb) return fail(SC_ERR_BAD_ARG, nb ? "numerator shorter than the divisor" : "empty divisor");
    const uint64_t m = na - nb + 1, nr = nb - 1;
    PoolTmp ops, res;
    SCCHK(ops.get((na + nb) * sizeof(Fe)));
    SCCHK(res.get((m + nr) * sizeof(Fe)));
    Fe *da = ops.fe(), *db = da + na, *dq = res.fe(), *dr = dq + m;
    PolyDivShape s;
    SCCHK(polydiv_args(da, na, na, 1, db, nb, q ? dq : nullptr, m, r ? dr : nullptr, nr, &s));
    hipStream_t st = g.stream;
    // (a failure behind an upload waits for the stream: the host buffers are the caller's, the pool buffers go back on return)
    auto run = [&]() -> int {
        SCCHK(upload(da, a, na * sizeof(Fe), st));
        SCCHK(upload(db, b, nb * sizeof(Fe), st));
        SCCHK(polydiv_columns(da, na, 1, db, q ? dq : nullptr, m, r ? dr : nullptr, nr, s, st));
        if (q) HIPCHK(hipMemcpyAsync(q, dq, m * sizeof(Fe), hipMemcpyDeviceToHost, st));
        if (r && nr) HIPCHK(hipMemcpyAsync(r, dr, nr * sizeof(Fe), hipMemcpyDeviceToHost, st));
        return SC_OK;
    };
    const int rc = run();
    if (hipStreamSynchronize(st) != hipSuccess && rc == SC_OK) return fail(SC_ERR_HIP, "division with remainder failed");
    return rc;
}


// ---- products, powers, products of many (polymul.cuh): Polynomial.__mul__ / __xor__, code/univariate.py:48-57, :140-150
int sc_poly_mul_columns_dev(const void* d_a, uint64_t na, uint64_t ld_a, uint64_t cols, const void* d_b, uint64_t nb, uint64_t ld_b, void* d_out, uint64_t ld_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    uint64_t len;
    SCCHK(polymul_args(d_a, na, ld_a, cols, d_b, nb, ld_b, d_out, ld_out, &len));
    if (cols == 0) return SC_OK;
    return polymul_columns((const Fe*)d_a, na, ld_a, cols, (const Fe*)d_b, nb, ld_b, (Fe*)d_out, ld_out, false, pick_stream(stream));
}
int sc_poly_mul_dev(const void* d_a, uint64_t na, const void* d_b, uint64_t nb, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    uint64_t len;
    SCCHK(polymul_args(d_a, na, na, 1, d_b, nb, nb, d_out, na + nb - 1, &len));
    return polymul_columns((const Fe*)d_a, na, na, 1, (const Fe*)d_b, nb, nb, (Fe*)d_out, len, d_a == d_b && na == nb, pick_stream(stream));
}
int sc_poly_pow_dev(const void* d_a, uint64_t na, uint64_t exponent, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!d_a || !d_out) return fail(SC_ERR_BAD_ARG, "null argument");
    if (na == 0) return fail(SC_ERR_BAD_ARG, "empty operand");
    const unsigned __int128 len = (unsigned __int128)exponent * (na - 1) + 1;
    if (na > PM_MAX_LEN || len > PM_MAX_LEN) return fail(SC_ERR_BAD_ARG, "result longer than the transforms take");
    if (pd_overlap(d_out, (uint64_t)len, d_a, na)) return fail(SC_ERR_BAD_ARG, "the output may not overlap the operand");
    return polypow((const Fe*)d_a, na, exponent, (Fe*)d_out, (uint64_t)len, pick_stream(stream));
}
int sc_poly_product_dev(const void* d_rows, uint64_t n, uint64_t ld, uint64_t count, void* d_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if (!d_rows || !d_out) return fail(SC_ERR_BAD_ARG, "null argument");
    if (n == 0) return fail(SC_ERR_BAD_ARG, "empty operand");
    if (ld < n) return fail(SC_ERR_BAD_ARG, "a row stride below the row length");
    if (count == 0) return SC_OK;
    const unsigned __int128 total = (unsigned __int128)count * (n - 1) + 1;
    uint64_t extent;
    if (n > PM_MAX_LEN || total > PM_MAX_LEN) return fail(SC_ERR_BAD_ARG, "result longer than the transforms take");
    if (!pm_extent(count, ld, n, &extent)) return fail(SC_ERR_BAD_ARG, "matrix larger than the address space");
    if (pd_overlap(d_out, (uint64_t)total, d_rows, extent)) return fail(SC_ERR_BAD_ARG, "the output may not overlap the operands");
    return polyproduct((const Fe*)d_rows, n, ld, count, (Fe*)d_out, (uint64_t)total, pick_stream(stream));
}

}  // extern "C"

// polyeval.hip -- polynomials resident in HBM evaluated at a list of points directly (csrc/polyeval.cuh): sc_poly_eval_points_dev and
// its host-buffer form.
#include "core.h"
#include "polyeval.cuh"

namespace {

// What a launch set aims at before it stops cutting the coefficients finer, in quarter waves: 4 waves per SIMD of the device where the
// coefficients lie across lanes (a thread's loads are independent of its products, four chains per thread at four points), 16 where the
// points do (a lane walks its chunk alone: more waves to hide it)
constexpr uint64_t PE_UNITS_WANTED = 16384;
constexpr uint64_t PE_UNITS_PER_WG = 4 * (PE_T / PE_W);
// workgroups of one launch at most (grid.y and grid.z: 65 535 each)
constexpr uint64_t PE_MAX_WGS = 1ull << 22;
constexpr uint64_t PE_MAX = 1ull << 32;

inline bool pe_extent(uint64_t rows, uint64_t ld, uint64_t n, uint64_t* out) {
    const unsigned __int128 e = rows && n ? (unsigned __int128)(rows - 1) * ld + n : 0;
    if (e > (~0ull) / sizeof(Fe)) return false;
    *out = (uint64_t)e;
    return true;
}
inline bool pe_overlap(const void* x, uint64_t nx, const void* y, uint64_t ny) {
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + nx * sizeof(Fe), y0 = (uintptr_t)y, y1 = y0 + ny * sizeof(Fe);
    return x && y && nx && ny && x0 < y1 && y0 < x1;
}

// everything sc_poly_eval_points_dev refuses before anything is enqueued
int polyeval_args(const void* d_coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, const void* d_points, uint64_t k, const void* d_out, uint64_t ld_out) {
    if ((m && cols && !d_coeffs) || (k && !d_points) || (k && cols && !d_out)) return fail(SC_ERR_BAD_ARG, "null argument");
    if (cols > 1 && (ld_in < m || ld_out < k)) return fail(SC_ERR_BAD_ARG, "a column stride below the column's length");
    if (m > PE_MAX) return fail(SC_ERR_BAD_ARG, "more than 2^32 coefficients");
    if ((unsigned __int128)k * cols > PE_MAX) return fail(SC_ERR_BAD_ARG, "more than 2^32 results");
    uint64_t ei, eo;
    if (!pe_extent(cols, ld_in, m, &ei) || !pe_extent(cols, ld_out, k, &eo)) return fail(SC_ERR_BAD_ARG, "matrix larger than the address space");
    if (pe_overlap(d_out, eo, d_coeffs, ei) || pe_overlap(d_out, eo, d_points, k)) return fail(SC_ERR_BAD_ARG, "the output may not overlap the coefficients or the points");
    return SC_OK;
}

// grid.y x grid.z of one launch for `ny` rows and `nz` columns still to serve and grid.x = nx: at most PE_MAX_WGS workgroups
inline void pe_tile(uint64_t nx, uint64_t ny, uint64_t nz, unsigned* gy, unsigned* gz) {
    const uint64_t room = std::max<uint64_t>(1, PE_MAX_WGS / nx);
    const uint64_t y = std::min<uint64_t>({ny, 65535, room});
    *gy = (unsigned)y;
    *gz = (unsigned)std::min<uint64_t>({nz, 65535, std::max<uint64_t>(1, room / y)});
}

// Points [0, kb) go points-across-lanes, points [kb, k) coefficients-across-lanes: whole waves of 64 points are served across lanes
// from eval_points_across_min points on, and so is a last part-wave of at least that many -- a shorter rest would leave most of its
// wave idle and is served by the other form.  Only in calls of at least 2^eval_across_min_products_log products: a smaller call does
// not fill the device whichever form it takes, and then the coefficients-across-lanes form, which spreads one chunk over a
// workgroup, has the shorter critical path (a lane of the other form walks its chunk alone).
inline uint64_t polyeval_across(uint64_t m, uint64_t k, uint64_t cols) {
    const uint64_t least = (uint64_t)g.eval_points_across_min;
    if (k < least || ((unsigned __int128)m * k * cols >> g.eval_across_min_products_log) == 0) return 0;
    const uint64_t rest = k & (PE_W - 1);
    return rest >= least || rest == 0 ? k : k - rest;
}

template <int G>
void pe_launch_coeffs(const Fe* coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, const Fe* points, uint64_t k, uint64_t j0, uint64_t chunks, int chunk_log, Fe* dst,
                      uint64_t dst_col, uint64_t dst_point, hipStream_t st) {
    const uint64_t groups = (k - j0 + G - 1) / G;
    unsigned gy, gz;
    pe_tile(chunks, groups, cols, &gy, &gz);
    for (uint64_t c0 = 0; c0 < cols; c0 += gz)
        for (uint64_t q = 0; q < groups; q += gy)
            hipLaunchKernelGGL(pe_coeffs_across_kernel<G>, dim3((unsigned)chunks, (unsigned)std::min<uint64_t>(gy, groups - q), (unsigned)std::min<uint64_t>(gz, cols - c0)), dim3(PE_T),
                               0, st, coeffs, m, ld_in, points, k, j0 + q * G, c0, chunk_log, dst, dst_col, dst_point);
}

int polyeval_enqueue(const Fe* coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, const Fe* points, uint64_t k, Fe* out, uint64_t ld_out, hipStream_t st) {
    const uint64_t total = k * cols;
    if (m == 0) {
        for (uint64_t o0 = 0; o0 < total; o0 += PE_MAX_WGS * 256)
            hipLaunchKernelGGL(pe_zero_kernel, dim3((unsigned)((std::min(total - o0, PE_MAX_WGS * 256) + 255) / 256)), dim3(256), 0, st, out, ld_out, k, total, o0);
        HIPCHK(hipGetLastError());
        return SC_OK;
    }
    const uint64_t kb = polyeval_across(m, k, cols), ka = k - kb;
    const int G = ka == 1 ? 1 : (ka == 2 ? 2 : 4);
    // The chunk: as many chunks as it takes to fill the device with waves together with the points and columns (at most
    // PE_UNITS_WANTED, then: fewer chunks mean fewer partials and, coefficients across lanes, more Horner steps per fold), but no
    // chunk below 2^eval_chunk_log coefficients (one Horner stride by default: a short polynomial is latency, not throughput)
    const uint64_t units = ((kb + PE_W - 1) / PE_W + (ka + G - 1) / G * PE_UNITS_PER_WG) * cols;
    const uint64_t chunks_wanted = (PE_UNITS_WANTED + units - 1) / units;
    const int chunk_log = std::max(g.eval_chunk_log, ilog2((m + chunks_wanted - 1) / chunks_wanted));
    const uint64_t chunks = (m + (1ull << chunk_log) - 1) >> chunk_log;
    PoolTmpAsync partial;
    Fe* dst = out;
    uint64_t dst_col = ld_out, dst_point = 1;
    if (chunks > 1) {
        SCCHK(partial.get(total * chunks * sizeof(Fe)));
        dst = partial.fe();
        dst_col = k * chunks;
        dst_point = chunks;
    }
    if (kb) {
        const uint64_t rows = (kb + PE_W - 1) / PE_W;
        unsigned gy, gz;
        pe_tile(chunks, rows, cols, &gy, &gz);
        for (uint64_t c0 = 0; c0 < cols; c0 += gz)
            for (uint64_t q = 0; q < rows; q += gy)
                hipLaunchKernelGGL(pe_points_across_kernel, dim3((unsigned)chunks, (unsigned)std::min<uint64_t>(gy, rows - q), (unsigned)std::min<uint64_t>(gz, cols - c0)), dim3(PE_W), 0,
                                   st, coeffs, m, ld_in, points, q * PE_W, kb, c0, chunk_log, dst, dst_col, dst_point);
    }
    if (ka) {
        if (G == 1) pe_launch_coeffs<1>(coeffs, m, ld_in, cols, points, k, kb, chunks, chunk_log, dst, dst_col, dst_point, st);
        else if (G == 2) pe_launch_coeffs<2>(coeffs, m, ld_in, cols, points, k, kb, chunks, chunk_log, dst, dst_col, dst_point, st);
        else pe_launch_coeffs<4>(coeffs, m, ld_in, cols, points, k, kb, chunks, chunk_log, dst, dst_col, dst_point, st);
    }
    if (chunks > 1) {
        for (uint64_t o0 = 0; o0 < total; o0 += PE_MAX_WGS * 4)
            hipLaunchKernelGGL(pe_combine_kernel, dim3((unsigned)((std::min(total - o0, PE_MAX_WGS * 4) + 3) / 4)), dim3(4 * PE_W), 0, st, (const Fe*)partial.fe(), chunks, chunk_log,
                               points, k, total, o0, out, ld_out);
    }
    HIPCHK(hipGetLastError());
    return SC_OK;
}

}  // namespace

extern "C" {

int sc_poly_eval_points_dev(const void* d_coeffs, uint64_t m, uint64_t ld_in, uint64_t cols, const void* d_points, uint64_t k, void* d_out, uint64_t ld_out, void* stream) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    SCCHK(polyeval_args(d_coeffs, m, ld_in, cols, d_points, k, d_out, ld_out));
    if (k == 0 || cols == 0) return SC_OK;
    return polyeval_enqueue((const Fe*)d_coeffs, m, ld_in, cols, (const Fe*)d_points, k, (Fe*)d_out, ld_out, pick_stream(stream));
}

int sc_poly_eval_points(const void* coeffs, uint64_t m, const void* points, uint64_t k, void* out) {
    std::lock_guard<std::mutex> lk(g_mu);
    SCCHK(ensure_init());
    if ((m && !coeffs) || (k && (!points || !out))) return fail(SC_ERR_BAD_ARG, "null argument");
    if (m > PE_MAX || k > PE_MAX) return fail(SC_ERR_BAD_ARG, "more than 2^32 coefficients or points");
    if (k == 0) return SC_OK;
    PoolTmp dc, dp, dv;
    SCCHK(dc.get((m ? m : 1) * sizeof(Fe)));
    SCCHK(dp.get(k * sizeof(Fe)));
    SCCHK(dv.get(k * sizeof(Fe)));
    hipStream_t st = g.stream;
    // (a failure behind an upload waits for the stream: the host buffers are the caller's, the pool buffers go back on return)
    auto run = [&]() -> int {
        SCCHK(upload(dc.p, coeffs, m * sizeof(Fe), st));
        SCCHK(upload(dp.p, points, k * sizeof(Fe), st));
        SCCHK(polyeval_enqueue(dc.fe(), m, m, 1, dp.fe(), k, dv.fe(), k, st));
        HIPCHK(hipMemcpyAsync(out, dv.p, k * sizeof(Fe), hipMemcpyDeviceToHost, st));
        return SC_OK;
    };
    const int rc = run();
    if (hipStreamSynchronize(st) != hipSuccess && rc == SC_OK) return fail(SC_ERR_HIP, "evaluation at points failed");
    return rc;
}

}  // extern "C"

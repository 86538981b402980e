// grind.hip -- the proof-of-work search of grinding.py / Fri(grinding_bits): windows of trials on the device (csrc/grind.cuh), issued in
// ascending order by a host loop that stops at the first window that reports a hit; the same search on one host core.
#include "core.h"
#include "grind.cuh"
#include "transcript.h"

namespace sci {

// The window: trials per launch and member (sc_set_tuning("grind_window"), -1 = this default).  Measured (tools/grind_timing.py,
// profiles/grinding/grind_timing.txt): 2^30 nonces without a hit run at 0.77, 3.07, 5.21, 6.31, 6.70, 6.79, 6.85 G trials/s with
// windows of 2^14, 2^16, ... 2^26 -- a window is a launch, a copy of the members' words and a hand-over to the host -- while a
// 20-bit search, which ends in the first window or two, takes 0.18 ms at 2^20, 0.28 at 2^22 and 0.41 at 2^24 (the window queued
// behind the hit is waited for).  The default is the smallest window within 3 % of the best rate.
constexpr int GRIND_WINDOW_DEFAULT = 1 << 22;
constexpr uint64_t GRIND_MAX_MEMBERS = 65535;             // members ride blockIdx.y

static uint64_t grind_window() { return g.grind_window > 0 ? (uint64_t)g.grind_window : (uint64_t)GRIND_WINDOW_DEFAULT; }

// what a search holds between its set-up and its end: everything is the call's own (no shared scratch)
struct GrindRun {
    uint64_t count = 0;
    char* h = nullptr;            // pinned: [seeds 32 count][per slot: order 4 count (padded to 8), best 8 count]
    char* d = nullptr;            // device: [seeds 32 count][best 8 count][order slot 0][order slot 1]
    size_t d_bytes = 0, order_bytes = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    uint64_t* h_seeds() const { return (uint64_t*)h; }
    uint32_t* h_order(int slot) const { return (uint32_t*)(h + 32 * count + slot * (order_bytes + 8 * count)); }
    uint64_t* h_best(int slot) const { return (uint64_t*)(h + 32 * count + slot * (order_bytes + 8 * count) + order_bytes); }
    uint64_t* d_seeds() const { return (uint64_t*)d; }
    uint64_t* d_best() const { return (uint64_t*)(d + 32 * count); }
    uint32_t* d_order(int slot) const { return (uint32_t*)(d + 40 * count + slot * order_bytes); }
};

// under g_mu
static int grind_setup(GrindRun& r, uint64_t count) {
    r.count = count;
    r.order_bytes = (size_t)((4 * count + 7) & ~7ull);
    SCCHK(host_pool_get(32 * count + 2 * (r.order_bytes + 8 * count), (void**)&r.h));
    r.d_bytes = 40 * count + 2 * r.order_bytes;
    hipError_t e = pool_alloc((void**)&r.d, r.d_bytes);
    if (e != hipSuccess) { host_pool_put(r.h); r.h = nullptr; return fail(SC_ERR_HIP, hipGetErrorString(e)); }
    r.ev[0] = event_get();
    r.ev[1] = event_get();
    if (!r.ev[0] || !r.ev[1]) return fail(SC_ERR_HIP, "grind: no event");
    return SC_OK;
}
static void grind_teardown(GrindRun& r) {
    if (r.d) release_after_streams(r.d, r.d_bytes);
    if (r.h) host_pool_put(r.h);
    for (hipEvent_t e : r.ev) if (e) g_event_pool.push_back(e);
    r = GrindRun();
}

// The host loop, WITHOUT g_mu (a search waits for the device; searches on other streams and every other entry go on meanwhile).
// offsets_out[m]: the smallest accepted offset from `start` below max_nonces, GRIND_NONE when there is none.
//
// Windows go out in ascending order; one more is queued before the host waits for a window's word (the device does not idle while
// the host looks), and the loop ends at the first window after which every member has a hit -- a hit in the first window that has
// one is the member's global minimum, since every smaller offset lies in a window already tested in full.  A member with a hit
// leaves the next window's list; in the window queued meanwhile its lanes see the word below their offsets and leave at once.
static hipError_t grind_search(GrindRun& r, int bits, uint64_t start, uint64_t max_nonces, uint64_t window, bool unrolled, unsigned max_blocks, hipStream_t st,
                               uint64_t* offsets_out) {
    const uint64_t count = r.count;
#define GRIND_HIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { (void)hipStreamSynchronize(st); return _e; } } while (0)
    GRIND_HIP(hipMemcpyAsync(r.d_seeds(), r.h_seeds(), 32 * count, hipMemcpyHostToDevice, st));
    GRIND_HIP(hipMemsetAsync(r.d_best(), 0xFF, 8 * count, st));
    std::vector<uint32_t> active(count);
    for (uint64_t m = 0; m < count; ++m) { active[m] = (uint32_t)m; offsets_out[m] = GRIND_NONE; }
    uint64_t next_base = 0;                // the first offset no window covers yet
    auto issue = [&](int slot) -> hipError_t {
        const uint64_t w = max_nonces - next_base < window ? max_nonces - next_base : window;
        memcpy(r.h_order(slot), active.data(), 4 * active.size());
        hipError_t e = hipMemcpyAsync(r.d_order(slot), r.h_order(slot), 4 * active.size(), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        const uint64_t blocks = (w + 255) / 256;
        const dim3 grid((unsigned)(blocks < max_blocks ? blocks : max_blocks), (unsigned)active.size());
        if (unrolled) hipLaunchKernelGGL(sc::grind_window_kernel<true>, grid, dim3(256), 0, st, r.d_seeds(), r.d_order(slot), r.d_best(), start, next_base, w, bits);
        else hipLaunchKernelGGL(sc::grind_window_kernel<false>, grid, dim3(256), 0, st, r.d_seeds(), r.d_order(slot), r.d_best(), start, next_base, w, bits);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(r.h_best(slot), r.d_best(), 8 * count, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        next_base += w;
        return hipEventRecord(r.ev[slot], st);
    };
    int slot = 0;
    if (max_nonces && count) GRIND_HIP(issue(0));
    else return hipSuccess;
    for (;;) {
        const bool queued = next_base < max_nonces;
        if (queued) GRIND_HIP(issue(slot ^ 1));
        GRIND_HIP(hipEventSynchronize(r.ev[slot]));
        const uint64_t* best = r.h_best(slot);
        size_t keep = 0;
        for (size_t i = 0; i < active.size(); ++i) {
            const uint32_t m = active[i];
            if (best[m] != GRIND_NONE) offsets_out[m] = best[m];
            else active[keep++] = m;
        }
        active.resize(keep);
        if (active.empty() || !queued) break;
        slot ^= 1;
    }
    return hipStreamSynchronize(st);       // (a window queued behind the last one looked at: its copy must have landed before the buffers go back)
#undef GRIND_HIP
}

static int grind_check(const std::string& what, int bits, uint64_t start, uint64_t max_nonces) {
    if (bits < 1 || bits > 63) return fail(SC_ERR_BAD_ARG, what + "1 .. 63 bits expected");
    if (max_nonces && start > ~0ull - (max_nonces - 1)) return fail(SC_ERR_BAD_ARG, what + "the range passes 2^64");
    return SC_OK;
}

// held: the caller holds g_mu and keeps it through the search
static int grind_batch(const std::string& what, const void* seeds, uint64_t count, int bits, uint64_t start, uint64_t max_nonces, uint64_t* nonces_out,
                       uint8_t* found_out, void* stream, bool held) {
    GrindRun r;
    uint64_t window;
    bool unrolled;
    unsigned max_blocks;
    hipStream_t st;
    std::unique_lock<std::mutex> lk(g_mu, std::defer_lock);
    {
        if (!held) lk.lock();
        SCCHK(grind_check(what, bits, start, max_nonces));
        if (count > GRIND_MAX_MEMBERS) return fail(SC_ERR_BAD_ARG, what + "at most 65535 seeds per call");
        if (count && (!seeds || !nonces_out || !found_out)) return fail(SC_ERR_BAD_ARG, what + "null argument");
        if (count == 0) return SC_OK;
        SCCHK(ensure_init());
        st = pick_stream(stream);
        window = grind_window();
        unrolled = g.grind_unrolled != 0;
        // lanes in flight: every CU filled several times over, split among the members of a batch (a lane strides through its window)
        const uint64_t per_member = (uint64_t)g.num_cus * 16 / count;
        max_blocks = (unsigned)(per_member < 8 ? 8 : per_member);
        const int rc = grind_setup(r, count);
        if (rc != SC_OK) { grind_teardown(r); return rc; }
        memcpy(r.h_seeds(), seeds, 32 * count);
        if (!held) lk.unlock();
    }
    std::vector<uint64_t> offsets(count);
    const hipError_t e = grind_search(r, bits, start, max_nonces, window, unrolled, max_blocks, st, offsets.data());
    if (!held) lk.lock();
    grind_teardown(r);
    if (e != hipSuccess) return fail(SC_ERR_HIP, what + hipGetErrorString(e));
    for (uint64_t m = 0; m < count; ++m) {
        found_out[m] = offsets[m] != GRIND_NONE;
        if (found_out[m]) nonces_out[m] = start + offsets[m];
    }
    return SC_OK;
}

int grind_seeds_locked(const std::string& what, const void* seeds, uint64_t count, int bits, uint64_t start, uint64_t max_nonces, uint64_t* nonces_out,
                       uint8_t* found_out, void* stream) {
    return grind_batch(what, seeds, count, bits, start, max_nonces, nonces_out, found_out, stream, true);
}

}  // namespace sci

int sc_grind(const uint8_t seed32[32], int bits, uint64_t start, uint64_t max_nonces, uint64_t* nonce_out, int* found_out, void* stream) {
    const std::string what = "grind: ";
    if (!seed32 || !nonce_out || !found_out) { std::lock_guard<std::mutex> lk(g_mu); return fail(SC_ERR_BAD_ARG, what + "null argument"); }
    uint8_t found = 0;
    uint64_t nonce = 0;
    SCCHK(grind_batch(what, seed32, 1, bits, start, max_nonces, &nonce, &found, stream, false));
    *found_out = found;
    if (found) *nonce_out = nonce;
    return SC_OK;
}

int sc_grind_batch(const uint8_t* seeds, uint64_t count, int bits, uint64_t start, uint64_t max_nonces, uint64_t* nonces_out, uint8_t* found_out, void* stream) {
    return grind_batch("grind batch: ", seeds, count, bits, start, max_nonces, nonces_out, found_out, stream, false);
}

int sc_grind_host(const uint8_t seed32[32], int bits, uint64_t start, uint64_t max_nonces, uint64_t* nonce_out, int* found_out) {
    const std::string what = "grind host: ";
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (!seed32 || !nonce_out || !found_out) return fail(SC_ERR_BAD_ARG, what + "null argument");
        SCCHK(grind_check(what, bits, start, max_nonces));
    }
    uint64_t seed[4];
    memcpy(seed, seed32, 32);
    *found_out = 0;
    for (uint64_t o = 0; o < max_nonces; ++o) {
        uint64_t s[25] = {seed[0], seed[1], seed[2], seed[3], start + o, 0x1full};
        s[16] = 1ull << 63;
        sc::keccak_f1600(s);
        if (sc::grind_accepts(s[0], bits)) {
            *nonce_out = start + o;
            *found_out = 1;
            break;
        }
    }
    return SC_OK;
}

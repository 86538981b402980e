// CPU walk of the Merkle forest's launches with the indexing functions the HIP kernels use (csrc/merkle_forest.cuh: the flat
// numbering, forest_place, the launch plan, the query kernel's routing and path gather).  The device BLAKE2b and decimal leaf encoder
// of merkle.cuh are device-only, so this build hashes with the host compression of csrc/transcript.h; what it checks is who hashes
// what and where it is stored: the climb loop below is this file's own restatement of forest_climb_kernel's one-lane walk over
// workgroup wg, thread t and level l, with an array in place of LDS; the placement of every node and the launch plan are the shared
// functions.  Not covered here (the GPU tests cover them): the fold's addressing and the four-lane levels' stores.
// Test infrastructure (built by tests/test_forest_emu.py).
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../stark-anatomy_amd/csrc/merkle_forest.cuh"
#include "../../stark-anatomy_amd/csrc/transcript.h"

using namespace sc;

static void leaf_digest(const uint8_t* residue, uint8_t out[64]) {
    unsigned __int128 v;
    memcpy(&v, residue, 16);
    char digits[40];
    int nd = 0;
    do { digits[nd++] = (char)('0' + (int)(v % 10)); v /= 10; } while (v);
    uint8_t text[40];
    for (int i = 0; i < nd; ++i) text[i] = (uint8_t)digits[nd - 1 - i];
    blake2b_512(text, (size_t)nd, out);
}

extern "C" {
// levels: count * 2N digests (tree-major), zeroed by the caller; roots: 64 bytes per tree; stats: launches, workgroups in all, workgroups
// of the first launch.  Returns 0, or -1 if a store fell outside the forest or hit a digest twice.
int emu_forest_build(const uint8_t* elems, uint64_t N, uint64_t count, uint8_t* levels, uint8_t* roots, uint64_t stats[3]) {
    ForestShape s{N, count, 0};
    while ((1ull << s.logN) < N) ++s.logN;
    std::vector<uint8_t> written(count * 2 * N, 0);
    stats[0] = stats[1] = stats[2] = 0;
    int lvl0 = 0;
    do {
        const int nlev = forest_launch_levels(s.logN, lvl0);
        const uint64_t wgs = forest_launch_workgroups(s, lvl0);
        if (lvl0 == 0) stats[2] = wgs;
        stats[0] += 1;
        stats[1] += wgs;
        for (uint64_t wg = 0; wg < wgs; ++wg) {
            uint8_t lds[FOREST_WG][64], nxt[FOREST_WG / 2][64];
            memset(lds, 0, sizeof lds);
            for (uint32_t t = 0; t < FOREST_WG; ++t) {                 // entry: leaves hashed, or nodes read
                uint64_t dig;
                const uint64_t flat = forest_wg_flat(wg, 0, t);
                if (!forest_place(s, lvl0, flat, &dig)) continue;
                if (lvl0 == 0) leaf_digest(elems + 16 * flat, lds[t]);
                else memcpy(lds[t], levels + 64 * dig, 64);
            }
            uint32_t width = FOREST_WG;
            for (int l = 0;; ++l) {
                if (lvl0 == 0 || l > 0) {
                    for (uint32_t p = 0; p < width; ++p) {             // publish
                        uint64_t dig, tree;
                        if (!forest_place(s, lvl0 + l, forest_wg_flat(wg, l, p), &dig, &tree)) continue;
                        if (dig >= count * 2 * N || written[dig]) return -1;
                        written[dig] = 1;
                        memcpy(levels + 64 * dig, lds[p], 64);
                        if (lvl0 + l == s.logN) memcpy(roots + 64 * tree, lds[p], 64);
                    }
                }
                if (l == nlev) break;
                width >>= 1;
                for (uint32_t t = 0; t < width; ++t) {
                    uint8_t msg[128];
                    memcpy(msg, lds[2 * t], 64);
                    memcpy(msg + 64, lds[2 * t + 1], 64);
                    blake2b_512(msg, 128, nxt[t]);
                }
                memcpy(lds, nxt, (size_t)width * 64);
            }
        }
        lvl0 += nlev;
    } while (lvl0 < s.logN);
    return 0;
}

// the query kernel, thread by thread: pairs of (levels, elems, N, count of openings)
int emu_forest_query(uint64_t n_pairs, const uint8_t* const* levels, const uint8_t* const* elems, const uint64_t* Ns, const uint64_t* counts, const uint64_t* trees,
                     const uint64_t* indices, uint8_t* elems_out, uint8_t* paths_out) {
    if (n_pairs > (uint64_t)FOREST_QUERY_MAX_PAIRS) return -1;
    ForestQuery Q;
    Q.count = 0;
    Q.total_threads = 0;
    uint64_t off = 0, poff = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (!counts[p]) continue;
        ForestQueryPair& T = Q.p[Q.count++];
        T.levels = (const uint64_t*)levels[p];
        T.elems = (const Fe*)elems[p];
        T.N = Ns[p];
        T.logN = 0;
        while ((1ull << T.logN) < T.N) ++T.logN;
        T.per_query = 4 * T.logN + 1;
        T.thread_off = Q.total_threads;
        T.idx_off = off;
        T.path_off = poff;
        Q.total_threads += counts[p] * T.per_query;
        off += counts[p];
        poff += counts[p] * T.logN;
    }
    for (uint64_t t = 0; t < Q.total_threads; ++t) {
        int w;
        uint64_t q;
        uint32_t r;
        forest_query_route(Q, t, &w, &q, &r);
        const ForestQueryPair& T = Q.p[w];
        const uint64_t tree = trees[T.idx_off + q], idx = indices[T.idx_off + q];
        if (r == T.per_query - 1) {
            memcpy(elems_out + 16 * (T.idx_off + q), (const uint8_t*)T.elems + 16 * (tree * T.N + idx), 16);
        } else {
            const uint32_t quarter = r & 3u, l = r >> 2;
            memcpy(paths_out + 64 * (T.path_off + q * T.logN + l) + 16 * quarter, (const uint8_t*)T.levels + 64 * forest_path_digest(T.N, tree, idx, l) + 16 * quarter, 16);
        }
    }
    return 0;
}
}

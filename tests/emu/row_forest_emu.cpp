// CPU walk of a ROW forest's launches (csrc/merkle_forest.cuh's forest_climb_kernel with the row leaf stage of csrc/merkle_rows.cuh):
// the same SC_HD functions the kernels run -- row_segment_address (which segment holds a column, where its value lies),
// forest_place / forest_wg_flat (who hashes what and where it is stored), the launch plan, row_leaf_walk (blocks, message words, counter,
// final flag, personalised state) -- compiled by g++ over transcript.h's compression and called workgroup by workgroup, lane by lane.
// Every address a lane reads is recorded and checked to lie inside the bytes of its segment; lanes past the last tree must read nothing.
// The climb above level 0 is tests/emu/merkle_forest_emu.cpp's restatement of the one-lane walk.  Test infrastructure (built by
// tests/test_row_forest_cpu.py).
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../stark-anatomy_amd/csrc/merkle_forest.cuh"
#include "../../stark-anatomy_amd/csrc/merkle_rows.cuh"
#include "../../stark-anatomy_amd/csrc/transcript.h"

using namespace sc;

namespace {
struct Reads {
    const RowSegments* S;
    const uint64_t* seg_bytes;        // bytes of every segment's buffer
    uint64_t count = 0, outside = 0;
    void note(const Fe* p) {
        ++count;
        bool inside = false;
        for (uint32_t s = 0; s < S->n; ++s) {
            const uint8_t* lo = (const uint8_t*)S->seg[s].base;
            if ((const uint8_t*)p >= lo && (const uint8_t*)p + 16 <= lo + seg_bytes[s]) inside = true;
        }
        if (!inside) ++outside;
    }
};
struct Lane {                          // RowForestColumns::Source on the host
    const RowSegments& S;
    uint64_t tree, row;
    Reads* reads;
    RowSegmentCursor k;
    void gate(bool) const {}
    Fe at(uint32_t c) {
        const Fe* p = row_segment_address(S, tree, c, row, k);
        reads->note(p);
        if (reads->outside) return Fe{0, 0};
        return *p;
    }
};
void compress(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last) {
    uint8_t block[128];
    memcpy(block, m, 128);
    blake2b_compress(h, block, t, last);
}
bool table(const void* const* bases, const uint64_t* per_tree, const uint64_t* pitch, uint64_t n_segs, uint64_t N, RowSegments* S) {
    if (!bases || !per_tree || !pitch || n_segs == 0 || n_segs > ROW_FOREST_MAX_SEGMENTS) return false;
    uint64_t w = 0;
    for (uint64_t s = 0; s < n_segs; ++s) {
        if (!bases[s] || per_tree[s] == 0 || per_tree[s] > ROWS_MAX_COLUMNS || pitch[s] < N) return false;
        S->seg[s] = RowSegment{(const Fe*)bases[s], per_tree[s], pitch[s]};
        w += per_tree[s];
    }
    if (w > ROWS_MAX_COLUMNS) return false;
    S->n = (uint32_t)n_segs;
    S->w = (uint32_t)w;
    return true;
}
}  // namespace

extern "C" {

// levels: count * 2N digests (tree-major), zeroed by the caller; roots: 64 bytes per tree; stats: launches, workgroups in all, values
// read.  Returns 0; -1: a store fell outside the forest or hit a digest twice; -2: a lane read outside its segments; -3: a bad table.
int emu_row_forest_build(const void* const* bases, const uint64_t* per_tree, const uint64_t* pitch, const uint64_t* seg_bytes, uint64_t n_segs, uint64_t N,
                         uint64_t count, uint8_t* levels, uint8_t* roots, uint64_t stats[3]) {
    RowSegments S;
    if (!table(bases, per_tree, pitch, n_segs, N, &S) || N < 2 || (N & (N - 1)) || count == 0) return -3;
    ForestShape s{N, count, 0};
    while ((1ull << s.logN) < N) ++s.logN;
    Reads reads{&S, seg_bytes};
    std::vector<uint8_t> written(count * 2 * N, 0);
    stats[0] = stats[1] = stats[2] = 0;
    int lvl0 = 0;
    do {
        const int nlev = forest_launch_levels(s.logN, lvl0);
        const uint64_t wgs = forest_launch_workgroups(s, lvl0);
        stats[0] += 1;
        stats[1] += wgs;
        for (uint64_t wg = 0; wg < wgs; ++wg) {
            uint8_t lds[FOREST_WG][64], nxt[FOREST_WG / 2][64];
            memset(lds, 0, sizeof lds);
            for (uint32_t t = 0; t < FOREST_WG; ++t) {                 // entry: rows hashed, or nodes read
                uint64_t dig, tree;
                const uint64_t flat = forest_wg_flat(wg, 0, t);
                if (!forest_place(s, lvl0, flat, &dig, &tree)) continue;                // (a lane past the last tree loads nothing)
                if (lvl0 == 0) {
                    uint64_t h[8];
                    row_leaf_walk(S.w, Lane{S, tree, flat & (N - 1), &reads, RowSegmentCursor{}}, compress, h);
                    memcpy(lds[t], h, 64);
                } else {
                    memcpy(lds[t], levels + 64 * dig, 64);
                }
            }
            if (reads.outside) return -2;
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
    stats[2] = reads.count;
    return 0;
}

// row_forest_query_kernel thread by thread: rows_out [k][w] values, paths_out [k][64 log2 N] bytes.  Same return codes.
int emu_row_forest_query(const void* const* bases, const uint64_t* per_tree, const uint64_t* pitch, const uint64_t* seg_bytes, uint64_t n_segs, uint64_t N,
                         const uint8_t* levels, const uint64_t* trees, const uint64_t* indices, uint64_t k, uint8_t* rows_out, uint8_t* paths_out) {
    RowSegments S;
    if (!table(bases, per_tree, pitch, n_segs, N, &S)) return -3;
    uint32_t logN = 0;
    while ((1ull << logN) < N) ++logN;
    Reads reads{&S, seg_bytes};
    const uint64_t per = row_forest_query_threads(S.w, logN);
    for (uint64_t t = 0; t < k * per; ++t) {
        const uint64_t q = t / per;
        const uint32_t r = (uint32_t)(t % per);
        if (r < S.w) {
            RowSegmentCursor cur;
            const Fe* p = row_segment_address(S, trees[q], r, indices[q], cur);
            reads.note(p);
            if (reads.outside) return -2;
            memcpy(rows_out + 16 * (q * S.w + r), p, 16);
        } else {
            const uint32_t quarter = (r - S.w) & 3u, l = (r - S.w) >> 2;
            memcpy(paths_out + 64 * (q * logN + l) + 16 * quarter, levels + 64 * forest_path_digest(N, trees[q], indices[q], l) + 16 * quarter, 16);
        }
    }
    return 0;
}

}  // extern "C"

#ifdef ROW_FOREST_EMU_MAIN
// stand-alone form (for sanitizer builds).  file: repeated [u64 n_segs][u64 N][u64 count][u64 pitch][u64 per_tree x n_segs], then every
// segment's count * per_tree * pitch elements; prints one line of hex per forest: its roots, then the path of the last row of the last tree
#include <cstdio>
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[4];
    while (fread(head, 8, 4, f) == 4) {
        const uint64_t n_segs = head[0], N = head[1], count = head[2], pitch = head[3];
        if (n_segs == 0 || n_segs > ROW_FOREST_MAX_SEGMENTS || N > (1u << 12) || count > 1024 || pitch > (1u << 13)) { fclose(f); return 3; }
        uint64_t per_tree[ROW_FOREST_MAX_SEGMENTS], pitches[ROW_FOREST_MAX_SEGMENTS], bytes[ROW_FOREST_MAX_SEGMENTS];
        if (fread(per_tree, 8, n_segs, f) != n_segs) { fclose(f); return 3; }
        std::vector<std::vector<Fe>> data(n_segs);
        const void* bases[ROW_FOREST_MAX_SEGMENTS];
        for (uint64_t s = 0; s < n_segs; ++s) {
            if (per_tree[s] > ROWS_MAX_COLUMNS) { fclose(f); return 3; }
            const uint64_t elems = count * per_tree[s] * pitch;
            data[s].resize(elems);
            if (elems && fread(data[s].data(), 16, elems, f) != elems) { fclose(f); return 3; }
            bases[s] = data[s].data();
            pitches[s] = pitch;
            bytes[s] = 16 * elems;
        }
        uint32_t logN = 0;
        while ((1ull << logN) < N) ++logN;
        std::vector<uint8_t> levels(64 * 2 * N * count, 0), roots(64 * count), row(16 * ROWS_MAX_COLUMNS), path(64 * logN + 1);
        uint64_t stats[3];
        if (emu_row_forest_build(bases, per_tree, pitches, bytes, n_segs, N, count, levels.data(), roots.data(), stats)) { fclose(f); return 4; }
        const uint64_t tree = count - 1, index = N - 1;
        if (emu_row_forest_query(bases, per_tree, pitches, bytes, n_segs, N, levels.data(), &tree, &index, 1, row.data(), path.data())) { fclose(f); return 4; }
        for (uint64_t i = 0; i < 64 * count; ++i) printf("%02x", roots[i]);
        for (uint64_t i = 0; i < 64 * logN; ++i) printf("%02x", path[i]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
#endif

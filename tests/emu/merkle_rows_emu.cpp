// CPU walk of the row-commitment leaf stage: the SAME block walk the HIP kernels run (csrc/merkle_rows.cuh row_leaf_walk: which column
// lands in which message word of which block, the byte counter, the final flag, the personalised initial state), compiled by g++ over
// transcript.h's blake2b_compress and called once per lane (= row) the way the kernels index their column table.  Test infrastructure: a
// shared object for tests/test_merkle_rows_cpu.py, and with -DMERKLE_ROWS_EMU_MAIN a stand-alone program (for sanitizer builds) that
// reads matrices from a file and prints their leaf digests.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../stark-anatomy_amd/csrc/merkle_rows.cuh"
#include "../../stark-anatomy_amd/csrc/transcript.h"

using namespace sc;

namespace {
struct Columns {                       // RowColumns::Source on the host: lane `row` reads col[c][row]
    const Fe* const* col;
    uint64_t row;
    void gate(bool) const {}
    Fe at(uint32_t c) const { return col[c][row]; }
};
void compress(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last) {
    uint8_t block[128];
    memcpy(block, m, 128);
    blake2b_compress(h, block, t, last);
}
}  // namespace

extern "C" {

// digests_out[64 * i] = the leaf digest of row i of the w columns cols[c][0 .. N); 0: done, 1: a bad argument (nothing is written)
int emu_row_leaves(const void* const* cols, uint64_t w, uint64_t N, uint8_t* digests_out) {
    if (!cols || !digests_out || w == 0 || w > ROWS_MAX_COLUMNS) return 1;
    for (uint64_t c = 0; c < w; ++c) if (!cols[c]) return 1;
    for (uint64_t i = 0; i < N; ++i) {
        uint64_t h[8];
        row_leaf_walk((uint32_t)w, Columns{(const Fe* const*)cols, i}, compress, h);
        memcpy(digests_out + 64 * i, h, 64);
    }
    return 0;
}

}  // extern "C"

#ifdef MERKLE_ROWS_EMU_MAIN
// file: repeated [u64 w][u64 N][w columns of N elements, 16 bytes each]; prints one line of hex per matrix (its N digests)
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[2];
    while (fread(head, 8, 2, f) == 2) {
        const uint64_t w = head[0], N = head[1];
        if (w == 0 || w > ROWS_MAX_COLUMNS || N > (1u << 20)) { fclose(f); return 3; }
        std::vector<std::vector<Fe>> data(w, std::vector<Fe>(N));
        std::vector<const void*> cols(w);
        for (uint64_t c = 0; c < w; ++c) {
            if (N && fread(data[c].data(), 16, N, f) != N) { fclose(f); return 3; }
            cols[c] = data[c].data();
        }
        std::vector<uint8_t> out(64 * N + 1);
        if (emu_row_leaves(cols.data(), w, N, out.data())) { fclose(f); return 4; }
        for (uint64_t i = 0; i < 64 * N; ++i) printf("%02x", out[i]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
#endif

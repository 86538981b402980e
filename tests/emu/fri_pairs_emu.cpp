// CPU walk of the fused fold-and-hash leaf stage of FRI's pair trees (csrc/fri_pairs.cuh PairFold): the SAME per-lane index function
// the HIP kernel runs (pair_fold_lane: which four inputs, which two outputs, which twiddle exponents), the fold in the kernel's own
// expression over field.cuh's host arithmetic, and the 32-byte row through row_leaf_walk over transcript.h's blake2b_compress -- compiled
// by g++ and called once per lane.  Test infrastructure: a shared object for tests/test_fri_pairs_cpu.py, and with -DFRI_PAIRS_EMU_MAIN a
// stand-alone program (for sanitizer builds) that reads cases from a file and prints the folded codeword and the leaf digests.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../stark-anatomy_amd/csrc/fri_pairs.cuh"
#include "../../stark-anatomy_amd/csrc/transcript.h"

using namespace sc;

namespace {
void compress(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last) {
    uint8_t block[128];
    memcpy(block, m, 128);
    blake2b_compress(h, block, t, last);
}
}  // namespace

extern "C" {

// in: N = 4q elements; tw_m[e], e < 2q: c * w^-e in Montgomery form.  Per lane j < q: lanes_out[8 j ..] = in[0..3], out[0..1], exp[0..1]
// of pair_fold_lane; out[] takes the folded elements, writes_out[i] counts the stores to out[i]; digests_out[64 j] = leaf j.
// 0: done, 1: a bad argument, 2: a lane's index outside its array (nothing is read or written through it)
int emu_pair_fold(const void* in, uint64_t N, const void* tw_m, void* out, uint32_t* writes_out, uint64_t* lanes_out, uint8_t* digests_out) {
    if (!in || !tw_m || !out || !writes_out || !lanes_out || !digests_out || N < 4 || (N & (N - 1))) return 1;
    const uint64_t q = N / 4;
    const Fe* x = (const Fe*)in;
    const Fe* tw = (const Fe*)tw_m;
    Fe* y = (Fe*)out;
    for (uint64_t j = 0; j < q; ++j) {
        const PairFoldLane L = pair_fold_lane(j, q);
        for (int k = 0; k < 4; ++k) { if (L.in[k] >= N) return 2; lanes_out[8 * j + k] = L.in[k]; }
        for (int k = 0; k < 2; ++k) {
            if (L.out[k] >= 2 * q || L.exp[k] >= 2 * q) return 2;
            lanes_out[8 * j + 4 + k] = L.out[k];
            lanes_out[8 * j + 6 + k] = L.exp[k];
        }
        PairSource pair;
        for (int k = 0; k < 2; ++k) {
            const Fe a = x[L.in[2 * k]], b = x[L.in[2 * k + 1]];
            pair.v[k] = fe_add(fe_half(fe_add(a, b)), mont_mul(fe_sub(a, b), tw[L.exp[k]]));
            y[L.out[k]] = pair.v[k];
            ++writes_out[L.out[k]];
        }
        uint64_t h[8];
        row_leaf_walk(2u, pair, compress, h);
        memcpy(digests_out + 64 * j, h, 64);
    }
    return 0;
}

}  // extern "C"

#ifdef FRI_PAIRS_EMU_MAIN
// file: repeated [u64 N][N elements][N/2 twiddles], 16 bytes each; prints two lines of hex per case: the folded codeword, the leaf digests
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t N;
    while (fread(&N, 8, 1, f) == 1) {
        if (N < 4 || (N & (N - 1)) || N > (1u << 20)) { fclose(f); return 3; }
        std::vector<Fe> in(N), tw(N / 2), out(N / 2);
        if (fread(in.data(), 16, N, f) != N || fread(tw.data(), 16, N / 2, f) != N / 2) { fclose(f); return 3; }
        std::vector<uint32_t> writes(N / 2, 0);
        std::vector<uint64_t> lanes(8 * (N / 4));
        std::vector<uint8_t> digests(64 * (N / 4));
        if (emu_pair_fold(in.data(), N, tw.data(), out.data(), writes.data(), lanes.data(), digests.data())) { fclose(f); return 4; }
        for (uint32_t w : writes) if (w != 1) { fclose(f); return 5; }
        const uint8_t* o = (const uint8_t*)out.data();
        for (uint64_t i = 0; i < 16 * (N / 2); ++i) printf("%02x", o[i]);
        printf("\n");
        for (uint64_t i = 0; i < digests.size(); ++i) printf("%02x", digests[i]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
#endif

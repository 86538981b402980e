// CPU build of the batched verifier's row checks: the SAME merkle_check_row / colinearity_check_row the HIP kernels run
// (csrc/merkle_verify.cuh), one row at a time.  The device BLAKE2b and decimal leaf encoder of merkle.cuh are device-only
// (gfx950 intrinsics), so this build hashes with the host compression of csrc/transcript.h and a plain decimal encoder; what it
// checks is everything around them: row layout, indexing, the position bits, the root comparison and the colinearity
// arithmetic.  Test infrastructure (built by tests/test_verify_emu.py).
#include <cstdint>
#include <cstring>
#include "../../stark-anatomy_amd/csrc/merkle_verify.cuh"
#include "../../stark-anatomy_amd/csrc/transcript.h"

using namespace sc;

struct HostBlake2b {
    static uint32_t leaf(Fe x, uint64_t m[16]) {
        unsigned __int128 v = ((unsigned __int128)x.hi << 64) | x.lo;
        char digits[40];
        int nd = 0;
        do { digits[nd++] = (char)('0' + (int)(v % 10)); v /= 10; } while (v);
        uint8_t block[128];
        memset(block, 0, sizeof block);
        for (int i = 0; i < nd; ++i) block[i] = (uint8_t)digits[nd - 1 - i];
        memcpy(m, block, 128);
        return (uint32_t)nd;
    }
    static void block(const uint64_t m[16], uint32_t len, uint64_t h[8]) {
        uint8_t in[128], out[64];
        memcpy(in, m, 128);
        blake2b_512(in, len, out);
        memcpy(h, out, 64);
    }
};

extern "C" {
int emu_row_sizes(uint64_t out[3]) {
    out[0] = sizeof(MerkleCheckRow);
    out[1] = sizeof(ColinearityRow);
    out[2] = sizeof(ColinearityRound);
    return 0;
}
// the kernels' loops (base 0: the whole tables are "staged")
void emu_merkle_verify(const void* rows, uint64_t n, const void* digests, const void* roots, uint8_t* out) {
    const MerkleCheckRow* r = (const MerkleCheckRow*)rows;
    const uint64_t* d = (const uint64_t*)digests;
    for (uint64_t i = 0; i < n; ++i)
        out[i] = merkle_check_row<HostBlake2b>(r[i], d, 0, r[i].kind == MV_LEAF_DIGEST ? d + 8 * r[i].leaf[0] : nullptr, (const uint64_t*)roots, 0);
}
void emu_colinearity(const void* rows, uint64_t n, const void* rounds, uint8_t* out) {
    const ColinearityRow* r = (const ColinearityRow*)rows;
    for (uint64_t i = 0; i < n; ++i) out[i] = colinearity_check_row(r[i], (const ColinearityRound*)rounds, 0);
}
}

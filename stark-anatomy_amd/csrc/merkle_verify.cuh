// merkle_verify.cuh -- the verifier's checks as flat rows, one thread per row (FastStark.verify_batch / Fri.verify_batch).
//
//   Merkle check       Merkle.verify_(root, position, path, leaf) of stark-anatomy_amd/merkle.py: the leaf is a residue (hashed as
//                      its decimal ASCII, merkle.cuh leaf_message) or a ready digest; then per level node = H(node || sibling) when
//                      the position bit is 0, H(sibling || node) when it is 1 -- one 128-byte block each -- and the node left at the
//                      top is compared with the root.
//   colinearity test   univariate.test_colinearity([(x_a, y_a), (x_b, y_b), (alpha, y_c)]) with x = offset * omega^e: for distinct
//                      abscissas (y_b - y_a)(alpha - x_a) == (y_c - y_a)(x_b - x_a) and y_b != y_a.  Coinciding abscissas (and any
//                      input that is not a canonical residue) leave the row undecided; the host decides it with test_colinearity.
//
// The row functions are written once over a hash policy: the kernels below use the device BLAKE2b of merkle.cuh, and
// tests/emu/merkle_verify_emu.cpp compiles the same functions for the host with the host compression of transcript.h.
// Layouts are mirrored by stark-anatomy_amd/starkcore.py (MERKLE_ROW, COLINEARITY_ROW, COLINEARITY_ROUND).
#pragma once
#include "field.cuh"
#if defined(__HIPCC__)
#include "merkle.cuh"
#endif

namespace sc {

enum : uint32_t { MV_LEAF_RESIDUE = 0, MV_LEAF_DIGEST = 1 };
enum : uint8_t { MV_REJECT = 0, MV_ACCEPT = 1, MV_UNDECIDED = 2 };
constexpr uint32_t MV_MAX_DEPTH = 64;

struct MerkleCheckRow {     // 48 bytes
    uint64_t position;
    uint64_t path;          // digest index of the first sibling (siblings path .. path + depth - 1, leaf level first)
    uint32_t root;          // index into the table of 64-byte roots
    uint32_t depth;         // <= MV_MAX_DEPTH
    uint32_t kind;          // MV_LEAF_RESIDUE: leaf = the residue (lo, hi); MV_LEAF_DIGEST: leaf[0] = digest index of the leaf digest
    uint32_t reserved;
    uint64_t leaf[2];
};

struct ColinearityRound {   // one per proof and FRI round: the round's coset and its challenge, canonical residues
    Fe offset, omega, alpha;
};

struct ColinearityRow {     // 80 bytes
    uint64_t a, b;          // exponents of x_a = offset * omega^a and x_b = offset * omega^b (b = a + half)
    uint32_t round;         // index into the round table
    uint32_t reserved[3];
    Fe ya, yb, yc;
};

// digests: the staged digests, the first of which has index digest_base (they cover the row's path, path .. path + depth - 1);
// leaf_digest: the row's leaf digest when its kind is MV_LEAF_DIGEST (staged on its own: it may lie anywhere in the caller's table);
// roots: the staged roots, the first of which has index root_base.  The caller has checked that every index of the row lies inside
// what is staged.
template <class Hash>
SC_HD uint8_t merkle_check_row(const MerkleCheckRow& r, const uint64_t* digests, uint64_t digest_base, const uint64_t* leaf_digest,
                               const uint64_t* roots, uint32_t root_base) {
    if (r.depth > MV_MAX_DEPTH || (r.depth < 64 && (r.position >> r.depth) != 0)) return MV_REJECT;   // merkle.py verify_: the index assertion
    uint64_t h[8], m[16];
    if (r.kind == MV_LEAF_RESIDUE) {
        const uint32_t len = Hash::leaf(Fe{r.leaf[0], r.leaf[1]}, m);
        Hash::block(m, len, h);
    } else {
        for (int i = 0; i < 8; ++i) h[i] = leaf_digest[i];
    }
    uint64_t pos = r.position;
    const uint64_t* sib = digests + 8 * (r.path - digest_base);
    for (uint32_t l = 0; l < r.depth; ++l, sib += 8, pos >>= 1) {
        const bool right = pos & 1;               // the node is the right child: H(sibling || node)
        for (int i = 0; i < 8; ++i) {
            const uint64_t s = sib[i];
            m[i] = right ? s : h[i];
            m[8 + i] = right ? h[i] : s;
        }
        Hash::block(m, 128u, h);
    }
    const uint64_t* root = roots + 8 * (r.root - root_base);
    uint64_t diff = 0;
    for (int i = 0; i < 8; ++i) diff |= h[i] ^ root[i];
    return diff == 0 ? MV_ACCEPT : MV_REJECT;
}

SC_HD uint8_t colinearity_check_row(const ColinearityRow& r, const ColinearityRound* rounds, uint32_t round_base) {
    const ColinearityRound& R = rounds[r.round - round_base];
    if (fe_ge_p(R.offset) || fe_ge_p(R.omega) || fe_ge_p(R.alpha) || fe_ge_p(r.ya) || fe_ge_p(r.yb) || fe_ge_p(r.yc)) return MV_UNDECIDED;
    const Fe offset_m = to_mont(R.offset), omega_m = to_mont(R.omega);
    const Fe xa = from_mont(mont_mul(offset_m, mont_pow(omega_m, r.a)));
    const Fe xb = from_mont(mont_mul(offset_m, mont_pow(omega_m, r.b)));
    if (fe_eq(xa, xb) || fe_eq(xa, R.alpha) || fe_eq(xb, R.alpha)) return MV_UNDECIDED;
    // both sides are Montgomery products (a factor R^-1 each), so the comparison needs no conversion
    const Fe lhs = mont_mul(fe_sub(r.yb, r.ya), fe_sub(R.alpha, xa));
    const Fe rhs = mont_mul(fe_sub(r.yc, r.ya), fe_sub(xb, xa));
    return (fe_eq(lhs, rhs) && !fe_eq(r.yb, r.ya)) ? MV_ACCEPT : MV_REJECT;
}

#if defined(__HIPCC__)
struct DeviceBlake2b {
    static __device__ __forceinline__ uint32_t leaf(Fe x, uint64_t m[16]) { return leaf_message(x, m); }
    static __device__ __forceinline__ void block(const uint64_t m[16], uint32_t len, uint64_t h[8]) { blake2b_single_block(m, len, h); }
};

// One lane per check: a proof has a few thousand rows, so the call is latency-bound (a depth-24 climb is 25 dependent compressions)
// and a wider spread of one check would only lengthen the chain of cross-lane exchanges.  Verdicts are plain byte stores.
// leaf_digests: one 64-byte slot per row of the chunk (read only for MV_LEAF_DIGEST rows)
__global__ void __launch_bounds__(256) merkle_verify_kernel(const MerkleCheckRow* __restrict__ rows, uint64_t n, const uint64_t* __restrict__ digests,
                                                            uint64_t digest_base, const uint64_t* __restrict__ leaf_digests,
                                                            const uint64_t* __restrict__ roots, uint32_t root_base, uint8_t* __restrict__ verdicts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    verdicts[i] = merkle_check_row<DeviceBlake2b>(rows[i], digests, digest_base, leaf_digests + 8 * i, roots, root_base);
}

__global__ void __launch_bounds__(256) colinearity_kernel(const ColinearityRow* __restrict__ rows, uint64_t n, const ColinearityRound* __restrict__ rounds,
                                                          uint32_t round_base, uint8_t* __restrict__ verdicts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    verdicts[i] = colinearity_check_row(rows[i], rounds, round_base);
}
#endif  // __HIPCC__

}  // namespace sc

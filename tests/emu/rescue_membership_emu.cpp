// CPU build of the path trace's lane functions: the SAME code the HIP kernels run (csrc/rescue_merkle.cuh), compiled by g++ with the
// portable field arithmetic, one item after the other.  The wide form is rm_path_trace_w as it is; the split form is its per-lane pieces
// (rm_trace_element, rm_trace_first, rm_trace_fill, rm_split_power, rm_split_mix, rm_split_constant) run lane by lane in the order
// rm_path_trace_split runs them, the exchange -- a shuffle on the device -- being a plain array here.  Test infrastructure (built by
// tests/test_rescue_membership_cpu.py; with RESCUE_MEMBERSHIP_MAIN a stand-alone program that the same test builds with
// -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../stark-anatomy_amd/csrc/rescue_merkle.cuh"

using namespace sc;

static std::vector<Fe> load(const void* params, int m, int rounds) {
    const Fe* h = (const Fe*)params;
    std::vector<Fe> C(m * m + 2 * m * rounds);
    for (size_t i = 0; i < C.size(); ++i) C[i] = to_mont(h[i]);
    return C;
}

// the split form of one item: M lanes in lockstep
template <int M>
static void split_trace(const Fe* C, int rounds, int d, const Fe* leaf, uint64_t index, const Fe* path, int depth, Fe* out, uint64_t T) {
    Fe own[M], s[M];
    for (int r = 0; r < M; ++r) {
        own[r] = r < d ? rp_reduce(leaf[r]) : fe_zero();
        out[(uint64_t)r * T] = own[r];
        if (r <= d) out[(uint64_t)(M + r) * T] = fe_zero();
    }
    for (int lvl = 0; lvl < depth; ++lvl) {
        const unsigned bit = (unsigned)((index >> lvl) & 1);
        const uint64_t t0 = (uint64_t)lvl * (rounds + 1);
        Fe reached[M];
        for (int r = 0; r < M; ++r) reached[r] = own[rm_trace_element(r, d)];                // the exchange
        for (int r = 0; r < M; ++r) {
            const int e = rm_trace_element(r, d);
            const Fe sib = r < 2 * d ? rp_reduce(path[(uint64_t)lvl * d + e]) : fe_zero();
            const Fe x = rm_trace_first(reached[r], sib, r, d, bit);
            out[(uint64_t)r * T + t0 + 1] = x;
            if (r < d) rm_trace_fill(out + (uint64_t)(M + r) * T, t0 + 1, rounds + 1, sib);
            if (r == d) rm_trace_fill(out + (uint64_t)(M + r) * T, t0 + 1, rounds + 1, Fe{bit, 0});
            s[r] = to_mont(x);
        }
        for (int rd = 0; rd < rounds; ++rd) {
            for (int h = 0; h < 2; ++h) {
                Fe pw[M];                                                                 // the exchange
                for (int r = 0; r < M; ++r) pw[r] = rm_split_power(s[r], h != 0);
                for (int r = 0; r < M; ++r) {
                    Fe row[M];
                    for (int j = 0; j < M; ++j) row[j] = C[r * M + j];
                    s[r] = rm_split_mix<M>(row, C[rm_split_constant(M, rd, h, r)], pw);
                }
            }
            for (int r = 0; r < M; ++r) {
                own[r] = from_mont(s[r]);
                out[(uint64_t)r * T + t0 + 2 + rd] = own[r];
            }
        }
    }
}

template <int M>
static void trace(bool split, const Fe* C, int rounds, int d, const Fe* leaves, const uint64_t* idx, const Fe* paths, uint64_t k, int depth, Fe* out) {
    const uint64_t T = rm_trace_rows(depth, rounds), W = M + d + 1;
    for (uint64_t t = 0; t < k; ++t) {
        if (split) split_trace<M>(C, rounds, d, leaves + t * d, idx[t], paths + t * depth * d, depth, out + W * T * t, T);
        else rm_path_trace_w<M>(C, rounds, d, leaves + t * d, idx[t], paths + t * depth * d, depth, out + W * T * t, T);
    }
}

extern "C" int emu_rm_path_trace(int m, const void* leaves, const uint64_t* idx, const void* paths, uint64_t k, int depth, int d, int rate,
                                 const void* params, int rounds, void* out, int split) {
    if (m < 4 || m > RP_MAX_M || rate < 2 || rate >= m || d < 1 || 2 * d >= rate || rounds < 1 || rounds > RP_MAX_ROUNDS || depth < 1 || depth > 63) return -1;
    for (uint64_t t = 0; t < k; ++t) if (idx[t] >> depth) return -1;
    const std::vector<Fe> C = load(params, m, rounds);
    switch (m) {
        case 4: trace<4>(split != 0, C.data(), rounds, d, (const Fe*)leaves, idx, (const Fe*)paths, k, depth, (Fe*)out); break;
        case 5: trace<5>(split != 0, C.data(), rounds, d, (const Fe*)leaves, idx, (const Fe*)paths, k, depth, (Fe*)out); break;
        case 6: trace<6>(split != 0, C.data(), rounds, d, (const Fe*)leaves, idx, (const Fe*)paths, k, depth, (Fe*)out); break;
        case 7: trace<7>(split != 0, C.data(), rounds, d, (const Fe*)leaves, idx, (const Fe*)paths, k, depth, (Fe*)out); break;
        default: trace<8>(split != 0, C.data(), rounds, d, (const Fe*)leaves, idx, (const Fe*)paths, k, depth, (Fe*)out); break;
    }
    return 0;
}

#ifdef RESCUE_MEMBERSHIP_MAIN
// Every width 4 .. 8 with the longest digest it takes, on heap buffers of exactly the size the layout promises (a sanitizer build
// reports any access past them): both forms write the same trace, every element of it is written, row 0 and the side columns hold what
// the layout says, and the last row is where a second walk from the same inputs ends.
int main() {
    const int rounds = 2, depth = 3;
    for (int m = 4; m <= RP_MAX_M; ++m) {
        const int rate = m - 1, d = (rate - 1) / 2;
        const uint64_t k = 3, T = rm_trace_rows(depth, rounds), W = m + d + 1;
        std::vector<Fe> params(m * m + 2 * m * rounds);
        for (size_t i = 0; i < params.size(); ++i) params[i] = Fe{0x9E3779B97F4A7C15ull * (i + 1), (0x1234567ull * (i + m)) << 20};   // far below p
        std::vector<Fe> leaves(k * d), paths(k * depth * d);
        for (size_t i = 0; i < leaves.size(); ++i) leaves[i] = Fe{i * 7 + 1, ~0ull - (i << 8)};                // words above p among them
        for (size_t i = 0; i < paths.size(); ++i) paths[i] = Fe{i * 13 + 5, i % 3 ? (uint64_t)i << 40 : ~0ull};
        std::vector<uint64_t> idx = {0, 7, 5};
        const Fe mark{0x5A5A5A5A5A5A5A5Aull, 0x5A5A5A5A5A5A5A5Aull};                                            // above p: no residue
        std::vector<Fe> wide(k * W * T, mark), split(k * W * T, mark);
        if (emu_rm_path_trace(m, leaves.data(), idx.data(), paths.data(), k, depth, d, rate, params.data(), rounds, wide.data(), 0)) return 1;
        if (emu_rm_path_trace(m, leaves.data(), idx.data(), paths.data(), k, depth, d, rate, params.data(), rounds, split.data(), 1)) return 1;
        if (memcmp(wide.data(), split.data(), wide.size() * sizeof(Fe))) return printf("m = %d: the forms differ\n", m), 2;
        for (size_t i = 0; i < wide.size(); ++i)
            if (fe_ge_p(wide[i])) return printf("m = %d: element %d is no canonical residue (or was never written)\n", m, (int)i), 3;
        for (uint64_t t = 0; t < k; ++t) {
            const Fe* item = wide.data() + W * T * t;
            for (uint64_t s = 0; s < W; ++s)
                if (!fe_eq(item[s * T], s < (uint64_t)d ? rp_reduce(leaves[t * d + s]) : fe_zero())) return printf("m = %d: row 0\n", m), 4;
            for (int lvl = 0; lvl < depth; ++lvl)
                for (int i = 0; i <= rounds; ++i) {
                    const uint64_t row = 1 + (uint64_t)lvl * (rounds + 1) + i;
                    for (int e = 0; e < d; ++e)
                        if (!fe_eq(item[(m + e) * T + row], rp_reduce(paths[(t * depth + lvl) * d + e]))) return printf("m = %d: a sibling column\n", m), 5;
                    if (!fe_eq(item[(uint64_t)(m + d) * T + row], Fe{(idx[t] >> lvl) & 1, 0})) return printf("m = %d: the bit column\n", m), 6;
                }
        }
        if (emu_rm_path_trace(m, leaves.data(), idx.data(), paths.data(), k, 64, d, rate, params.data(), rounds, wide.data(), 0) != -1) return 7;
    }
    printf("rescue membership ok\n");
    return 0;
}
#endif

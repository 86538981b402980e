// CPU build of the Rescue-Prime Merkle tree's lane functions: the SAME code the HIP kernels run (csrc/rescue_merkle.cuh), compiled by
// g++ with the portable field arithmetic, one node after the other.  The wide form is rm_sponge_w with each of its sources; the split
// form is its per-lane pieces (rm_split_absorb, rm_split_power, rm_split_mix, rm_split_constant) run lane by lane, the exchange --
// a shuffle on the device -- being a plain array here.  Test infrastructure (built by tests/test_rescue_merkle_cpu.py; with
// RESCUE_MERKLE_MAIN a stand-alone program that the same test builds with -fsanitize=address,undefined).
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

// the split form of one node: M lanes in lockstep
template <int M, class Src>
static void split_sponge(const Fe* C, int rounds, const Src& src, uint64_t len, int rate, Fe (&s)[M]) {
    for (int r = 0; r < M; ++r) s[r] = fe_zero();
    const uint64_t blocks = len / (uint64_t)rate + 1;
    for (uint64_t b = 0; b < blocks; ++b) {
        for (int r = 0; r < M; ++r) {
            const uint64_t i = b * (uint64_t)rate + r;
            const bool in_rate = r < rate;
            s[r] = rm_split_absorb(s[r], in_rate && i < len ? src(i) : fe_zero(), i, len, in_rate);
        }
        for (int rd = 0; rd < rounds; ++rd)
            for (int h = 0; h < 2; ++h) {
                Fe pw[M];                                           // the exchange
                for (int r = 0; r < M; ++r) pw[r] = rm_split_power(s[r], h != 0);
                for (int r = 0; r < M; ++r) {
                    Fe row[M];
                    for (int j = 0; j < M; ++j) row[j] = C[r * M + j];
                    s[r] = rm_split_mix<M>(row, C[rm_split_constant(M, rd, h, r)], pw);
                }
            }
    }
}

template <int M, class Src>
static void sponge(bool split, const Fe* C, int rounds, const Src& src, uint64_t len, int rate, Fe (&s)[M]) {
    if (split) split_sponge<M>(C, rounds, src, len, rate, s);
    else rm_sponge_w<M>(C, rounds, src, len, rate, s);
}

static uint64_t level_offset(uint64_t N, int d, int level) { return (uint64_t)d * (2 * N - 2 * (N >> level)); }

// levels: d * (2 N - 1) elements, level j at level_offset, element e of node k at e * (N >> j) + k
template <int M>
static void build(bool split, const Fe* C, int rounds, const Fe* rows, uint64_t ld, uint64_t width, uint64_t N, int d, int rate, Fe* levels) {
    for (int j = 0; (N >> j) >= 1; ++j) {
        const uint64_t n = N >> j;
        Fe* out = levels + level_offset(N, d, j);
        const Fe* below = j ? levels + level_offset(N, d, j - 1) : nullptr;
        for (uint64_t k = 0; k < n; ++k) {
            Fe s[M];
            if (j == 0) sponge<M>(split, C, rounds, RmLeafSrc{rows + k, ld}, width, rate, s);
            else sponge<M>(split, C, rounds, RmNodeSrc{below + 2 * k, 2 * n, d}, 2 * (uint64_t)d, rate, s);
            for (int e = 0; e < d; ++e) out[(uint64_t)e * n + k] = from_mont(s[e]);
        }
    }
}

template <int M>
static void verify(bool split, const Fe* C, int rounds, const Fe* roots, const uint64_t* idx, const Fe* paths, const Fe* rows, uint64_t k,
                   int depth, uint64_t width, int d, int rate, uint8_t* verdicts) {
    std::vector<Fe> pair(2 * k * d);             // the wide form's buffer: element i of item t's next message at i * k + t
    for (uint64_t t = 0; t < k; ++t) {
        const Fe* row = rows + t * width;
        const Fe* path = paths + t * depth * d;
        if (!split) {
            verdicts[t] = rm_verify_w<M>(C, rounds, rate, d, row, width, idx[t], path, depth, roots + t * d, pair.data() + t, k);
            continue;
        }
        // the split form: the digest stays with the lanes (own[]); a lane that absorbs element e of it gets it through the exchange
        Fe own[M];
        for (int lvl = -1; lvl < depth; ++lvl) {
            const unsigned bit = lvl < 0 ? 0 : (unsigned)((idx[t] >> lvl) & 1);
            const Fe* sibs = path + (lvl < 0 ? 0 : lvl) * (uint64_t)d;
            auto word = [&](uint64_t i) {
                if (lvl < 0) return row[i];
                const uint64_t child = i >= (uint64_t)d, e = i - child * d;
                return child == bit ? own[e] : sibs[e];
            };
            Fe s[M];
            split_sponge<M>(C, rounds, word, lvl < 0 ? width : 2 * (uint64_t)d, rate, s);
            for (int e = 0; e < d; ++e) own[e] = from_mont(s[e]);
        }
        bool ok = true;
        for (int e = 0; e < d; ++e) ok = ok && fe_eq(own[e], rp_reduce(roots[t * d + e]));
        verdicts[t] = ok;
    }
}

static bool shape_ok(int m, int rate, int d, int rounds) {
    return m >= 2 && m <= RP_MAX_M && rate >= 2 && rate < m && d >= 1 && d <= rate && rounds >= 1 && rounds <= RP_MAX_ROUNDS;
}

#define DISPATCH(m, call, ...)                      \
    switch (m) {                                \
        case 3: call<3>(__VA_ARGS__); break;                 \
        case 4: call<4>(__VA_ARGS__); break;                 \
        case 5: call<5>(__VA_ARGS__); break;                 \
        case 6: call<6>(__VA_ARGS__); break;                 \
        case 7: call<7>(__VA_ARGS__); break;                 \
        default: call<8>(__VA_ARGS__); break;                \
    }

extern "C" {
int emu_rm_build(int m, const void* rows, uint64_t ld, uint64_t width, uint64_t N, int d, int rate, const void* params, int rounds, void* levels, int split) {
    if (!shape_ok(m, rate, d, rounds) || !N || (N & (N - 1)) || ld < N || !width) return -1;
    const std::vector<Fe> C = load(params, m, rounds);
    DISPATCH(m, build, split != 0, C.data(), rounds, (const Fe*)rows, ld, width, N, d, rate, (Fe*)levels);
    return 0;
}
int emu_rm_verify(int m, const void* roots, const uint64_t* idx, const void* paths, const void* rows, uint64_t k, int depth, uint64_t width, int d,
                  int rate, const void* params, int rounds, uint8_t* verdicts, int split) {
    if (!shape_ok(m, rate, d, rounds) || depth < 0 || depth > 63 || !width) return -1;
    const std::vector<Fe> C = load(params, m, rounds);
    DISPATCH(m, verify, split != 0, C.data(), rounds, (const Fe*)roots, idx, (const Fe*)paths, (const Fe*)rows, k, depth, width, d, rate, verdicts);
    return 0;
}
}

#ifdef RESCUE_MERKLE_MAIN
// Every width 3 .. 8 and the long digests on heap buffers of exactly the size the layout promises (a sanitizer build reports any access past them):
// a strided matrix, both forms build the same tree, every leaf's path verifies in both forms and no longer does with one word changed.
int main() {
    const int rounds = 2;
    // {m, d} at capacity 1: every width at d = 1 or 2, then the long digests (tests/rescue_merkle_cases.py LONG_SHAPES: node messages
    // whose right child lies across two blocks, and d = rate)
    const int shapes[][2] = {{3, 1}, {4, 1}, {5, 2}, {6, 2}, {7, 2}, {8, 2}, {8, 4}, {5, 3}, {7, 5}, {6, 4}, {8, 7}, {3, 2}};
    for (const auto& shape : shapes) {
        const int m = shape[0], rate = m - 1, d = shape[1];
        const uint64_t N = 8, ld = N + 3, width = rate + 1;
        const int depth = 3;
        std::vector<Fe> params(m * m + 2 * m * rounds);
        for (size_t i = 0; i < params.size(); ++i) params[i] = Fe{0x9E3779B97F4A7C15ull * (i + 1), (0x1234567ull * (i + m)) << 20};   // far below p
        std::vector<Fe> rows((width - 1) * ld + N);
        for (size_t i = 0; i < rows.size(); ++i) rows[i] = Fe{i * 7 + 1, ~0ull - (i << 8)};                    // words above p among them
        std::vector<Fe> wide(d * (2 * N - 1)), split(wide.size());
        if (emu_rm_build(m, rows.data(), ld, width, N, d, rate, params.data(), rounds, wide.data(), 0)) return 1;
        if (emu_rm_build(m, rows.data(), ld, width, N, d, rate, params.data(), rounds, split.data(), 1)) return 1;
        if (memcmp(wide.data(), split.data(), wide.size() * sizeof(Fe))) return printf("m = %d d = %d: the forms differ\n", m, d), 2;
        std::vector<Fe> roots(N * d), paths(N * depth * d), items(N * width);
        std::vector<uint64_t> idx(N);
        for (uint64_t t = 0; t < N; ++t) {
            idx[t] = t;
            for (int e = 0; e < d; ++e) roots[t * d + e] = wide[level_offset(N, d, depth) + e];
            for (uint64_t c = 0; c < width; ++c) items[t * width + c] = rows[c * ld + t];
            for (int j = 0; j < depth; ++j)
                for (int e = 0; e < d; ++e) paths[(t * depth + j) * d + e] = wide[level_offset(N, d, j) + e * (N >> j) + ((t >> j) ^ 1)];
        }
        for (int form = 0; form < 2; ++form) {
            std::vector<uint8_t> verdicts(N, 7);
            if (emu_rm_verify(m, roots.data(), idx.data(), paths.data(), items.data(), N, depth, width, d, rate, params.data(), rounds, verdicts.data(), form)) return 1;
            for (uint64_t t = 0; t < N; ++t)
                if (verdicts[t] != 1) return printf("m = %d d = %d form %d: path %d does not verify\n", m, d, form, (int)t), 3;
            std::vector<Fe> bad = paths;
            bad[(3 * depth + 1) * d].lo ^= 1;
            emu_rm_verify(m, roots.data(), idx.data(), bad.data(), items.data(), N, depth, width, d, rate, params.data(), rounds, verdicts.data(), form);
            for (uint64_t t = 0; t < N; ++t)
                if (verdicts[t] != (t != 3)) return printf("m = %d d = %d form %d: a changed path\n", m, d, form), 4;
            // depth 0: the leaf digest against the root
            std::vector<Fe> leaf_roots(N * d);
            for (uint64_t t = 0; t < N; ++t)
                for (int e = 0; e < d; ++e) leaf_roots[t * d + e] = wide[e * N + t];
            std::vector<uint64_t> zeros(N, 0);
            emu_rm_verify(m, leaf_roots.data(), zeros.data(), nullptr, items.data(), N, 0, width, d, rate, params.data(), rounds, verdicts.data(), form);
            for (uint64_t t = 0; t < N; ++t)
                if (verdicts[t] != 1) return printf("m = %d d = %d form %d: depth 0\n", m, d, form), 5;
        }
    }
    printf("rescue merkle ok\n");
    return 0;
}
#endif

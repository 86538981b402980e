// CPU walk of the randomized-trace-matrix kernel: the SAME per-thread body the HIP kernel runs (randomized_cols_thread of
// csrc/columns.cuh), compiled by g++ with the portable field arithmetic and called once per (workgroup, thread) of the grid the
// library would launch.  Test infrastructure (built by tests/test_randomize_emu.py).
#include <cstdint>
#include "../../stark-anatomy_amd/csrc/columns.cuh"

using namespace sc;

extern "C" {

// randomized_cols_kernel over its whole grid: (position blocks) x (columns), 256 threads each; `draws` as the kernel reads them
// (any stride from one member's block to the next)
void emu_randomized_cols(const void* trace, uint64_t rows, uint64_t ld_trace, uint64_t members, uint64_t registers, const void* draws, uint64_t draws_stride,
                         uint64_t extra, uint32_t width, void* out, uint64_t ld_out) {
    const uint64_t cols = members * registers, gx = (rows + extra + COLS_WG - 1) / COLS_WG;
    // two launches when there is more than one column, as the entry splits a batch of more than 65 535: the second starts at col0
    const uint64_t first = cols > 1 ? cols / 2 : cols;
    for (uint64_t col0 = 0; col0 < cols; col0 += first) {
        const uint64_t k = cols - col0 < first ? cols - col0 : first;
        const RandomizedCols D{(const Fe*)trace, rows, ld_trace, registers, (const uint8_t*)draws, draws_stride, extra, width, (Fe*)out, ld_out, col0};
        for (uint64_t y = 0; y < k; ++y)
            for (uint64_t x = 0; x < gx; ++x)
                for (uint32_t t = 0; t < COLS_WG; ++t) randomized_cols_thread(D, (uint32_t)x, (uint32_t)y, t);
    }
}

// fe_sample_bytes alone: Field.sample of one byte string
void emu_sample_bytes(const void* bytes, uint32_t width, void* out) { *(Fe*)out = fe_sample_bytes((const uint8_t*)bytes, width); }
}

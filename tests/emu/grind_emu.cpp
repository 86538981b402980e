// CPU build of the grinding kernel's lane function: the SAME code the HIP kernel runs (csrc/grind.cuh: grind_pow_value, both the loop
// and the unrolled instantiation, and grind_accepts), compiled by g++, one trial after the other.  Test infrastructure (built by
// tests/test_grind_cpu.py; with GRIND_EMU_MAIN a stand-alone program that the same test builds with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../stark-anatomy_amd/csrc/grind.cuh"
#include "../../stark-anatomy_amd/csrc/transcript.h"

extern "C" {
// values_out[i] = pow_value(seeds[32 i ..], nonces[i])
void emu_grind_values(const uint8_t* seeds, const uint64_t* nonces, uint64_t count, int unrolled, uint64_t* values_out) {
    for (uint64_t i = 0; i < count; ++i) {
        uint64_t s[4];
        memcpy(s, seeds + 32 * i, 32);
        values_out[i] = unrolled ? sc::grind_pow_value<true>(s[0], s[1], s[2], s[3], nonces[i]) : sc::grind_pow_value<false>(s[0], s[1], s[2], s[3], nonces[i]);
    }
}
int emu_grind_accepts(uint64_t value, int bits) { return sc::grind_accepts(value, bits); }
// one window as the kernel walks it: the smallest accepted offset in [base, base + window) from `start`, ~0 when there is none
uint64_t emu_grind_window(const uint8_t* seed, uint64_t start, uint64_t base, uint64_t window, int bits) {
    uint64_t s[4], best = sc::GRIND_NONE;
    memcpy(s, seed, 32);
    for (uint64_t w = 0; w < window; ++w) {
        const uint64_t o = base + w;
        if (o > best) break;
        if (sc::grind_accepts(sc::grind_pow_value<false>(s[0], s[1], s[2], s[3], start + o), bits) && o < best) best = o;
    }
    return best;
}
}

#ifdef GRIND_EMU_MAIN
// the lane function against the sponge of csrc/transcript.h (itself compared with hashlib by tests/test_host_cpu.py) on nonces around the carry
int main() {
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(i * 37 + 11);
    const uint64_t nonces[] = {0, 1, 0xFFFFFFFFull, 0x100000000ull, 0x123456789ABCDEFull, ~0ull - 1, ~0ull};
    for (uint64_t nonce : nonces) {
        uint8_t msg[40], out[8];
        memcpy(msg, seed, 32);
        memcpy(msg + 32, &nonce, 8);
        sc::shake256(msg, 40, out, 8);
        uint64_t expect, got[2];
        memcpy(&expect, out, 8);
        emu_grind_values(seed, &nonce, 1, 0, got);
        emu_grind_values(seed, &nonce, 1, 1, got + 1);
        if (got[0] != expect || got[1] != expect) return printf("nonce %llx: the lane function differs from the sponge\n", (unsigned long long)nonce), 1;
    }
    if (emu_grind_window(seed, ~0ull - 299, 0, 300, 4) == sc::GRIND_NONE) return printf("no accepted nonce in the last 300 at 4 bits\n"), 2;
    printf("grind ok\n");
    return 0;
}
#endif

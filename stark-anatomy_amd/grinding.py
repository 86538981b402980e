"""Proof-of-work grinding on the Fiat-Shamir transcript.

Before the query indices of a FRI proof are sampled the prover finds a nonce whose hash with the transcript seed has `bits` leading
zero bits, and pushes it onto the stream; the indices then depend on it.  An adversary who retries Fiat-Shamir pays 2^bits hashes per
retry, which buys `bits` bits of soundness and lets the proof carry fewer colinearity tests (fast_stark.FastStark: 2 * checks + bits
>= security level).

The specification (the library's kernel, csrc/grind.cuh, computes exactly this):

    pow_value(seed, nonce) = int.from_bytes(shake_256(seed + nonce.to_bytes(8, "little")).digest(8), "little")     0 <= nonce < 2^64
    accepts(seed, nonce, bits)  iff  pow_value(seed, nonce) >> (64 - bits) == 0                                    1 <= bits <= 63

`seed` is 32 bytes (a prover_fiat_shamir() digest).  The prover takes the SMALLEST accepted nonce, so a proof is reproducible byte for
byte whichever route computes it.  The 40-byte message fits SHAKE-256's rate: one trial is one Keccak-f[1600].

MAX_BITS = 40 is what the constructors (Fri, FastStark) take at most: a search needs 2^bits trials on average, and at the library's
rate of a few 10^9 trials per second 2^40 trials are minutes per proof; nothing beyond that is a sensible parameter.
"""
import ctypes
from hashlib import shake_256

import starkcore as _sc

MAX_BITS = 40
NONCE_LIMIT = 1 << 64


def pow_value(seed, nonce):
    assert(type(nonce) is int and 0 <= nonce < NONCE_LIMIT), "a nonce is an integer below 2^64"
    return int.from_bytes(shake_256(bytes(seed) + nonce.to_bytes(8, "little")).digest(8), "little")


def accepts_value(value, bits):
    assert(1 <= bits <= 63), "1 .. 63 bits"
    return value >> (64 - bits) == 0


def accepts(seed, nonce, bits):
    return accepts_value(pow_value(seed, nonce), bits)


def check(seed, nonce, bits):
    """the verifier's test of a nonce pulled from a proof stream: a plain int below 2^64 that is accepted"""
    return type(nonce) is int and 0 <= nonce < NONCE_LIMIT and accepts(seed, nonce, bits)


def _range(seed, bits, start, max_nonces):
    assert(len(seed) == 32), "a seed is 32 bytes"
    assert(1 <= bits <= 63), "1 .. 63 bits"
    assert(0 <= start < NONCE_LIMIT), "start below 2^64"
    if max_nonces is None:
        max_nonces = min(NONCE_LIMIT - start, NONCE_LIMIT - 1)
    assert(0 <= max_nonces and start + max_nonces <= NONCE_LIMIT), "the range passes 2^64"
    return max_nonces


def grind_host(seed, bits, start=0, max_nonces=None):
    """the smallest accepted nonce in [start, start + max_nonces), None when there is none -- the hashlib loop (a microsecond per trial:
    for tests)"""
    for nonce in range(start, start + _range(seed, bits, start, max_nonces)):
        if accepts(seed, nonce, bits):
            return nonce
    return None


def grind(seed, bits, start=0, max_nonces=None, stream=None):
    """the same search on the GPU (sc_grind): windows of trials in ascending order, one lane per trial"""
    max_nonces = _range(seed, bits, start, max_nonces)
    nonce, found = ctypes.c_uint64(0), ctypes.c_int(0)
    _sc._check(_sc.lib().sc_grind(bytes(seed), bits, start, max_nonces, ctypes.byref(nonce), ctypes.byref(found), stream))
    return int(nonce.value) if found.value else None


def grind_library_host(seed, bits, start=0, max_nonces=None):
    """the same search on one host core in the library (sc_grind_host): the baseline of the measurements"""
    max_nonces = _range(seed, bits, start, max_nonces)
    nonce, found = ctypes.c_uint64(0), ctypes.c_int(0)
    _sc._check(_sc.lib().sc_grind_host(bytes(seed), bits, start, max_nonces, ctypes.byref(nonce), ctypes.byref(found)))
    return int(nonce.value) if found.value else None


def grind_batch(seeds, bits, start=0, max_nonces=None, stream=None):
    """[grind(seed, bits, start, max_nonces) for seed in seeds] in shared launches (sc_grind_batch): the members ride one grid and a
    member that has its nonce does no more work"""
    seeds = [bytes(seed) for seed in seeds]
    if not seeds:
        return []
    max_nonces = max(_range(seed, bits, start, max_nonces) for seed in seeds)
    count = len(seeds)
    nonces, found = (ctypes.c_uint64 * count)(), (ctypes.c_uint8 * count)()
    _sc._check(_sc.lib().sc_grind_batch(b"".join(seeds), count, bits, start, max_nonces, nonces, found, stream))
    return [int(nonces[m]) if found[m] else None for m in range(count)]

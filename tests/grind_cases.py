"""Cases of the proof-of-work search (grinding.py, csrc/grind.cuh), shared by tests/test_grind_cpu.py (which derives every expectation
with hashlib) and tests/test_gpu_grind.py / tests/test_gpu_grind_scale.py (which run the kernel on them).  Plain hashlib here: no
library, no GPU.

Where the recorded values come from:
  CASES      hashlib loops from `start`; the two 20-bit ones are long (4 037 874 trials), so test_grind_cpu.py walks them with hashlib
             over the last 2^16 nonces only and from zero with sc_grind_host, which it holds to the recorded constant.
  DEEP_CPU   the smallest accepted nonce FROM ZERO at 22, 23 and 24 bits, found once by the hashlib loop of `smallest` (2 to 7 million
             trials each, seconds) and recorded.  test_grind_cpu.py proves value and nonce with hashlib over the last 2^16 nonces and
             has sc_grind_host repeat the whole search from zero.
  DEEP_GPU   nonces whose value has 33 or more leading zero bits: 2^33 trials and more, out of any CPU loop's reach.  They were found
             once with grinding.grind(seed, bits) on an MI355X (bits = 33, 34, 36, 33 in the order below) and are recorded with the
             value HASHLIB gives at them.  As far as any CPU check goes they are minimal ONLY over the last 2^16 nonces in front of
             them (test_grind_cpu.py walks that stretch with hashlib); that they are minimal from zero is what the search that found
             them claims and nothing here verifies, so no test may assert more than: accepted at the nonce, nothing accepted in the
             2^16 in front of it.
  QUIET      a seed whose values over the nonces [0, 2^16) have at most 16 leading zero bits (test_grind_cpu.py: none has 28).
  batch_members   seeds seed_of(base + k) with the minima `smallest` finds -- hashlib, computed when asked for and kept."""
import functools
from hashlib import shake_256


def pow_value(seed, nonce):
    return int.from_bytes(shake_256(seed + nonce.to_bytes(8, "little")).digest(8), "little")


def accepted(seed, nonce, bits):
    return pow_value(seed, nonce) >> (64 - bits) == 0


def smallest(seed, bits, start=0, limit=1 << 23):
    """the smallest accepted nonce in [start, start + limit), None when there is none"""
    for nonce in range(start, start + limit):
        if accepted(seed, nonce, bits):
            return nonce
    return None


# (seed, bits, start, the smallest accepted nonce from start on) -- computed with hashlib; test_grind_cpu.py recomputes the cheap
# ones in full, checks the two long ones at the nonce and over the last stretch in front of it, and has sc_grind_host walk them from zero
CASES = [
    (b"\x00" * 32, 16, 0, 40591),
    (b"\x00" * 32, 20, 0, 40591),
    (b"\x01" * 32, 16, 0, 269517),
    (b"\x01" * 32, 20, 0, 4037874),
    (b"\x01" * 32, 12, (1 << 32) - 1000, 4294966442),           # below 2^32
    (b"\x02" * 32, 12, (1 << 32) - 1000, 4294969125),           # across the carry into the high word
]

# windows the GPU tests set "grind_window" to: two multiples of the wave, one that is not
WINDOWS = [(64, 6), (256, 8), (100, 7)]                         # (window, bits: a minimum lies about one window in)


def seed_of(k):
    return shake_256(b"grind case %d" % k).digest(32)


@functools.lru_cache(maxsize=None)
def placements(window, bits):
    """{place: (seed, minimum)} for a window size: seeds whose smallest accepted nonce (from 0) falls
      last    on the last nonce of a window
      first   on the first nonce of a window that is not window 0
      far     three or more windows on
      two     in a window that holds a second accepted nonce behind it (the smaller must win)
    found by trying seeds seed_of(0), seed_of(1), ...: a few hundred seeds of about 2^bits trials each"""
    found = {}
    for k in range(100000):
        seed = seed_of(k)
        low = smallest(seed, bits)
        if low % window == window - 1:
            found.setdefault("last", (seed, low))
        if low % window == 0 and low >= window:
            found.setdefault("first", (seed, low))
        if low >= 3 * window:
            found.setdefault("far", (seed, low))
        if "two" not in found and any(accepted(seed, nonce, bits) for nonce in range(low + 1, (low // window + 1) * window)):
            found["two"] = (seed, low)
        if len(found) == 4:
            return found
    raise AssertionError("no seeds for window %d" % window)


def batch_seeds(count):
    """seeds for sc_grind_batch at 8 bits: the first has its minimum at a tiny nonce, one is a duplicate of another (count >= 3),
    the rest fall where they fall -- in different windows of 64"""
    tiny = next(seed_of(k) for k in range(1000, 100000) if smallest(seed_of(k), 8) < 4)
    seeds = [tiny] + [seed_of(2000 + k) for k in range(count - 1)]
    if count >= 3:
        seeds[-1] = seeds[1]
    return seeds


def leading_zeros(value):
    return 64 - value.bit_length()


# (seed, nonce, pow_value(seed, nonce)) -- see the module's docstring for where each group comes from and what is proved of it
DEEP_CPU = [
    (b"\x03" * 32, 1665965, 0x2195D18A915),                     # 22 leading zero bits; the smallest from 0 at 22 bits
    (b"\x06" * 32, 1565676, 0x12BF9647DCD),                     # 23
    (b"\x05" * 32, 6570675, 0xCD1EBE10E5),                      # 24
]
DEEP_GPU = [
    (b"\x08" * 32, 8414119693, 0x77968429),                     # 33 leading zero bits; every nonce lies above 2^32
    (b"\x09" * 32, 4495174319, 0x38EC11FB),                     # 34
    (b"\x0a" * 32, 22509517392, 0xD7509F0),                     # 36
    (b"\x0b" * 32, 12585378260, 0x21BB918B),                    # 34 (searched at 33)
]
DEEP = DEEP_CPU + DEEP_GPU
STRETCH = 1 << 16                                               # the nonces in front of a DEEP nonce that hashlib walks

# a seed and a range in which nothing has 28 or more leading zero bits; its minima at 1, 2 and 3 bits are 2, 7 and 22
QUIET = (b"\x0f" * 32, 1 << 16)


@functools.lru_cache(maxsize=None)
def batch_members(count, bits, base):
    """(seeds, minima): seed_of(base + k) for k < count and the smallest accepted nonce from 0 of each.  600 members at 10 bits
    take about 0.7 s (at base 30000: minima up to 6828, in 18 different windows of 256), 65535 members at 3 bits as long (at base
    100000: the largest minimum is 85)."""
    seeds = tuple(seed_of(base + k) for k in range(count))
    return seeds, tuple(smallest(seed, bits) for seed in seeds)

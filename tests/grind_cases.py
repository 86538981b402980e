"""Cases of the proof-of-work search (grinding.py, csrc/grind.cuh), shared by tests/test_grind_cpu.py (which derives every expectation
with hashlib) and tests/test_gpu_grind.py (which runs the kernel on them).  Plain hashlib here: no library, no GPU."""
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
# ones in full and checks the two long ones at the nonce and over the last stretch in front of it
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

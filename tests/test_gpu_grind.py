"""The proof-of-work search on the GPU (sc_grind, sc_grind_batch; csrc/grind.cuh, csrc/grind.hip) against the hashlib loop: the cases of
tests/grind_cases.py, minima placed at the edges of small windows, ranges that end one short of a minimum or at the top of the 64-bit
range, batches whose members finish in different windows, two searches in flight on two streams, and outputs between sentinels."""
import ctypes
import threading

import pytest

import grind_cases as gc

pytestmark = pytest.mark.gpu

NONE = 0xA5A5A5A5A5A5A5A5         # what an output word holds before a call


@pytest.fixture(scope="module")
def sc():
    import starkcore
    assert starkcore.device_count() > 0, "no GPU visible: the HIP path is mandatory for these tests"
    starkcore.init()
    return starkcore


@pytest.fixture(scope="module")
def grinding(sc):
    import grinding
    return grinding


@pytest.fixture()
def window(sc):
    """sets "grind_window" for a test and puts the default back"""
    yield lambda value: sc.set_tuning("grind_window", value)
    sc.set_tuning("grind_window", -1)
    sc.set_tuning("grind_unrolled", 0)


def test_cases(sc, grinding, window):
    """every case equals the expectation that test_grind_cpu.py derives with hashlib; the case at 4037874 runs many full windows of the
    default size (the first hit is in a window that is not the first) -- and all of them with the unrolled kernel as well"""
    for unrolled in (0, 1):
        sc.set_tuning("grind_unrolled", unrolled)
        for seed, bits, start, expected in gc.CASES:
            assert grinding.grind(seed, bits, start) == expected
    sc.set_tuning("grind_unrolled", 0)
    window(1 << 16)                                    # 61 full windows in front of the hit
    assert grinding.grind(b"\x01" * 32, 20) == 4037874


@pytest.mark.parametrize("size,bits", gc.WINDOWS)
def test_minimum_at_the_edges_of_small_windows(sc, grinding, window, size, bits):
    window(size)
    places = gc.placements(size, bits)
    for place, (seed, low) in places.items():
        assert grinding.grind(seed, bits) == low, place
        # a range that ends one short of the minimum holds nothing; one that just reaches it holds it
        assert grinding.grind(seed, bits, 0, low) is None, place
        assert grinding.grind(seed, bits, 0, low + 1) == low, place
        # from behind the minimum on: the next accepted nonce
        assert grinding.grind(seed, bits, low + 1) == gc.smallest(seed, bits, low + 1), place
    # the same seeds as one batch: members whose minima lie in different windows
    seeds = [seed for seed, _ in places.values()]
    assert grinding.grind_batch(seeds, bits) == [low for _, low in places.values()]


def test_top_of_the_range(sc, grinding, window):
    seed = b"\x07" * 32
    start = 2 ** 64 - 300
    expected = gc.smallest(seed, 4, start, 300)
    assert expected is not None
    for size in (-1, 64, 100):
        window(size)
        assert grinding.grind(seed, 4, start) == expected              # max_nonces = 300: up to 2^64 - 1 and no further
        assert grinding.grind(seed, 4, start, 300) == expected
        assert grinding.grind(seed, 40, start) is None                 # nothing accepted up to the last nonce: no wrap to the small ones
        assert grinding.grind(seed, 40, 2 ** 64 - 1) is None           # the last nonce alone
    nonce, found = ctypes.c_uint64(NONE), ctypes.c_int(7)
    assert sc.lib().sc_grind(seed, 4, start, 301, ctypes.byref(nonce), ctypes.byref(found), None) != 0      # a range past 2^64 is refused
    assert (nonce.value, found.value) == (NONE, 7)


def _batch_raw(sc, seeds, bits, start=0, max_nonces=2 ** 64 - 1, guard=3):
    """sc_grind_batch with its outputs inside arrays of sentinels: (nonces, found, the arrays as they are afterwards)"""
    count = len(seeds)
    nonces = (ctypes.c_uint64 * (count + 2 * guard))(*[NONE] * (count + 2 * guard))
    found = (ctypes.c_uint8 * (count + 2 * guard))(*[0x5A] * (count + 2 * guard))
    sc._check(sc.lib().sc_grind_batch(b"".join(seeds), count, bits, start, max_nonces,
                                      ctypes.byref(nonces, 8 * guard), ctypes.byref(found, guard), None))
    return list(nonces), list(found)


@pytest.mark.parametrize("count", [1, 2, 17])
def test_batch(sc, grinding, window, count):
    window(64)
    seeds = gc.batch_seeds(count)
    expected = [gc.smallest(seed, 8) for seed in seeds]
    assert expected[0] < 4 and (count < 3 or (seeds[-1] == seeds[1] and len(set(e // 64 for e in expected)) > 1))
    nonces, found = _batch_raw(sc, seeds, 8)
    assert nonces == [NONE] * 3 + expected + [NONE] * 3 and found == [0x5A] * 3 + [1] * count + [0x5A] * 3
    assert [grinding.grind(seed, 8) for seed in seeds] == expected          # each result equals the single call's
    # a range that ends before some members' minima: those report nothing and their words stay as they were
    limit = sorted(expected)[count // 2] + 1
    nonces, found = _batch_raw(sc, seeds, 8, 0, limit)
    assert found[3:3 + count] == [1 if e < limit else 0 for e in expected]
    assert nonces[3:3 + count] == [e if e < limit else NONE for e in expected]
    assert nonces[:3] + nonces[3 + count:] == [NONE] * 6 and found[:3] + found[3 + count:] == [0x5A] * 6
    window(-1)
    assert grinding.grind_batch(seeds, 8) == expected                       # the default window: all in one launch


def test_empty_batch_touches_nothing(sc, grinding):
    nonces, found = _batch_raw(sc, [], 8)
    assert nonces == [NONE] * 6 and found == [0x5A] * 6
    assert sc.lib().sc_grind_batch(None, 0, 8, 0, 100, None, None, None) == 0
    assert grinding.grind_batch([], 8) == []


def test_single_call_outputs_between_sentinels(sc):
    seed, bits, start, expected = gc.CASES[0]
    nonces = (ctypes.c_uint64 * 3)(NONE, NONE, NONE)
    found = (ctypes.c_int * 3)(7, 7, 7)
    at = lambda array, size: ctypes.cast(ctypes.byref(array, size), ctypes.POINTER(array._type_))
    sc._check(sc.lib().sc_grind(seed, bits, start, 2 ** 64 - 1, at(nonces, 8), at(found, 4), None))
    assert list(nonces) == [NONE, expected, NONE] and list(found) == [7, 1, 7]
    sc._check(sc.lib().sc_grind(seed, bits, start, expected, at(nonces, 8), at(found, 4), None))       # nothing in range: the nonce stays
    assert list(nonces) == [NONE, expected, NONE] and list(found) == [7, 0, 7]
    sc._check(sc.lib().sc_grind(seed, bits, start, 0, at(nonces, 8), at(found, 4), None))
    assert list(found) == [7, 0, 7]


def test_two_searches_in_flight_on_two_streams(sc, grinding, window):
    """two host threads, each with a stream of its own, search at the same time (the library does not hold its lock while a search
    waits for the device); every result equals the single-stream one"""
    import torch
    window(256)                                        # many windows per search: the two interleave on the device
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    jobs = [[(seed, bits, low) for seed, low in gc.placements(size, bits).values()] + [(gc.CASES[0][0], 16, 40591)] for size, bits in gc.WINDOWS[:2]]
    results, errors = [None, None], []

    def run(k):
        try:
            handle = ctypes.c_void_p(streams[k].cuda_stream)
            results[k] = [grinding.grind(seed, bits, stream=handle) for seed, bits, _ in jobs[k]]
        except Exception as e:                         # noqa: BLE001  (reported below, in the test's thread)
            errors.append(e)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert results[k] == [low for _, _, low in jobs[k]]
    torch.cuda.synchronize()

"""The proof-of-work search on the GPU (sc_grind, sc_grind_batch; csrc/grind.cuh, csrc/grind.hip) where tests/test_gpu_grind.py does not
reach: every bit count from 1 to 63 on values with 22 to 36 leading zero bits (the acceptance shift across the 32-bit half, the
rotations of the device branch behind it), deep values found by search over the stretch hashlib has walked, the long searches from
zero against the library's host search, batches of more than twice as many members as the part has compute units (the floor of the
blocks per member: every lane strides through its window), the member limit and one past it, and a batch on a stream of its own while
another thread searches.  Every expectation is hashlib's (tests/grind_cases.py, proved by tests/test_grind_cpu.py) or sc_grind_host's
where that test holds it to a recorded constant; the recorded 33-bit-and-up nonces are claimed minimal over the 2^16 nonces in front
of them and no further."""
import ctypes
import threading

import pytest

import grind_cases as gc

pytestmark = pytest.mark.gpu

NONE = 0xA5A5A5A5A5A5A5A5         # what an output word holds before a call
SC_ERR_BAD_ARG = -6               # include/starkcore.h
WINDOWS = [-1, 100, 4096]         # the default (2^22), one that is no multiple of the wave, one of 16 workgroups


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
    """sets "grind_window" for a test and puts the defaults back"""
    yield lambda value: sc.set_tuning("grind_window", value)
    sc.set_tuning("grind_window", -1)
    sc.set_tuning("grind_unrolled", 0)


def _batch_raw(sc, seeds, bits, start=0, max_nonces=2 ** 64 - 1, guard=3, stream=None):
    """sc_grind_batch with its outputs inside arrays of sentinels: (the nonce words, the found bytes) as they are afterwards"""
    count = len(seeds)
    nonces = (ctypes.c_uint64 * (count + 2 * guard))(*[NONE] * (count + 2 * guard))
    found = (ctypes.c_uint8 * (count + 2 * guard))(*[0x5A] * (count + 2 * guard))
    sc._check(sc.lib().sc_grind_batch(b"".join(seeds), count, bits, start, max_nonces, ctypes.byref(nonces, 8 * guard), ctypes.byref(found, guard), stream))
    return list(nonces), list(found)


# ---- every bit count --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unrolled", [0, 1])
def test_every_bit_count_on_one_trial(sc, grinding, window, unrolled):
    """one nonce, one trial: accepted at every bit count up to the value's leading zeros and at none above -- 31, 32 and 33 lie on
    both sides of that edge among the triples"""
    sc.set_tuning("grind_unrolled", unrolled)
    for seed, nonce, value in gc.DEEP:
        z = gc.leading_zeros(value)
        got = [grinding.grind(seed, bits, nonce, 1) for bits in range(1, 64)]
        assert got == [nonce if bits <= z else None for bits in range(1, 64)], (nonce, z)


def test_every_bit_count_on_one_trial_in_a_batch(sc, window):
    """the same through sc_grind_batch: a batch has ONE start, so every DEEP nonce in turn is the single trial of all members -- the
    DEEP seeds and eight arbitrary ones, whose values there have few leading zeros and give the low thresholds both verdicts"""
    seeds = [seed for seed, _, _ in gc.DEEP] + [gc.seed_of(7000 + k) for k in range(8)]
    seen = set()
    for _, nonce, _ in gc.DEEP:
        zeros = [gc.leading_zeros(gc.pow_value(seed, nonce)) for seed in seeds]
        seen.update(zeros)
        for bits in range(1, 64):
            nonces, found = _batch_raw(sc, seeds, bits, nonce, 1)
            hit = [z >= bits for z in zeros]
            assert found == [0x5A] * 3 + [int(h) for h in hit] + [0x5A] * 3, (nonce, bits)
            assert nonces == [NONE] * 3 + [nonce if h else NONE for h in hit] + [NONE] * 3, (nonce, bits)
    assert seen >= {0, 1, 2, 3} and max(seen) >= 36


@pytest.mark.parametrize("unrolled", [0, 1])
def test_every_bit_count_on_a_quiet_range(sc, grinding, window, unrolled):
    sc.set_tuning("grind_unrolled", unrolled)
    seed, count = gc.QUIET
    for bits in (28, 31, 32, 33, 48, 63):
        assert grinding.grind(seed, bits, 0, count) is None, bits
    for bits in (1, 2, 3):
        assert grinding.grind(seed, bits, 0, count) == gc.smallest(seed, bits, 0, count), bits


@pytest.mark.parametrize("size", WINDOWS)
def test_a_deep_value_is_found_by_search(sc, grinding, window, size):
    """from 2^16 nonces in front of a DEEP nonce, at the value's own bit count: the range that reaches it finds it, the range one short
    of it finds nothing (hashlib has walked that stretch, tests/test_grind_cpu.py)"""
    window(size)
    for seed, nonce, value in gc.DEEP:
        z = gc.leading_zeros(value)
        assert grinding.grind(seed, z, nonce - gc.STRETCH, gc.STRETCH + 1) == nonce, (nonce, z)
        assert grinding.grind(seed, z, nonce - gc.STRETCH, gc.STRETCH) is None, (nonce, z)


LONG = [(seed, bits, expected) for seed, bits, start, expected in gc.CASES if bits == 20] + [(seed, gc.leading_zeros(value), nonce) for seed, nonce, value in gc.DEEP_CPU]


@pytest.mark.parametrize("case", range(len(LONG)))
def test_long_searches_from_zero_equal_the_library_host_search(sc, grinding, case):
    """the searches of 40 591 to 6 570 675 trials from nonce 0 on: the kernel, the library's host loop (an independent Keccak-f that
    tests/test_grind_cpu.py holds to hashlib and to these constants) and the recorded minimum agree"""
    seed, bits, expected = LONG[case]
    assert grinding.grind(seed, bits) == grinding.grind_library_host(seed, bits) == expected


# ---- batches at scale -------------------------------------------------------------------------------------------------------------
def _crowd(sc):
    """more than 2 * (compute units) members at 10 bits with their hashlib minima; three seeds stand a second time far from the first"""
    import torch
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    count = 2 * num_cus + 8
    assert count > 2 * num_cus and num_cus * 16 // count < 8           # grind.hip: max_blocks sits on its floor of 8
    seeds, minima = gc.batch_members(count, 10, 30000)
    seeds, minima = list(seeds), list(minima)
    for here, there in ((count - 1, 0), (count // 2, 3), (count - 7, count // 2 + 1)):
        seeds[here], minima[here] = seeds[there], minima[there]
    return seeds, minima


@pytest.mark.parametrize("size", [-1, 256])
def test_batch_above_the_block_floor(sc, grinding, window, size):
    """8 workgroups per member: at the default window a lane strides through 2^22 offsets 2048 lanes at a time (minima above 2047 are
    met only by striding); at a window of 256 the members finish in more than 16 different launches and the list of members
    shrinks from launch to launch"""
    seeds, minima = _crowd(sc)
    count = len(seeds)
    assert max(minima) > 2048 and len(set(low // 256 for low in minima)) > 16
    window(size)
    assert grinding.grind_batch(seeds, 10) == minima
    nonces, found = _batch_raw(sc, seeds, 10)
    assert nonces == [NONE] * 3 + minima + [NONE] * 3 and found == [0x5A] * 3 + [1] * count + [0x5A] * 3
    # a range that ends behind the median minimum: exactly the members at or below it are found, the others' words stay as they were
    limit = sorted(minima)[count // 2] + 1
    nonces, found = _batch_raw(sc, seeds, 10, 0, limit)
    assert 0 < sum(low < limit for low in minima) < count
    assert found == [0x5A] * 3 + [1 if low < limit else 0 for low in minima] + [0x5A] * 3
    assert nonces == [NONE] * 3 + [low if low < limit else NONE for low in minima] + [NONE] * 3


def test_the_member_limit(sc, grinding, window):
    """65535 members ride blockIdx.y of one launch"""
    seeds, minima = gc.batch_members(65535, 3, 100000)
    nonces, found = _batch_raw(sc, seeds, 3)
    assert found == [0x5A] * 3 + [1] * 65535 + [0x5A] * 3
    assert nonces == [NONE] * 3 + list(minima) + [NONE] * 3


def test_one_member_too_many_is_refused(sc):
    seeds = gc.batch_members(65535, 3, 100000)[0] + (gc.seed_of(1),)
    count = len(seeds)
    assert count == 65536
    nonces = (ctypes.c_uint64 * count)(*[NONE] * count)
    found = (ctypes.c_uint8 * count)(*[0x5A] * count)
    assert sc.lib().sc_grind_batch(b"".join(seeds), count, 3, 0, 2 ** 64 - 1, nonces, found, None) == SC_ERR_BAD_ARG
    assert "at most 65535" in sc.lib().sc_last_error().decode()
    assert set(nonces) == {NONE} and set(found) == {0x5A}


def test_a_batch_on_its_own_stream_beside_single_searches(sc, grinding, window):
    """a batch of members that finish in different windows, on a stream of the caller's, while a second host thread runs single
    searches on another stream: the batch's results are those of the batch alone (and hashlib's)"""
    import torch
    window(256)
    seeds, minima = gc.batch_members(200, 10, 30000)
    seeds, minima = list(seeds), list(minima)
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    handles = [ctypes.c_void_p(s.cuda_stream) for s in streams]
    singles = [(seed, bits, low) for size, bits in gc.WINDOWS[:2] for seed, low in gc.placements(size, bits).values()] + [(gc.CASES[0][0], 16, 40591)]
    alone = grinding.grind_batch(seeds, 10, stream=handles[0])
    assert alone == minima
    results, errors = {}, []

    def batch():
        try:
            results["batch"] = [grinding.grind_batch(seeds, 10, stream=handles[0]) for _ in range(2)]
        except Exception as e:                         # noqa: BLE001  (reported below, in the test's thread)
            errors.append(e)

    def single():
        try:
            results["single"] = [grinding.grind(seed, bits, stream=handles[1]) for seed, bits, _ in singles]
        except Exception as e:                         # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=batch), threading.Thread(target=single)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert results["batch"] == [alone, alone]
    assert results["single"] == [low for _, _, low in singles]
    torch.cuda.synchronize()

"""Proof-of-work grinding without a GPU: the host specification (grinding.py) against an independent Keccak-f[1600], the g++ build of
the kernel's lane function (csrc/grind.cuh through tests/emu/grind_emu.cpp) against hashlib, the library's host search, every recorded constant of
tests/grind_cases.py (the deep values, the quiet range, the batch members) proved with hashlib, the member limit of a batch, the
verifier's check of the nonce on transcripts built by hand, and the constructors."""
import ctypes
import os
import random
import subprocess
from hashlib import shake_256

import pytest

from conftest import REPO, PKG
import grind_cases as gc
import grinding

EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = [os.path.join(PKG, "csrc", name) for name in ("grind.cuh", "transcript.h")]


# ---- an independent Keccak-f[1600] (FIPS 202, section 3.2, written from the step mappings; lanes as a[x][y]) --------------------------
def _rol(v, n):
    n %= 64
    return ((v << n) | (v >> (64 - n))) & (2 ** 64 - 1) if n else v


def keccak_f(lanes):
    a = [[lanes[x + 5 * y] for y in range(5)] for x in range(5)]
    lfsr = 1
    for _ in range(24):
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        x, y, current = 1, 0, a[1][0]                          # rho and pi along the (x, y) -> (y, 2 x + 3 y) orbit
        for t in range(24):
            x, y = y, (2 * x + 3 * y) % 5
            current, a[x][y] = a[x][y], _rol(current, (t + 1) * (t + 2) // 2)
        a = [[a[x][y] ^ (~a[(x + 1) % 5][y] & a[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        for j in range(7):                                     # iota: the round constant's bits from the LFSR
            lfsr = ((lfsr << 1) ^ ((lfsr >> 7) * 0x71)) % 256
            if lfsr & 2:
                a[0][0] ^= 1 << ((1 << j) - 1)
    return [a[i % 5][i // 5] for i in range(25)]


def one_permutation(seed, nonce):
    """the issue's layout of one trial: words 0 .. 3 the seed, word 4 the nonce, word 5 = 0x1f, word 16 = 1 << 63; the value is word 0"""
    lanes = [int.from_bytes(seed[8 * i:8 * i + 8], "little") for i in range(4)] + [nonce, 0x1F] + [0] * 19
    lanes[16] = 1 << 63
    return keccak_f(lanes)[0]


def test_spec_is_one_permutation_of_an_independent_keccak():
    rng = random.Random(1)
    for nonce in [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1] + [rng.getrandbits(64) for _ in range(6)]:
        seed = bytes(rng.getrandbits(8) for _ in range(32))
        assert grinding.pow_value(seed, nonce) == one_permutation(seed, nonce) == gc.pow_value(seed, nonce)


def test_accepts_at_the_edges():
    for bits in (1, 63, 20):
        assert grinding.accepts_value(2 ** (64 - bits) - 1, bits) and not grinding.accepts_value(2 ** (64 - bits), bits)
        assert grinding.accepts_value(0, bits) and not grinding.accepts_value(2 ** 64 - 1, bits)
    for bits in (0, 64):
        with pytest.raises(AssertionError):
            grinding.accepts_value(0, bits)
    seed = b"\x05" * 32
    with pytest.raises(AssertionError):
        grinding.pow_value(seed, 2 ** 64)
    with pytest.raises(AssertionError):
        grinding.pow_value(seed, -1)
    assert grinding.check(seed, gc.smallest(seed, 8), 8)
    for bad in (None, b"\x00", 1.0, True, -1, 2 ** 64):        # not a plain int below 2^64
        assert not grinding.check(seed, bad, 8)


def test_cases_are_what_hashlib_says():
    """every case at its nonce; the search in full where it is short, over the last 2^16 nonces in front of the minimum where it is long"""
    for seed, bits, start, expected in gc.CASES:
        assert gc.accepted(seed, expected, bits)
        first = start if expected - start <= 1 << 17 else expected - (1 << 16)
        assert gc.smallest(seed, bits, first, expected - first + 1) == expected
    for window, bits in gc.WINDOWS:
        places = gc.placements(window, bits)
        assert places["last"][1] % window == window - 1 and places["first"][1] % window == 0 and places["first"][1] >= window
        assert places["far"][1] >= 3 * window
        for seed, low in places.values():
            assert gc.smallest(seed, bits) == low


def test_deep_cases_are_what_hashlib_says():
    """the recorded (seed, nonce, value) triples of grind_cases.DEEP: the value is hashlib's, and over the 2^16 nonces in front of the
    nonce nothing is accepted at the value's own count of leading zero bits -- for the 33-bit-and-up ones that stretch is ALL a CPU
    check proves of their being minimal (the search that found them ran on a GPU)"""
    for seed, nonce, value in gc.DEEP:
        assert gc.pow_value(seed, nonce) == value == grinding.pow_value(seed, nonce)
        z = gc.leading_zeros(value)
        assert value >> (64 - z) == 0 and value >> (63 - z) == 1
        assert gc.accepted(seed, nonce, z) and not gc.accepted(seed, nonce, z + 1)
        assert nonce > gc.STRETCH
        assert gc.smallest(seed, z, nonce - gc.STRETCH, gc.STRETCH + 1) == nonce
    assert [gc.leading_zeros(value) for _, _, value in gc.DEEP_CPU] == [22, 23, 24]
    assert len(gc.DEEP_GPU) >= 2 and all(gc.leading_zeros(value) >= 33 and nonce >= 2 ** 32 for _, nonce, value in gc.DEEP_GPU)
    assert len(set(seed for seed, _, _ in gc.DEEP)) == len(gc.DEEP)


def test_library_host_search_finds_the_cpu_found_deep_cases_from_zero():
    """sc_grind_host (transcript.h's Keccak-f, not hashlib) walks the 1.6 to 6.6 million nonces from 0 and ends on the recorded one"""
    for seed, nonce, value in gc.DEEP_CPU:
        z = gc.leading_zeros(value)
        assert grinding.grind_library_host(seed, z) == nonce
        assert grinding.grind_library_host(seed, z, nonce - gc.STRETCH, gc.STRETCH) is None      # one short of it


def test_quiet_range_holds_nothing_at_28_bits():
    seed, count = gc.QUIET
    values = [gc.pow_value(seed, nonce) for nonce in range(count)]
    assert max(gc.leading_zeros(v) for v in values) < 28
    assert [gc.smallest(seed, bits, 0, count) for bits in (1, 2, 3)] == [2, 7, 22]
    for bits in (28, 31, 32, 33, 48, 63):
        assert grinding.grind_library_host(seed, bits, 0, count) is None


def test_batch_members_fall_in_many_windows():
    """what tests/test_gpu_grind_scale.py needs of the members it takes (2 * 256 + 8 on a part of 256 compute units): minima in more
    than 16 different windows of 256, and the library's host search agrees with hashlib on some of them"""
    seeds, minima = gc.batch_members(520, 10, 30000)
    assert len(seeds) == len(set(seeds)) == 520 and None not in minima
    assert len(set(low // 256 for low in minima)) > 16
    for k in (0, 1, 519, minima.index(max(minima))):
        assert grinding.grind_library_host(seeds[k], 10) == minima[k]
    seeds, minima = gc.batch_members(65535, 3, 100000)
    assert len(set(seeds)) == 65535 and None not in minima and max(minima) < 256


# ---- the lane function, compiled by g++ ---------------------------------------------------------------------------------------------
def build(target, extra):
    srcs = [os.path.join(EMU_DIR, "grind_emu.cpp")] + CSRC
    out = os.path.join(EMU_DIR, target)
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17"] + extra + ["-o", out, srcs[0]])
    return out


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(build("libgrind_emu.so", ["-O2", "-shared", "-fPIC"]))
    u64, vp, i = ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int
    lib.emu_grind_values.restype = None
    lib.emu_grind_values.argtypes = [vp, vp, u64, i, vp]
    lib.emu_grind_accepts.restype = i
    lib.emu_grind_accepts.argtypes = [u64, i]
    lib.emu_grind_window.restype = u64
    lib.emu_grind_window.argtypes = [vp, u64, u64, u64, i]
    return lib


def test_lane_function_against_hashlib(emu):
    rng = random.Random(2)
    nonces = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1] + [rng.getrandbits(64) for _ in range(40)] + [rng.getrandbits(20) for _ in range(17)]
    seeds = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in nonces]
    expect = [gc.pow_value(seed, nonce) for seed, nonce in zip(seeds, nonces)]
    for unrolled in (0, 1):
        got = (ctypes.c_uint64 * len(nonces))()
        emu.emu_grind_values(b"".join(seeds), (ctypes.c_uint64 * len(nonces))(*nonces), len(nonces), unrolled, got)
        assert list(got) == expect
    for bits in range(1, 64):                                  # every shift, those across the 32-bit half included
        assert emu.emu_grind_accepts(2 ** (64 - bits) - 1, bits) == 1 and emu.emu_grind_accepts(2 ** (64 - bits), bits) == 0
        assert emu.emu_grind_accepts(0, bits) == 1 and emu.emu_grind_accepts(2 ** 64 - 1, bits) == 0 and emu.emu_grind_accepts(2 ** 63, bits) == 0


def test_window_walk_of_the_lane_function(emu):
    """a window as the kernel walks it: the minimum of the window, nothing when the window holds none, no wrap at the top of the range"""
    for window, bits in gc.WINDOWS:
        for seed, low in gc.placements(window, bits).values():
            index = low // window
            assert emu.emu_grind_window(seed, 0, index * window, window, bits) == low
            if index:
                assert emu.emu_grind_window(seed, 0, (index - 1) * window, window, bits) == 2 ** 64 - 1
    seed = b"\x07" * 32
    start = 2 ** 64 - 300
    assert start + emu.emu_grind_window(seed, start, 0, 300, 4) == gc.smallest(seed, 4, start, 300)


def test_standalone_program_under_sanitizers():
    program = build("grind_emu_main", ["-DGRIND_EMU_MAIN", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    done = subprocess.run([program], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert done.returncode == 0 and "grind ok" in done.stdout, (done.stdout + done.stderr)[-2000:]


# ---- the library's host search (no device needed) -----------------------------------------------------------------------------------
def test_library_host_search_on_the_cases():
    for seed, bits, start, expected in gc.CASES:
        assert grinding.grind_library_host(seed, bits, start, expected - start + 1) == expected   # a range that just reaches the minimum
        if expected - start <= 1 << 17:                        # (the hashlib loop takes a microsecond or two per trial)
            assert grinding.grind_host(seed, bits, start) == expected
            assert grinding.grind_library_host(seed, bits, start) == expected
            assert grinding.grind_library_host(seed, bits, start, expected - start) is None       # one short of the minimum
    seed = b"\x07" * 32
    assert grinding.grind_library_host(seed, 4, 2 ** 64 - 300, 300) == gc.smallest(seed, 4, 2 ** 64 - 300, 300) == grinding.grind_host(seed, 4, 2 ** 64 - 300)
    assert grinding.grind_library_host(seed, 63, 5, 100) is None and grinding.grind_host(seed, 63, 5, 100) is None
    assert grinding.grind_library_host(seed, 4, 0, 0) is None


def test_library_refuses_bad_ranges():
    import starkcore
    lib = starkcore.lib()
    nonce, found = ctypes.c_uint64(7), ctypes.c_int(7)
    seed = b"\x07" * 32
    for bits, start, count in ((0, 0, 10), (64, 0, 10), (-1, 0, 10), (8, 2 ** 64 - 300, 301), (8, 2, 2 ** 64 - 1)):
        assert lib.sc_grind_host(seed, bits, start, count, ctypes.byref(nonce), ctypes.byref(found)) != 0
        assert lib.sc_grind(seed, bits, start, count, ctypes.byref(nonce), ctypes.byref(found), None) != 0     # refused before any device is touched
        assert lib.sc_grind_batch(seed, 1, bits, start, count, ctypes.byref(nonce), ctypes.byref(ctypes.c_uint8(0)), None) != 0
    assert (nonce.value, found.value) == (7, 7)
    with pytest.raises(AssertionError):
        grinding.grind_host(seed, 8, 2 ** 64 - 300, 301)
    with pytest.raises(AssertionError):
        grinding.grind(seed, 0)
    assert grinding.grind_batch([], 8) == []


def test_library_refuses_more_than_65535_members_before_any_device_work():
    """no device is needed (or looked for) to refuse the batch: the answer is SC_ERR_BAD_ARG, not a HIP error, and nothing is written"""
    import starkcore
    lib = starkcore.lib()
    count = 65536
    nonces, found = (ctypes.c_uint64 * count)(*[7] * count), (ctypes.c_uint8 * count)(*[7] * count)
    assert lib.sc_grind_batch(b"\x07" * (32 * count), count, 3, 0, 100, nonces, found, None) == -6          # SC_ERR_BAD_ARG (include/starkcore.h)
    assert "at most 65535" in lib.sc_last_error().decode()
    assert set(nonces) == {7} and set(found) == {7}


# ---- the verifier's check, on transcripts built by hand ------------------------------------------------------------------------------
@pytest.fixture()
def fri_by_hand(monkeypatch):
    """a Fri of two rounds at 8 grinding bits and a transcript [root, root, last codeword]: the last codeword's own checks (a Merkle
    tree and an interpolation, both device work) are answered by hand, so that the walk reaches the proof of work without a GPU"""
    import fri as fri_module
    from algebra import Field, FieldElement
    from ip import ProofStream
    field = Field.main()
    fri = fri_module.Fri(field.generator(), field.primitive_nth_root(32), 32, 4, 2, grinding_bits=8)
    assert fri.num_rounds() == 2
    roots = [b"\x11" * 64, b"\x22" * 64]
    monkeypatch.setattr(fri_module.Merkle, "commit", lambda data: roots[-1])
    monkeypatch.setattr(fri_module.Fri, "_last_codeword_degree", lambda self, *a: 0)

    def stream(*behind):
        ps = ProofStream()
        for obj in roots + [[FieldElement(3, field)] * 16] + list(behind):
            ps.push(obj)
        return ps
    seed = stream().prover_fiat_shamir()
    return fri, stream, seed


def test_verify_rejects_a_bad_nonce(fri_by_hand, capsys):
    fri, stream, seed = fri_by_hand
    good = grinding.grind_host(seed, 8)
    later = ("later", "objects")
    bad = [None, b"\x00" * 8, float(good), True, -1, 2 ** 64, 2 ** 64 + good, good + 1 if not grinding.accepts(seed, good + 1, 8) else good + 2]
    assert not grinding.accepts(seed, bad[-1], 8)
    for nonce in bad:
        ps = stream(nonce, later)
        assert fri.verify(ps, []) is False
        assert "proof of work fails" in capsys.readouterr().out
        assert ps.read_index == 4 and ps.objects[4] is later    # the nonce was the last object read
    # nothing behind the last codeword: the pull itself fails
    with pytest.raises(AssertionError):
        fri.verify(stream(), [])
    # the accepted nonce passes the check: the walk goes on to the query phase and finds the stream empty there
    ps = stream(good)
    assert fri._check_grinding(_read(ps, 3)) is True and ps.read_index == 4
    with pytest.raises(AssertionError, match="queue empty"):
        fri.verify(stream(good), [])
    assert "proof of work fails" not in capsys.readouterr().out
    # in a batch: False for exactly the members with a bad nonce (or none), whatever their neighbours hold
    verdicts = fri.verify_batch([stream(nonce, later) for nonce in bad] + [stream()], [[] for _ in range(len(bad) + 1)])
    assert verdicts == [False] * (len(bad) + 1)


def _read(ps, count):
    for _ in range(count):
        ps.pull()
    return ps


def test_zero_bits_push_and_pull_nothing():
    import fri as fri_module
    from algebra import Field
    from ip import ProofStream
    field = Field.main()
    plain = fri_module.Fri(field.generator(), field.primitive_nth_root(32), 32, 4, 2)
    assert plain.grinding_bits == 0 and fri_module.Fri(field.generator(), field.primitive_nth_root(32), 32, 4, 2, 0).grinding_bits == 0
    ps = ProofStream()
    ps.push(b"\x01" * 64)
    ps.prover_fiat_shamir = ps.verifier_fiat_shamir = None     # no seed is taken
    plain.grind(ps)
    assert ps.objects == [b"\x01" * 64]
    assert plain._check_grinding(ps) is True and ps.read_index == 0


def test_constructors():
    import fri as fri_module
    from algebra import Field
    from fast_stark import FastStark
    from sharded_fri import ShardedFri
    field = Field.main()
    make = lambda bits: fri_module.Fri(field.generator(), field.primitive_nth_root(32), 32, 4, 2, grinding_bits=bits)
    assert make(grinding.MAX_BITS).grinding_bits == grinding.MAX_BITS == 40
    for bits in (grinding.MAX_BITS + 1, -1, 8.0, None):
        with pytest.raises(AssertionError):
            make(bits)
    stark = FastStark(field, 4, 4, 16, 2, 4, grinding_bits=8)
    assert stark.grinding_bits == 8 and stark.fri.grinding_bits == 8 and stark.fri.num_colinearity_tests == 4 and stark.num_randomizers == 16
    assert FastStark(field, 4, 8, 16, 2, 4).fri.grinding_bits == 0
    with pytest.raises(AssertionError):
        FastStark(field, 4, 4, 16, 2, 4, grinding_bits=7)       # 2 * 4 + 7 < 16
    with pytest.raises(AssertionError):
        FastStark(field, 4, 4, 16, 2, 4)
    with pytest.raises(AssertionError):
        FastStark(field, 4, 4, 64, 2, 4, grinding_bits=grinding.MAX_BITS + 16)
    with pytest.raises(AssertionError, match="sharded provers do not grind"):
        ShardedFri(make(8), 4, 0, 1, None, engine=object())


def test_lazy_objects_pickle_a_nonce_like_pickle():
    """the prover's described objects with a plain int among them: the library's pickler writes what pickle.dumps writes"""
    import pickle
    import proof_objects
    for nonce in (0, 255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1):
        lazy = proof_objects.LazyProofObjects([b"\x01" * 64, b"\x02" * 64])
        lazy.append(nonce)
        lazy.append([b"\x03" * 64, b"\x04" * 64])
        assert lazy.pickled() == pickle.dumps([b"\x01" * 64, b"\x02" * 64, nonce, [b"\x03" * 64, b"\x04" * 64]])

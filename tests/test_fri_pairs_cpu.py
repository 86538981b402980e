"""Pair leaves for FRI without a GPU (Fri(pair_leaves=True), csrc/fri_pairs.cuh): Merkle.commit_pairs / open_pair /
verify_pair against hashlib written out here; the plain-Python prover of tests/fri_pairs_cases.py -- the specification the GPU tests
compare bytes with -- checked against the verifier's rules by hand; the exact digest count of a proof; and the per-lane index function of
the fused fold-and-hash leaf stage, compiled for the host by tests/emu/fri_pairs_emu.cpp, lane by lane against Python integers and once
more as a stand-alone program under ASan + UBSan (FRI_PAIRS_EMU_CXXFLAGS overrides the flags)."""
import ctypes
import os
import struct
import subprocess
from hashlib import blake2b

import pytest

from conftest import REPO
import fri_pairs_cases as cases
from fri_pairs_cases import G, P

EMU_DIR = os.path.join(REPO, "tests", "emu")
CSRC = os.path.join(REPO, "stark-anatomy_amd", "csrc")
SOURCES = [os.path.join(EMU_DIR, "fri_pairs_emu.cpp")] + [os.path.join(CSRC, f) for f in ("fri_pairs.cuh", "merkle_rows.cuh", "merkle.cuh", "field.cuh", "transcript.h")]


def stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in SOURCES)


def fe(values):
    from algebra import Field, FieldElement
    field = Field.main()
    return [FieldElement(v, field) for v in values]


@pytest.mark.parametrize("n", (2, 4, 64))
def test_pair_trees_against_hashlib(n):
    from merkle import Merkle
    ints = cases.codeword(64, 4)[:n]
    half = n // 2
    leaves = [blake2b(ints[i].to_bytes(16, "little") + ints[i + half].to_bytes(16, "little"), person=b"sc-merkle-row").digest() for i in range(half)]
    level, levels = leaves, [leaves]
    while len(level) > 1:
        level = [blake2b(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
        levels.append(level)
    root = level[0]
    codeword = fe(ints)
    assert Merkle.commit_pairs(codeword) == root == cases.pair_levels(ints)[-1][0]
    assert Merkle.commit_pairs(codeword) == Merkle.commit_rows([codeword[:half], codeword[half:]])
    # neither the plain tree over the same codeword (decimal leaves, written out) nor the pair tree with the halves swapped
    assert root != Merkle.commit_([blake2b(b"%d" % v).digest() for v in ints])
    assert root != Merkle.commit_pairs(codeword[half:] + codeword[:half])
    one = codeword[0].field.one()
    for index in range(half):
        pair, path = Merkle.open_pair(index, codeword)
        assert type(pair) is tuple and [v.value for v in pair] == [ints[index], ints[index + half]]
        assert path == [lvl[(index >> l) ^ 1] for l, lvl in enumerate(levels[:-1])] and len(path) == half.bit_length() - 1
        assert Merkle.verify_pair(root, index, path, pair) is True
        assert cases.verify_pair(root, index, path, pair[0].value, pair[1].value)
        assert Merkle.verify_pair(root, index, path, (pair[1], pair[0])) is False
        assert Merkle.verify_pair(root, index, path, (pair[0] + one, pair[1])) is False
        assert Merkle.verify_pair(root, index, path, (pair[0], pair[1] + one)) is False
        if half > 1:
            assert Merkle.verify_pair(root, index ^ 1, path, pair) is False
            assert Merkle.verify_pair(root, index >> 1, path[:-1], pair) is False


def test_pair_trees_refuse_bad_shapes():
    from merkle import Merkle
    codeword = fe(cases.codeword(64, 4)[:8])
    for bad in (codeword[:1], codeword[:3], codeword[:6]):
        with pytest.raises(AssertionError):
            Merkle.commit_pairs(bad)
    for index in (-1, 4):
        with pytest.raises(AssertionError):
            Merkle.open_pair(index, codeword)


def test_the_option_is_taken_and_off_by_default():
    from algebra import Field
    from fri import Fri
    field = Field.main()
    omega = field.primitive_nth_root(64)
    assert Fri(field.generator(), omega, 64, 4, 2).pair_leaves is False
    on = Fri(field.generator(), omega, 64, 4, 2, pair_leaves=True)
    assert on.pair_leaves is True and on.num_rounds() == cases.num_rounds(64, 4, 2) == 3
    assert on._batchable([]) is False          # (no pair forests: prove_batch goes member by member)


def spec_proof(n, expansion, s, grinding_bits=0, seed=0):
    from algebra import Field, FieldElement
    from ip import ProofStream
    field = Field.main()
    stream = ProofStream()
    values = cases.codeword(n, expansion, seed)
    top, codewords, roots = cases.prove(values, G, cases.root_of_unity(n), expansion, s, stream, lambda v: FieldElement(v, field), grinding_bits)
    return stream, top, codewords, roots


@pytest.mark.parametrize("grinding_bits", (0, 4))
def test_plain_prover_by_the_verifiers_rules(grinding_bits):
    """N = 64, expansion 4, s = 2: three codewords.  The verifier's walk by hand, in integers and hashlib: challenges from the stream's
    prefix, the last codeword under its pair root and of low degree, y_c looked up in the next round's pair or in the last codeword,
    colinearity, and every pair under its round's root."""
    from ip import ProofStream
    n, expansion, s = 64, 4, 2
    stream, top, codewords, roots = spec_proof(n, expansion, s, grinding_bits)
    rounds = cases.num_rounds(n, expansion, s)
    assert rounds == 3 and [len(c) for c in codewords] == [64, 32, 16]
    reader = ProofStream()
    reader.objects = list(stream.objects)
    pulled_roots, alphas = [], []
    for _ in range(rounds):
        pulled_roots.append(reader.pull())
        alphas.append(int.from_bytes(reader.verifier_fiat_shamir(), "big") % P)
    assert pulled_roots == roots
    last = [v.value for v in reader.pull()]
    assert last == codewords[-1] and cases.pair_levels(last)[-1][0] == roots[-1]
    # the last codeword on its coset is of degree < 16 / 4: it agrees with the interpolant through its first four points everywhere
    omega, offset = cases.root_of_unity(n), G
    w2, o2 = pow(omega, 4, P), pow(offset, 4, P)
    xs = [o2 * pow(w2, i, P) % P for i in range(16)]

    def lagrange(x):
        total = 0
        for i in range(4):
            term = last[i]
            for j in range(4):
                if j != i:
                    term = term * (x - xs[j]) % P * pow(xs[i] - xs[j], -1, P) % P
            total = (total + term) % P
        return total
    assert [lagrange(x) for x in xs] == last
    if grinding_bits:
        seed = reader.verifier_fiat_shamir()
        nonce = reader.pull()
        assert type(nonce) is int and nonce == cases.grind(seed, grinding_bits)
    assert cases.sample_indices(reader.verifier_fiat_shamir(), n // 2, 16, s) == top
    pairs, paths = [], []
    for r in range(rounds - 1):
        pairs.append([reader.pull() for _ in range(s)])
        paths.append([reader.pull() for _ in range(s)])
    assert reader.read_index == len(reader.objects)
    for r in range(rounds - 1):
        half = n >> (r + 1)
        for t, index in enumerate(top):
            a = index % half
            ya, yb = (v.value for v in pairs[r][t])
            assert (ya, yb) == (codewords[r][a], codewords[r][a + half])
            if r + 2 < rounds:
                yc = pairs[r + 1][t][0 if a < half // 2 else 1].value
            else:
                yc = last[a]
            assert yc == codewords[r + 1][a]
            assert cases.colinear([(offset * pow(omega, a, P) % P, ya), (offset * pow(omega, a + half, P) % P, yb), (alphas[r], yc)])
            assert len(paths[r][t]) == half.bit_length() - 1 and cases.verify_pair(roots[r], a, paths[r][t], ya, yb)
        omega, offset = omega * omega % P, offset * offset % P


@pytest.mark.parametrize("n,expansion,s", ((64, 4, 2), (4096, 4, 4), (4096, 4, 64)))
def test_digest_count_is_exact(n, expansion, s):
    """s (log2 N - r - 1) digests and 2 s values per queried round, counted by walking the stream; at the signature scheme's FRI shape
    (2^12, s = 64: four codewords) that is 64 (11 + 10 + 9) = 1 920 digests"""
    if s == 64:
        assert cases.digest_count(n, expansion, s) == 1920
    stream, top, codewords, roots = spec_proof(n, expansion, s)
    rounds = cases.num_rounds(n, expansion, s)
    objects = stream.objects
    assert all(type(o) is bytes and len(o) == 64 for o in objects[:rounds]) and type(objects[rounds]) is list
    at, digests, values = rounds + 1, 0, 0
    for r in range(rounds - 1):
        depth = (n >> (r + 1)).bit_length() - 1
        for pair in objects[at:at + s]:
            assert type(pair) is tuple and len(pair) == 2
            values += 2
        for path in objects[at + s:at + 2 * s]:
            assert type(path) is list and len(path) == depth and all(type(d) is bytes and len(d) == 64 for d in path)
            digests += len(path)
        at += 2 * s
    assert at == len(objects)
    assert values == 2 * s * (rounds - 1)
    assert digests == cases.digest_count(n, expansion, s) == s * sum((n.bit_length() - 1) - r - 1 for r in range(rounds - 1))


# ---- the fused leaf stage's index function on the host
@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libfri_pairs_emu.so")
    if stale(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, SOURCES[0]])
    lib = ctypes.CDLL(so)
    lib.emu_pair_fold.restype = ctypes.c_int
    lib.emu_pair_fold.argtypes = [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 5
    return lib


def twiddles(n, alpha):
    """c * w^-e, e < n/2, in Montgomery form (times 2^128), with c = alpha / (2 offset): what the kernel multiplies a - b with"""
    w_inv = pow(cases.root_of_unity(n), -1, P)
    c = alpha * pow(2 * G, -1, P) % P
    out, t = [], c
    for _ in range(n // 2):
        out.append((t << 128) % P)
        t = t * w_inv % P
    return out


@pytest.mark.parametrize("n", (1024, 4096))
def test_lane_function_on_the_host(emu, n):
    """every lane of a fold of n elements: the inputs read, the outputs written -- each exactly once, together 0 .. n/2 - 1 -- the
    twiddle exponents, the folded values and the leaf bytes"""
    q = n // 4
    raw = cases.fold_input(n)
    ints = cases.unpack(raw)
    out = ctypes.create_string_buffer(b"\xEE" * (16 * (n // 2) + 16))
    writes = (ctypes.c_uint32 * (n // 2 + 1))()
    lanes = (ctypes.c_uint64 * (8 * q + 8))()
    digests = ctypes.create_string_buffer(b"\xEE" * (64 * q + 64))
    assert emu.emu_pair_fold(raw, n, cases.pack(twiddles(n, cases.FOLD_ALPHA)), out, writes, lanes, digests) == 0
    for j in range(q):
        assert list(lanes[8 * j:8 * j + 8]) == [j, j + 2 * q, j + q, j + 3 * q, j, j + q, j, j + q]
    assert list(lanes[8 * q:]) == [0] * 8
    assert list(writes) == [1] * (n // 2) + [0]
    folded = cases.fold(ints, cases.FOLD_ALPHA, G, cases.root_of_unity(n))
    assert cases.unpack(out.raw[:16 * (n // 2)]) == folded and out.raw[16 * (n // 2):16 * (n // 2) + 16] == b"\xEE" * 16
    assert [digests.raw[64 * j:64 * j + 64] for j in range(q)] == cases.pair_levels(folded)[0]
    assert digests.raw[64 * q:64 * q + 64] == b"\xEE" * 64


def test_lane_function_refuses_bad_shapes(emu):
    buffers = [ctypes.create_string_buffer(64) for _ in range(6)]
    for n in (0, 2, 3, 12):
        assert emu.emu_pair_fold(buffers[0], n, *buffers[1:]) == 1
    assert emu.emu_pair_fold(None, 4, *buffers[1:]) == 1


def test_standalone_lane_function_under_sanitizers(tmp_path):
    """the same program with a main of its own, built under ASan + UBSan and run once: n = 4, 1024 and 4096"""
    flags = os.environ.get("FRI_PAIRS_EMU_CXXFLAGS", "-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer").split()
    program = os.path.join(EMU_DIR, "fri_pairs_emu_main")
    if stale(program) or "FRI_PAIRS_EMU_CXXFLAGS" in os.environ:
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DFRI_PAIRS_EMU_MAIN"] + flags + ["-o", program, SOURCES[0]])
    sizes = (4, 1024, 4096)
    call = b"".join(struct.pack("<Q", n) + cases.fold_input(n) + cases.pack(twiddles(n, cases.FOLD_ALPHA)) for n in sizes)
    path = tmp_path / "cases.bin"
    path.write_bytes(call)
    done = subprocess.run([program, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert done.returncode == 0, done.stderr[-2000:]
    lines = done.stdout.split("\n")
    assert len(lines) == 2 * len(sizes) + 1 and lines[-1] == ""
    for k, n in enumerate(sizes):
        folded = cases.fold(cases.unpack(cases.fold_input(n)), cases.FOLD_ALPHA, G, cases.root_of_unity(n))
        assert cases.unpack(bytes.fromhex(lines[2 * k])) == folded
        assert bytes.fromhex(lines[2 * k + 1]) == b"".join(cases.pair_levels(folded)[0])

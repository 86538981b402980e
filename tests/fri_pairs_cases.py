"""Pair leaves for FRI (Fri(pair_leaves=True), csrc/fri_pairs.cuh): the specification in plain Python -- integers
modulo p, Python lists and hashlib -- shared by tests/test_fri_pairs_cpu.py and tests/test_gpu_fri_pairs.py.  Nothing here calls the
library; the prover only pushes onto the proof stream it is given (whose Fiat-Shamir step is the protocol's) and wraps what it pushes
in the field-element class it is given, because a proof is the pickle of those objects.

    pair leaf i of a codeword cw of n values   blake2b(cw[i] || cw[i + n/2], person = "sc-merkle-row"), 16 little-endian bytes each
    node                                       blake2b(left || right)
    a proof                                    rounds roots, the last codeword, [the nonce], then per round r < rounds - 1:
                                               s pairs (cw_r[a], cw_r[a + half]), then s paths of leaf a (log2 half digests)
"""
import functools
import random
from hashlib import blake2b, shake_256

PERSON = b"sc-merkle-row"
P = 1 + 407 * (1 << 119)
G = 85408008396924667383611388730472331217            # of multiplicative order 2^119


def root_of_unity(n):
    return pow(G, 1 << (119 - (n.bit_length() - 1)), P)


def pack(values):
    return b"".join(v.to_bytes(16, "little") for v in values)


def unpack(raw):
    return [int.from_bytes(raw[i:i + 16], "little") for i in range(0, len(raw), 16)]


def pair_leaf(ya, yb):
    return blake2b(ya.to_bytes(16, "little") + yb.to_bytes(16, "little"), person=PERSON).digest()


def pair_levels(values):
    """every level of the pair tree over a codeword of n >= 2 integers, the n/2 leaves first, the root's level last"""
    n = len(values)
    assert n >= 2 and n & (n - 1) == 0
    level = [pair_leaf(values[i], values[i + n // 2]) for i in range(n // 2)]
    out = [level]
    while len(level) > 1:
        level = [blake2b(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
        out.append(level)
    return out


def pair_levels_packed(raw):
    """pair_levels over packed residues (a 2^20-element case without a million Python integers)"""
    n = len(raw) // 16
    level = [blake2b(raw[16 * i:16 * i + 16] + raw[16 * (i + n // 2):16 * (i + n // 2) + 16], person=PERSON).digest() for i in range(n // 2)]
    out = [level]
    while len(level) > 1:
        level = [blake2b(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
        out.append(level)
    return out


def path(levels, index):
    """fresh bytes objects, as an opening makes them: a proof is pickled, and pickle writes an object it has seen as a reference"""
    return [bytes(bytearray(level[(index >> l) ^ 1])) for l, level in enumerate(levels[:-1])]


def verify_pair(root, index, auth_path, ya, yb):
    node = pair_leaf(ya, yb)
    for sibling in auth_path:
        node = blake2b(node + sibling).digest() if index % 2 == 0 else blake2b(sibling + node).digest()
        index >>= 1
    return index == 0 and node == root


def fold(values, alpha, offset, omega):
    """the split-and-fold of the tutorial: out[i] = ((1 + alpha / x_i) cw[i] + (1 - alpha / x_i) cw[i + n/2]) / 2, x_i = offset omega^i"""
    n = len(values)
    half, inv2 = n // 2, pow(2, -1, P)
    out, x = [], offset
    for i in range(half):
        t = alpha * pow(x, -1, P) % P
        out.append(inv2 * ((1 + t) * values[i] + (1 - t) * values[i + half]) % P)
        x = x * omega % P
    return out


def num_rounds(n, expansion, s):
    rounds = 0
    while n > expansion and n > 4 * s:
        rounds, n = rounds + 1, n // 2
    return rounds


def sample_indices(seed, size, reduced_size, number):
    chosen, residues, counter = [], set(), 0
    while len(chosen) < number:
        candidate = int.from_bytes(blake2b(seed + bytes(counter)).digest(), "big") % size
        counter += 1
        if candidate % reduced_size in residues:
            continue
        residues.add(candidate % reduced_size)
        chosen.append(candidate)
    return chosen


def grind(seed, bits):
    nonce = 0
    while int.from_bytes(shake_256(bytes(seed) + nonce.to_bytes(8, "little")).digest(8), "little") >> (64 - bits):
        nonce += 1
    return nonce


def digest_count(n, expansion, s):
    """path digests of a proof: s per round r < rounds - 1, each of log2(n) - r - 1"""
    log_n = n.bit_length() - 1
    return s * sum(log_n - r - 1 for r in range(num_rounds(n, expansion, s) - 1))


def prove(values, offset, omega, expansion, s, stream, element, grinding_bits=0):
    """The prover of the protocol.  values: the first codeword as integers; stream: push / prover_fiat_shamir; element(v): the
    object an integer travels as.  Returns (top-level indices, the codewords as integers, the roots)."""
    n = len(values)
    rounds = num_rounds(n, expansion, s)
    codewords, trees, roots = [], [], []
    current = list(values)
    for r in range(rounds):
        tree = pair_levels(current)
        stream.push(tree[-1][0])
        codewords.append(current)
        trees.append(tree)
        roots.append(tree[-1][0])
        if r == rounds - 1:
            break
        alpha = int.from_bytes(stream.prover_fiat_shamir(), "big") % P
        current = fold(current, alpha, offset, omega)
        omega, offset = omega * omega % P, offset * offset % P
    stream.push([element(v) for v in codewords[-1]])
    if grinding_bits:
        stream.push(grind(stream.prover_fiat_shamir(), grinding_bits))
    top = sample_indices(stream.prover_fiat_shamir(), n // 2, len(codewords[-1]), s)
    for r in range(rounds - 1):
        half = n >> (r + 1)
        lower = [index % half for index in top]
        for a in lower:
            stream.push((element(codewords[r][a]), element(codewords[r][a + half])))
        for a in lower:
            stream.push(path(trees[r], a))
    return top, codewords, roots


def colinear(points):
    """three points (x, y) on one line, in integers modulo p"""
    (x0, y0), (x1, y1), (x2, y2) = points
    return ((y1 - y0) * (x2 - x0) - (y2 - y0) * (x1 - x0)) % P == 0


def _transform(values, root):
    """values of the polynomial with these coefficients at root^0, root^1, ... (radix-2 recursion)"""
    n = len(values)
    if n == 1:
        return list(values)
    even, odd = _transform(values[0::2], root * root % P), _transform(values[1::2], root * root % P)
    out, x = [0] * n, 1
    for i in range(n // 2):
        t = x * odd[i] % P
        out[i], out[i + n // 2] = (even[i] + t) % P, (even[i] - t) % P
        x = x * root % P
    return out


@functools.lru_cache(maxsize=None)
def _codeword(n, expansion, seed):
    rng = random.Random(7919 * n + seed)
    coefficients = [rng.randrange(P) for _ in range(n // expansion)] + [0] * (n - n // expansion)
    scaled, x = [], 1
    for c in coefficients:                                 # f(G x): coefficient i times G^i
        scaled.append(c * x % P)
        x = x * G % P
    return tuple(_transform(scaled, root_of_unity(n)))


def codeword(n, expansion, seed=0):
    """a codeword of length n on G * <root_of_unity(n)> of a random polynomial of degree < n / expansion, as integers"""
    return list(_codeword(n, expansion, seed))


# ---- inputs of the fold-and-commit kernel tests
def fold_input(n, seed=0):
    """n >= 8 residues, packed: 0, 1 and p - 1 at positions 0 .. 2, in[3] == in[3 + n/2], in[1 + n/2] == -in[1]; the rest random (above
    4096 elements drawn as bytes with the top bit cleared: below 2^127 < p).  n == 4: [1, 0, p - 1, 0]."""
    if n == 4:
        return pack([1, 0, P - 1, 0])
    rng = random.Random(104729 * n + seed)
    half = n // 2
    if n <= 4096:
        raw = bytearray(pack([rng.randrange(P) for _ in range(n)]))
    else:
        mask = int.from_bytes((b"\xff" * 15 + b"\x7f") * n, "little")
        raw = bytearray((int.from_bytes(rng.randbytes(16 * n), "little") & mask).to_bytes(16 * n, "little"))
    for i, v in ((0, 0), (1, 1), (2, P - 1), (1 + half, P - 1)):
        raw[16 * i:16 * i + 16] = v.to_bytes(16, "little")
    raw[16 * (3 + half):16 * (4 + half)] = raw[16 * 3:16 * 4]
    return bytes(raw)


FOLD_ALPHA = 0x1234567890ABCDEF1234567890ABCDEF % P


@functools.lru_cache(maxsize=None)
def fold_reference(n):
    """(packed input, folded integers, levels of the pair tree over them) for n <= 2048, computed once (callers leave them unchanged)"""
    raw = fold_input(n)
    folded = fold(unpack(raw), FOLD_ALPHA, G, root_of_unity(n))
    return raw, folded, pair_levels(folded)

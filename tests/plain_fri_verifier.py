"""An independent FRI verifier, and the option-off prover beside it, in plain Python: integers modulo p, hashlib and pickle (the
transcript IS a pickle).  Written from the protocol as DESIGN.md 3.4e, grinding.py's specification and the docstrings of fri.py and
fri_pairs_cases.py state it; nothing here calls the library.  A field element is read by its `value` and `field.p`.

    a proof            rounds roots, the last codeword, [the nonce], then per round r < rounds - 1
      decimal leaves   s triples (cw_r[a], cw_r[a + half], cw_{r+1}[a]), then per test the paths of a and a + half under root r and of a
                       under root r + 1; a leaf is blake2b(decimal ASCII of the value)
      pair leaves      s pairs (cw_r[a], cw_r[a + half]), then s paths of leaf a under root r (fri_pairs_cases.pair_leaf); y_c is not
                       in the proof: it is the member of round r + 1's pair of the same test that lies at position a -- member 0 when
                       a < half / 2, else member 1 -- or last_codeword[a] in the last queried round
    challenges         shake_256(prefix + pickle.dumps(objects read so far)).digest(32): alpha_r after root r (big-endian, mod p), the
                       proof of work's seed after the last codeword, the indices' seed after the nonce; prefix = b"" for a plain
                       ProofStream, the document's digest for a document-bound one
    a test             (offset_r omega_r^a, y_a), (offset_r omega_r^(a + half), y_b), (alpha_r, y_c) on one line, a = index % half

failures() walks the whole proof and lists every check that fails as (reason, round) -- round None outside the query phase -- in the
order shape / last codeword / degree / proof of work, then per round its colinearity tests and its paths.  A failure of the first four
kinds ends the walk: nothing behind it can be read.  verify() is (no failure, the first failure's reason)."""
import pickle
from hashlib import blake2b, shake_256

import fri_pairs_cases as cases
from fri_pairs_cases import P

REASONS = ("shape", "last codeword", "degree", "proof of work", "colinearity", "merkle")


# ---- decimal leaves: the tree of the option-off protocol
def decimal_leaf(value):
    return blake2b(b"%d" % value).digest()


def decimal_levels(values):
    level = [decimal_leaf(v) for v in values]
    out = [level]
    while len(level) > 1:
        level = [blake2b(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
        out.append(level)
    return out


def climbs_to(root, index, path, node):
    for sibling in path:
        node = blake2b(node + sibling).digest() if index % 2 == 0 else blake2b(sibling + node).digest()
        index >>= 1
    return index == 0 and node == root


def prove_decimal(values, offset, omega, expansion, s, stream, element, grinding_bits=0):
    """The option-off prover (fri_pairs_cases.prove is the option-on one; same arguments, same return).  A value that the proof holds
    twice -- y_c of round r is y_a or y_b of round r + 1, or an entry of the last codeword -- travels as ONE object: the transcript is
    a pickle, which writes an object it has seen as a reference."""
    n = len(values)
    rounds = cases.num_rounds(n, expansion, s)
    codewords, trees, roots = [], [], []
    current = list(values)
    for r in range(rounds):
        tree = decimal_levels(current)
        stream.push(tree[-1][0])
        codewords.append(current)
        trees.append(tree)
        roots.append(tree[-1][0])
        if r == rounds - 1:
            break
        alpha = int.from_bytes(stream.prover_fiat_shamir(), "big") % P
        current = cases.fold(current, alpha, offset, omega)
        omega, offset = omega * omega % P, offset * offset % P
    entries = [{} for _ in range(rounds)]
    entries[-1] = {i: element(v) for i, v in enumerate(codewords[-1])}

    def entry(r, i):
        if i not in entries[r]:
            entries[r][i] = element(codewords[r][i])
        return entries[r][i]

    stream.push([entries[-1][i] for i in range(len(codewords[-1]))])
    if grinding_bits:
        stream.push(cases.grind(stream.prover_fiat_shamir(), grinding_bits))
    top = cases.sample_indices(stream.prover_fiat_shamir(), n // 2, len(codewords[-1]), s)
    for r in range(rounds - 1):
        half = n >> (r + 1)
        lower = [index % half for index in top]
        for a in lower:
            stream.push((entry(r, a), entry(r, a + half), entry(r + 1, a)))
        for a in lower:
            stream.push(cases.path(trees[r], a))
            stream.push(cases.path(trees[r], a + half))
            stream.push(cases.path(trees[r + 1], a))
    return top, codewords, roots


# ---- the verifier
class _Shape(Exception):
    pass


def _value(obj, canonical):
    """the integer of a field element of this field; canonical: below p (pair leaves hash 16 bytes of it and refuse anything else)"""
    if type(obj).__name__ != "FieldElement" or type(obj.value) is not int or getattr(obj.field, "p", None) != P:
        raise _Shape()
    if obj.value < 0 or (canonical and obj.value >= P):
        raise _Shape()
    return obj.value


def _values(obj, count, canonical):
    if type(obj) not in (list, tuple) or len(obj) != count:
        raise _Shape()
    return [_value(member, canonical) for member in obj]


def _path(obj, depth=None):
    if type(obj) not in (list, tuple) or not all(type(d) is bytes and len(d) == 64 for d in obj) or (depth is not None and len(obj) != depth):
        raise _Shape()
    return list(obj)


def _degree(values, omega):
    """of the interpolant through `values` on a coset of <omega>: the coset's offset scales coefficient k by offset^-k, which moves no
    zero, so the plain inverse transform's highest non-zero coefficient decides"""
    n = len(values)
    inverse = pow(omega, -1, P)
    for k in range(n - 1, -1, -1):
        if sum(v * pow(inverse, i * k, P) for i, v in enumerate(values)) % P:
            return k
    return -1


def accepts(seed, nonce, bits):
    """grinding.py's specification"""
    return type(nonce) is int and 0 <= nonce < (1 << 64) and \
        int.from_bytes(shake_256(bytes(seed) + nonce.to_bytes(8, "little")).digest(8), "little") >> (64 - bits) == 0


def failures(objects, n, expansion, s, offset, omega, pair_leaves, grinding_bits=0, prefix=b""):
    """every failed check as (reason, round)"""
    objects = list(objects)
    rounds = cases.num_rounds(n, expansion, s)
    n_last = n >> (rounds - 1)
    at = [0]

    def pull():
        if at[0] >= len(objects):
            raise _Shape()
        at[0] += 1
        return objects[at[0] - 1]

    def seed():
        return shake_256(prefix + pickle.dumps(objects[:at[0]])).digest(32)

    queried = None
    try:
        roots, alphas = [], []
        for _ in range(rounds):
            root = pull()
            if type(root) is not bytes or len(root) != 64:
                raise _Shape()
            roots.append(root)
            alphas.append(int.from_bytes(seed(), "big") % P)
        try:
            last = _values(pull(), n_last, pair_leaves)
            levels = cases.pair_levels(last) if pair_leaves else decimal_levels(last)
        except (_Shape, OverflowError):
            return [("last codeword", None)]
        if levels[-1][0] != roots[-1]:
            return [("last codeword", None)]
        if _degree(last, pow(omega, 1 << (rounds - 1), P)) > n_last // expansion - 1:
            return [("degree", None)]
        if grinding_bits:
            pow_seed = seed()
            if not accepts(pow_seed, pull(), grinding_bits):
                return [("proof of work", None)]
        top = cases.sample_indices(seed(), n // 2, n_last, s)
        ys, paths = [], []
        for r in range(rounds - 1):
            queried = r
            depth = (n >> (r + 1)).bit_length() - 1
            if pair_leaves:
                ys.append([_values(pull(), 2, True) for _ in range(s)])
                paths.append([[_path(pull(), depth)] for _ in range(s)])
            else:
                ys.append([_values(pull(), 3, False) for _ in range(s)])
                paths.append([[_path(pull()) for _ in range(3)] for _ in range(s)])
    except _Shape:
        return [("shape", queried)]
    found = []
    for r in range(rounds - 1):
        half = n >> (r + 1)
        for t, index in enumerate(top):
            a = index % half
            if not pair_leaves:
                ya, yb, yc = (y % P for y in ys[r][t])
            else:
                ya, yb = ys[r][t]
                if r + 2 < rounds:
                    yc = ys[r + 1][t][0 if a < half // 2 else 1]
                else:
                    yc = last[a]
            if not cases.colinear([(offset * pow(omega, a, P) % P, ya), (offset * pow(omega, a + half, P) % P, yb), (alphas[r], yc)]):
                found.append(("colinearity", r))
        for t, index in enumerate(top):
            a = index % half
            if pair_leaves:
                ya, yb = ys[r][t]
                held = cases.verify_pair(roots[r], a, paths[r][t][0], ya, yb)
            else:
                ya, yb, yc = ys[r][t]                          # (as they stand: the leaf is the decimal string of the value as sent)
                held = (climbs_to(roots[r], a, paths[r][t][0], decimal_leaf(ya)) and climbs_to(roots[r], a + half, paths[r][t][1], decimal_leaf(yb))
                        and climbs_to(roots[r + 1], a, paths[r][t][2], decimal_leaf(yc)))
            if not held:
                found.append(("merkle", r))
        omega, offset = omega * omega % P, offset * offset % P
    return found


def verify(objects, n, expansion, s, offset, omega, pair_leaves, grinding_bits=0, prefix=b""):
    """(verdict, reason): (True, None), or False and the first failed check's reason; whatever raises inside is False"""
    try:
        found = failures(objects, n, expansion, s, offset, omega, pair_leaves, grinding_bits, prefix)
    except Exception:
        return False, "shape"
    return (True, None) if not found else (False, found[0][0])

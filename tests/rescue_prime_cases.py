"""States, rounds, constants and inputs for the Rescue-Prime kernels (sc_rescue_prime_hash_dev / sc_rescue_prime_trace_dev,
stark-anatomy_amd/csrc/rescue.hip and rescue_prime.cuh).  tests/test_gpu_rescue_prime_edges.py runs them on the GPU,
tests/test_rescue_prime_cases_cpu.py proves on the host that every case reaches the states it names.  Nothing here touches a GPU,
pytest, rescue_prime.RescuePrime or csrc/: the expectations are Python integers mod p = 1 + 407 * 2^119 through `pow`.

With the reference's constants a state element that is 0, 1 or p - 1 INSIDE the permutation has probability about 2^-128 per round.
So the constants are chosen instead: `steer` solves for the round constants under which one input passes through a chosen state
after every half-round, for any matrix.  The chosen states come from TABLE (the plain edge residues and residues whose Montgomery
form -- what the kernel's registers hold -- is special) and, for one case, from the elements of small or two-power order.

The ABI (include/starkcore.h): params = 4 + 4 * rounds canonical residues, the matrix row-major, then per round two constants added
after the cube's mix and two after the inverse cube's mix; hash: out[k] = register 0 of the last state; trace: register s of
input k's state t at out[(2 k + s) * (rounds + 1) + t]."""
import functools
import json
import os
import random

P = 407 * (1 << 119) + 1
ALPHA = 3
ALPHAINV = (2 * P - 1) // 3                       # 3^-1 mod (p - 1)
R = (1 << 128) % P                                # the Montgomery radix of csrc/field.cuh
RINV = pow(R, -1, P)
MAX_ROUNDS = 27
TOP = (1 << 128) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pack(values):
    return b"".join(int(v).to_bytes(16, "little") for v in values)


def unpack(buf):
    return [int.from_bytes(buf[i:i + 16], "little") for i in range(0, len(buf), 16)]


# ---- the model ------------------------------------------------------------------------------------------------------------------

def half_round(state, mds, rc, off, exponent):
    w = [pow(v, exponent, P) for v in state]
    return [(mds[2 * i] * w[0] + mds[2 * i + 1] * w[1] + rc[off + i]) % P for i in range(2)]


def half_states(x, mds, rc, rounds):
    """[x mod p, 0] and the state after each of the 2 * rounds half-rounds: entry 2 r + 1 stands in front of round r's inverse
    cube, entry 2 r in front of round r's cube"""
    state = [x % P, 0]
    out = [state]
    for r in range(rounds):
        state = half_round(state, mds, rc, 4 * r, ALPHA)
        out.append(state)
        state = half_round(state, mds, rc, 4 * r + 2, ALPHAINV)
        out.append(state)
    return out


def states(x, mds, rc, rounds):
    """the rounds + 1 states of the input x: mds four residues (row-major), rc 4 * rounds residues"""
    return half_states(x, mds, rc, rounds)[::2]


def steer(x, mds, targets):
    """round constants under which input x has state targets[j] after half-round j (len(targets) = 2 * rounds pairs): each constant
    is the target minus the matrix times the powered state, so any matrix does, the zero matrix included"""
    assert len(targets) % 2 == 0
    state, rc = [x % P, 0], []
    for j, target in enumerate(targets):
        w = [pow(v, ALPHAINV if j % 2 else ALPHA, P) for v in state]
        rc += [(target[i] - mds[2 * i] * w[0] - mds[2 * i + 1] * w[1]) % P for i in range(2)]
        state = [t % P for t in target]
    return rc


def expected_hash(xs, mds, rc, rounds):
    return [states(x, mds, rc, rounds)[rounds][0] for x in xs]


def expected_trace(xs, mds, rc, rounds):
    """the trace entry's output: 2 n (rounds + 1) residues"""
    out = []
    for x in xs:
        st = states(x, mds, rc, rounds)
        for s in range(2):
            out += [row[s] for row in st]
    return out


# ---- the states steered to ------------------------------------------------------------------------------------------------------

def of_form(form):
    """the residue whose Montgomery form is `form`"""
    assert 0 <= form < P
    return form * RINV % P


_FORM = random.Random(0x5EED0).randrange(P)        # a seeded form: its limbs are cut below
# Forms below p whose 32-bit or 64-bit limbs are all zero or all one.  p's top 32-bit limb is 0xCB800000, so no form below p has
# an all-one top limb: p - 2 = 0xCB7FFFFF FFFFFFFF FFFFFFFF FFFFFFFF stands for it (every limb below the top one all ones).
SPECIAL = {
    "form 1": RINV,
    "form R^2": R,
    "form low32 zero": of_form(_FORM & ~0xFFFFFFFF),
    "form low32 ones": of_form(_FORM | 0xFFFFFFFF),
    "form high32 zero": of_form(_FORM & ((1 << 96) - 1)),
    "form p-2": of_form(P - 2),
    "form low64 zero": of_form(1 << 64),
    "form low64 ones high64 zero": of_form((1 << 64) - 1),
    "form 2^32": of_form(1 << 32),
}
_S = list(SPECIAL.values())
# (register 0, register 1).  The first six are the plain edge states; the rest put every special value into both registers.
TABLE = ((0, 0), (0, 1), (1, 0), (P - 1, P - 1), (1, P - 1), (0, P - 1)) \
    + tuple((_S[i], _S[(i + 1) % len(_S)]) for i in range(len(_S))) + ((P - 1, RINV),)
assert len(TABLE) == 16 and len(set(TABLE)) == 16


def targets_for(rounds, start, table=TABLE):
    """2 * rounds states from `table`, one step along it per half-round from `start` on; an even-sized table takes one further step
    per pass, so that either kind of table shows every entry at both parities"""
    skip = len(table) % 2 == 0
    return [table[(start + j + (j // len(table) if skip else 0)) % len(table)] for j in range(2 * rounds)]


# ---- elements whose powers pass through 1 ---------------------------------------------------------------------------------------

ORDERS = (2, 4, 11, 37, 407, 1 << 60, 1 << 119)


def prime_factors(d):
    return [q for q in (2, 11, 37) if d % q == 0]


def has_order(e, d):
    return pow(e, d, P) == 1 and all(pow(e, d // q, P) != 1 for q in prime_factors(d))


def element_of_order(d):
    """h^((p - 1) / d) for the smallest base h >= 2 that gives the exact order d (the field's usual generator does not reach the odd
    part of the group: its (p - 1) / 11-th power is 1)"""
    assert (P - 1) % d == 0
    h = 2
    while not has_order(pow(h, (P - 1) // d, P), d):
        h += 1
    return pow(h, (P - 1) // d, P)


STRUCTURED = tuple(v for d in ORDERS for v in (element_of_order(d), P - element_of_order(d)))
STRUCTURED_TABLE = tuple((STRUCTURED[i], STRUCTURED[(i + 3) % len(STRUCTURED)]) for i in range(len(STRUCTURED))) + ((STRUCTURED[5], 0),)


# ---- matrices -------------------------------------------------------------------------------------------------------------------

def reference_parameters():
    """(matrix, round constants) of the reference, as it printed them (tests/golden/rescue_prime_params.json)"""
    with open(os.path.join(GOLDEN, "rescue_prime_params.json")) as f:
        prm = json.load(f)
    assert int(prm["p"]) == P and prm["m"] == 2 and prm["N"] == MAX_ROUNDS and prm["alpha"] == ALPHA and int(prm["alphainv"]) == ALPHAINV
    return [int(v) for row in prm["MDS"] for v in row], [int(v) for v in prm["round_constants"]]


REF_MDS, REF_RC = reference_parameters()
_M = random.Random(0x5EED1)
MATRICES = {
    "reference": REF_MDS,
    "identity": [1, 0, 0, 1],
    "zero": [0, 0, 0, 0],
    "all p-1": [P - 1] * 4,
    "random": [_M.randrange(P) for _ in range(4)],
}
ROUNDS = (1, 2, 3, 13, 26, 27)
STEERED_INPUTS = {"0": 0, "1": 1, "p-1": P - 1, "p": P, "p+1": P + 1, "2^128-1": TOP, "seeded": random.Random(0x5EED2).randrange(P)}
SIZES = (1, 2, 64, 255, 256, 257, 513)
POSITIONS = (0, 63, 64, 255, 256)                  # and n - 1
NOT_A_RESIDUE = b"\xff" * 16                       # the word behind the last constant read


def positions_of(n):
    return sorted(set(k for k in POSITIONS + (n - 1,) if k < n))


def batch(seed, n, k_star, x):
    """n seeded 128-bit words, three in four of them not below p, with x at lane k_star"""
    rng = random.Random(seed)
    xs = [rng.randrange(P, 1 << 128) if rng.randrange(4) else rng.getrandbits(128) for _ in range(n)]
    xs[k_star] = x
    return xs


class Case:
    """One launch of each entry: `n` inputs, `rounds` rounds, a matrix, and the constants that steer lane k_star through `targets`."""

    def __init__(self, name, matrix, rounds, x, n, k_star, start, table=TABLE, seed=0):
        self.name, self.matrix, self.rounds, self.x, self.n, self.k_star = name, matrix, rounds, x, n, k_star
        self.mds = MATRICES[matrix]
        self.targets = targets_for(rounds, start, table)
        self.rc = steer(x, self.mds, self.targets)
        self.inputs = batch(0xBA7C0 + seed, n, k_star, x)
        self.input_bytes = pack(self.inputs)
        # what the ABI reads, then a word it must not look at
        self.params = pack(self.mds + self.rc) + NOT_A_RESIDUE

    @functools.cached_property
    def lane_states(self):
        return [states(x, self.mds, self.rc, self.rounds) for x in self.inputs]

    @functools.cached_property
    def hash(self):
        return pack(st[self.rounds][0] for st in self.lane_states)

    @functools.cached_property
    def trace(self):
        return pack(row[s] for st in self.lane_states for s in range(2) for row in st)

    def __repr__(self):
        return self.name


def _steered_cases():
    """49 cases: case i takes matrix i mod 5 and rounds (i div 5) mod 6 -- the first 30 are every (rounds, matrix) pair once --, the
    steered input i mod 7 and the size (i + i div 7 + 6) mod 7, so every (input, size) pair appears once and case 25 is the largest
    launch, 513 lanes of 27 rounds; each size walks through its positions; the table is entered at 3 i, which puts every entry in front of both powers"""
    matrices, inputs = list(MATRICES), list(STEERED_INPUTS)
    seen, out = {}, []
    for i in range(49):
        matrix, rounds = matrices[i % 5], ROUNDS[(i // 5) % 6]
        label, n = inputs[i % 7], SIZES[(i + i // 7 + 6) % 7]
        where = positions_of(n)
        k_star = where[seen.setdefault(n, 0) % len(where)]
        seen[n] += 1
        name = "%02d-%s-r%d-x=%s-n%d-k%d" % (i, matrix.replace(" ", ""), rounds, label, n, k_star)
        out.append(Case(name, matrix, rounds, STEERED_INPUTS[label], n, k_star, 3 * i, seed=i))
    return out


CASES = _steered_cases()
# the elements of small and two-power order in front of every cube and inverse cube of one lane, under the reference's matrix
STRUCTURED_STEERED = Case("structured-states-reference-r27-n65-k64", "reference", MAX_ROUNDS, STRUCTURED[8], 65, 64, 0, table=STRUCTURED_TABLE, seed=99)
ALL_CASES = CASES + [STRUCTURED_STEERED]
# the group that also runs on a caller's stream: the largest launch, more than one block, one lane, the structured states
STREAM_CASES = [CASES[25]] + [c for c in CASES if c.n in (257, 513) and c is not CASES[25]][:3] + [c for c in CASES if c.n == 1][:1] + [STRUCTURED_STEERED]


class StructuredInputs:
    """The elements of order 2, 4, 11, 37, 407, 2^60, 2^119 and their negatives as INPUTS, under the reference's own parameters at
    27 rounds: the first cube and everything behind it."""
    name, rounds, mds, rc = "structured-inputs", MAX_ROUNDS, REF_MDS, REF_RC
    inputs = list(STRUCTURED)
    n = len(inputs)
    input_bytes = pack(inputs)
    params = pack(REF_MDS + REF_RC) + NOT_A_RESIDUE
    lane_states = [states(x, REF_MDS, REF_RC, MAX_ROUNDS) for x in inputs]
    hash = pack(st[MAX_ROUNDS][0] for st in lane_states)
    trace = pack(row[s] for st in lane_states for s in range(2) for row in st)


# ---- blocks the entries must refuse ---------------------------------------------------------------------------------------------

def refused_blocks(case):
    """(what, params, rounds): each must be SC_ERR_BAD_ARG.  The words are those of `case` with one of them set to p -- the last
    constant read, a matrix entry that is not the first word -- or one round too many (with constants enough for it)."""
    words = case.mds + case.rc
    last = list(words)
    last[-1] = P
    entry = list(words)
    entry[3] = P
    middle = list(words)
    middle[1] = P
    return (("last constant is p", pack(last) + NOT_A_RESIDUE, case.rounds),
            ("matrix entry 3 is p", pack(entry) + NOT_A_RESIDUE, case.rounds),
            ("matrix entry 1 is p", pack(middle) + NOT_A_RESIDUE, case.rounds),
            ("28 rounds", pack(REF_MDS + REF_RC + REF_RC[:4]) + NOT_A_RESIDUE, MAX_ROUNDS + 1))

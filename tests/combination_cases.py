"""Cases of the verifier's combination check at the opened points (csrc/combination.cuh, sc_stark_combination_batch), built from
Python integers by a model of the loop of FastStark.verify written HERE: trace = quotient * zerofier(x) + interpolant(x), the AIR at
(x, trace at x, trace at the successor), the transition quotients, the degree shifts, the weighted sum.  Shared by
tests/test_combination_emu.py (the CPU walk of the kernels) and tests/test_gpu_combination.py (the library's entry)."""
import copy
import ctypes
import functools
import random
import struct

P = 1 + 407 * (1 << 119)
G = 85408008396924667383611388730472331217          # of multiplicative order 2^119 (the reference's generator)
STEP = 4
ACCEPT, REJECT, UNDECIDED = 1, 0, 2
BIG_SHIFT = (1 << 32) + 5

u64, vp = ctypes.c_uint64, ctypes.c_void_p


class Shared(ctypes.Structure):
    """sc_combination_t of include/starkcore.h"""
    _fields_ = [("registers", u64), ("ncons", u64), ("nterms", vp), ("exps", vp), ("coefs", vp), ("generator", u64 * 2), ("omega", u64 * 2),
                ("domain_length", u64), ("step", u64), ("transition_shifts", vp), ("boundary_shifts", vp), ("members", u64), ("weights", vp),
                ("polys", vp), ("pool", vp), ("pool_len", u64)]


def pack(values):
    return b"".join(int(v).to_bytes(16, "little") for v in values)


def unpack(raw):
    return [int.from_bytes(raw[i:i + 16], "little") for i in range(0, len(raw), 16)]


def root_of_unity(n):
    return pow(G, (1 << 119) // n, P)


def horner(coefficients, x):
    acc = 0
    for c in reversed(coefficients):
        acc = (acc * x + c) % P
    return acc


def evaluate(terms, point):
    total = 0
    for exps, coef in terms:
        value = coef
        for e, v in zip(exps, point):
            value = value * pow(v, e, P) % P
        total = (total + value) % P
    return total


class Case:
    """w registers, constraints [[(exponents over 1 + 2 w variables, coefficient)]], members [{weights, zerofiers, interpolants}] (the
    lists per register, lowest degree first), rows [{member, index, claimed, randomizer, zerofier, current[w], next[w]}]"""

    def __init__(self, name, w, constraints, n, transition_shifts, boundary_shifts, members, rows, generator=G, step=STEP):
        self.name, self.w, self.constraints, self.n, self.step = name, w, constraints, n, step
        self.transition_shifts, self.boundary_shifts = transition_shifts, boundary_shifts
        self.members, self.rows = members, rows
        self.generator, self.omega = generator, root_of_unity(n)

    @property
    def nvars(self):
        return 1 + 2 * self.w

    # -- the model -----------------------------------------------------------------------------------
    def point(self, row):
        """[x, trace at x, trace at the successor] of a row whose residues are canonical"""
        member = self.members[row["member"]]
        out = [self.generator * pow(self.omega, row["index"], P) % P]
        for leaves, at in ((row["current"], row["index"]), (row["next"], (row["index"] + self.step) % self.n)):
            x = self.generator * pow(self.omega, at, P) % P
            out += [(leaves[s] * horner(member["zerofiers"][s], x) + horner(member["interpolants"][s], x)) % P for s in range(self.w)]
        return out

    def used(self, row):
        member = self.members[row["member"]]
        return ([row["claimed"], row["randomizer"], row["zerofier"]] + row["current"] + row["next"] + member["weights"] +
                [c for lists in (member["zerofiers"], member["interpolants"]) for coefficients in lists for c in coefficients] + [self.generator, self.omega])

    def verdict(self, row):
        if row["zerofier"] == 0 or any(v >= P for v in self.used(row)):
            return UNDECIDED
        point, weights = self.point(row), iter(self.members[row["member"]]["weights"])
        x = point[0]
        total = row["randomizer"] * next(weights) % P
        for terms, shift in zip(self.constraints, self.transition_shifts):
            quotient = evaluate(terms, point) * pow(row["zerofier"], P - 2, P) % P
            total = (total + quotient * next(weights) + quotient * pow(x, shift, P) * next(weights)) % P
        for s, shift in enumerate(self.boundary_shifts):
            quotient = row["current"][s]
            total = (total + quotient * next(weights) + quotient * pow(x, shift, P) * next(weights)) % P
        return ACCEPT if total == row["claimed"] else REJECT

    def total(self, row):
        """the claimed value that makes the row honest"""
        probe = dict(row, claimed=0)
        point, weights = self.point(probe), iter(self.members[row["member"]]["weights"])
        x = point[0]
        total = row["randomizer"] * next(weights) % P
        for terms, shift in zip(self.constraints, self.transition_shifts):
            quotient = evaluate(terms, point) * pow(row["zerofier"], P - 2, P) % P
            total = (total + quotient * next(weights) + quotient * pow(x, shift, P) * next(weights)) % P
        for s, shift in enumerate(self.boundary_shifts):
            total = (total + row["current"][s] * next(weights) + row["current"][s] * pow(x, shift, P) * next(weights)) % P
        return total

    # -- the entry's arguments -------------------------------------------------------------------------
    def packed_rows(self):
        return b"".join(struct.pack("<QQ", r["member"], r["index"]) + pack([r["claimed"], r["randomizer"], r["zerofier"]] + r["current"] + r["next"])
                        for r in self.rows)

    def tables(self):
        """(nterms, exponent bytes, packed coefficients, packed weights, polys as a flat list, packed pool); equal lists share their
        place in the pool"""
        nterms = [len(terms) for terms in self.constraints]
        exps = bytes(e for terms in self.constraints for k, _ in terms for e in k)
        coefs = pack([v for terms in self.constraints for _, v in terms])
        pool, places, polys = [], {}, []
        for member in self.members:
            for s in range(self.w):
                for coefficients in (member["zerofiers"][s], member["interpolants"][s]):
                    key = tuple(coefficients)
                    if key not in places:
                        places[key] = len(pool)
                        pool += coefficients
                    polys += [places[key] if coefficients else 0, len(coefficients)]
        weights = pack([v for member in self.members for v in member["weights"]])
        return nterms, exps, coefs, weights, polys, pack(pool)

    def shared(self, **overrides):
        """(the C structure, what keeps its buffers alive); overrides: fields of the structure set after it is built"""
        nterms, exps, coefs, weights, polys, pool = self.tables()
        arrays = [(u64 * max(1, len(nterms)))(*nterms), ctypes.create_string_buffer(exps, max(1, len(exps))), ctypes.create_string_buffer(coefs, max(16, len(coefs))),
                  (u64 * max(1, len(self.transition_shifts)))(*self.transition_shifts), (u64 * self.w)(*self.boundary_shifts),
                  ctypes.create_string_buffer(weights, len(weights)), (u64 * len(polys))(*polys), ctypes.create_string_buffer(pool, max(16, len(pool)))]
        at = [ctypes.addressof(a) for a in arrays]
        words = lambda v: (u64 * 2)(v & (2 ** 64 - 1), v >> 64)
        shared = Shared(self.w, len(nterms), at[0], at[1], at[2], words(self.generator), words(self.omega), self.n, self.step, at[3], at[4], len(self.members),
                        at[5], at[6], at[7], len(pool) // 16)
        for field, value in overrides.items():
            setattr(shared, field, value)
        return shared, arrays


def _constraints(rng, nvars, ncons):
    """ncons constraints; the second of three has no terms; exponents up to 5 in one variable, so the plan's Horner walk has steps"""
    out = []
    for c in range(ncons):
        if ncons == 3 and c == 1:
            out.append([])
            continue
        terms = []
        for t in range(rng.randrange(3, 7)):
            exps = [rng.choice([0, 0, 1, 1, 2, 3]) for _ in range(nvars)]
            exps[(c + 1) % nvars] = rng.choice([0, 2, 5])
            terms.append((tuple(exps), rng.choice([1, P - 1, rng.randrange(P)])))
        terms.append(((0,) * nvars, rng.randrange(P)))
        out.append(terms)
    return out


def _member(rng, w, ncons, boundary_points):
    """boundary_points[s]: coefficients of register s's zerofier (that many + 1) and interpolant; 0: no boundary point (zerofier [1],
    interpolant empty)"""
    zerofiers, interpolants = [], []
    for s in range(w):
        k = boundary_points[s]
        zerofiers.append([rng.randrange(P) for _ in range(k)] + [1])
        interpolants.append([rng.randrange(P) for _ in range(k)])
    return {"weights": [rng.randrange(P) for _ in range(1 + 2 * ncons + 2 * w)], "zerofiers": zerofiers, "interpolants": interpolants}


SHAPES = {      # name: (w, ncons, domain length, rows, members)
    "w1_c0_n8_r1": (1, 0, 8, 1, 1),
    "w2_c1_n8_r255": (2, 1, 8, 255, 2),
    "w3_c3_n4096_r256": (3, 3, 1 << 12, 256, 3),
    "w5_c3_n4096_r257": (5, 3, 1 << 12, 257, 2),
    "w2_c3_n4096_r1000": (2, 3, 1 << 12, 1000, 3),
}
NAMES = list(SHAPES)
LARGEST = "w2_c3_n4096_r1000"


@functools.lru_cache(maxsize=None)
def _honest(name):
    w, ncons, n, count, nmembers = SHAPES[name]
    rng = random.Random(name)
    shifts = [0, 1, BIG_SHIFT, 7, 1]
    # members whose lists differ in length: member m's register s has (s + m) % 3 boundary points, register 0 of member 0 none
    members = [_member(rng, w, ncons, [(s + m) % 3 for s in range(w)]) for m in range(nmembers)]
    case = Case(name, w, _constraints(rng, 1 + 2 * w, ncons), n, [shifts[(c + 2) % 5] for c in range(ncons)], [shifts[s % 5] for s in range(w)], members, [])
    special = [n - STEP, 0, n - 1]                      # the successor wraps to 0; the ends of the domain
    for i in range(count):
        row = {"member": rng.randrange(nmembers), "index": special[i] if i < len(special) else rng.randrange(n), "claimed": 0,
               "randomizer": rng.randrange(P), "zerofier": rng.randrange(1, P), "current": [rng.choice([0, 1, P - 1, rng.randrange(P)]) for _ in range(w)],
               "next": [rng.randrange(P) for _ in range(w)]}
        row["claimed"] = case.total(row)
        case.rows.append(row)
    return case


def honest(name):
    """every row's claimed value is the model's total (a fresh copy: callers change it)"""
    return copy.deepcopy(_honest(name))


MUTATIONS = ["claimed_off_by_one", "weight", "coefficient", "list_coefficient", "leaf", "zerofier_leaf_zero", "leaf_is_p"]      # ("coefficient" needs a constraint)


def mutated(name, what):
    """(case, rows that must no longer be accepted -> the verdict they must get)"""
    case = honest(name)
    rows, hit = case.rows, {}
    if what == "claimed_off_by_one":
        for i in range(0, len(rows), 3):
            rows[i]["claimed"] = (rows[i]["claimed"] + 1) % P
            hit[i] = REJECT
    elif what == "weight":
        member = rows[0]["member"]
        weights = case.members[member]["weights"]
        weights[0] = (weights[0] + 1) % P                 # the randomizer's weight: every row of the member has a non-zero randomizer
        hit = {i: REJECT for i, r in enumerate(rows) if r["member"] == member}
    elif what == "coefficient":
        terms = case.constraints[0]                       # the constant term of the first constraint: every transition quotient moves by 1 / leaf
        terms[-1] = (terms[-1][0], (terms[-1][1] + 1) % P)
        hit = {i: REJECT for i in range(len(rows))}
    elif what == "list_coefficient":
        member = rows[0]["member"]
        zerofier = case.members[member]["zerofiers"][case.w - 1]
        zerofier[0] = (zerofier[0] + 1) % P               # the trace value moves by the quotient leaf; whether the AIR sees it the model decides
    elif what == "leaf":
        for i in range(0, len(rows), 2):
            rows[i]["current"][0] = (rows[i]["current"][0] + 1) % P
            hit[i] = REJECT
    elif what == "zerofier_leaf_zero":
        for i in range(0, len(rows), 4):
            rows[i]["zerofier"] = 0
            hit[i] = UNDECIDED
    elif what == "leaf_is_p":
        fields = ["claimed", "randomizer", "zerofier", "current", "next"]
        for i in range(0, len(rows), 2):
            field = fields[(i // 2) % 5]
            if field in ("current", "next"):
                rows[i][field][-1] = P
            else:
                rows[i][field] = P
            hit[i] = UNDECIDED
    else:
        raise KeyError(what)
    return case, hit


@functools.lru_cache(maxsize=None)
def expected(name, what=None):
    """(verdicts, point matrix rows or None for an undecided row) of the model, computed once per case"""
    case = honest(name) if what is None else mutated(name, what)[0]
    verdicts = [case.verdict(r) for r in case.rows]
    points = [case.point(r) if v != UNDECIDED else None for r, v in zip(case.rows, verdicts)]
    return verdicts, points


def rescue_prime_case(count):
    """rows over RescuePrime.transition_constraints (the terms the prover's plan takes), the first two with a wrong claimed value"""
    from algebra import Field
    from rescue_prime import RescuePrime
    rp = RescuePrime()
    constraints = [a.value_domain_terms([1] * 5)[1] for a in rp.transition_constraints(Field.main().primitive_nth_root(1 << 9))]
    constraints = [[(tuple(k), int(v)) for k, v in terms] for terms in constraints]
    rng = random.Random(count)
    w, n = 2, 1 << 11
    members = [_member(rng, w, 2, [2, 1]) for _ in range(2)]
    case = Case("rescue_prime", w, constraints, n, [3, 0], [BIG_SHIFT, 1], members, [])
    for i in range(count):
        row = {"member": i % 2, "index": rng.randrange(n), "claimed": 0, "randomizer": rng.randrange(P), "zerofier": rng.randrange(1, P),
               "current": [rng.randrange(P) for _ in range(w)], "next": [rng.randrange(P) for _ in range(w)]}
        row["claimed"] = (case.total(row) + (1 if i < 2 else 0)) % P
        case.rows.append(row)
    verdicts = [case.verdict(r) for r in case.rows]
    return case, (verdicts, [case.point(r) for r in case.rows])

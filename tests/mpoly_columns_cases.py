"""The cases of sc_mpoly_eval_columns_dev that tests/test_mpoly_columns_emu.py walks on the CPU and tests/test_gpu_mpoly_columns.py runs
through the C ABI: operands laid out as the entry takes them, and the expected results from Python integers (pow(v, e, p)), computed
once per case and shared.

Every case has the same five kinds of constraint where its variables allow them:
  horner   one variable with exponents up to 78 in a list with gaps (drop > 1), repeats (drop == 0) and a non-zero minimum (tail > 0),
           the others 0 ... 5
  tie      two variables reach the same highest exponent 5: the lower index is the Horner variable
  constant a constant only (no Horner variable at all)
  empty    no terms: zeros
  tall     exponents 255, 128 and 0 in one variable (tail == 0)
"""
import functools
import random

P = 1 + 407 * (1 << 119)
SENTINEL = (1 << 128) - 1            # not a residue: no kernel can produce it
ABSENT = 0xFFFFFFFF


def pack(values):
    return b"".join(v.to_bytes(16, "little") for v in values)


def unpack(raw):
    return [int.from_bytes(raw[i:i + 16], "little") for i in range(0, len(raw), 16)]


#        name                 nvars  n  members turned
SHAPES = [("n1_v1_k1", 1, 1, 1, False),
          ("n1_v4_k3", 4, 1, 3, False),
          ("n3_v2_k1", 2, 3, 1, False),
          ("n3_v6_k3", 6, 3, 3, False),
          ("n256_v3_k1", 3, 256, 1, False),
          ("n256_v5_k3", 5, 256, 3, False),
          ("n257_v6_k1", 6, 257, 1, False),
          ("n257_v4_k3", 4, 257, 3, False),
          ("n2_v3_k1_turned", 3, 2, 1, True),
          ("n2_v6_k3_turned", 6, 2, 3, True),
          ("n512_v5_k1_turned", 5, 512, 1, True),
          ("n512_v4_k3_turned", 4, 512, 3, True)]
NAMES = [s[0] for s in SHAPES]
MANY_PAIRS = "n1_v2_k32769_pairs_above_one_launch"       # members * ncons = 65 538 > 65 535 rows of a grid


class Case:
    """buf: the value buffer (bytes, 16 per element, sentinels wherever no stored variable lies); var_base / var_ld / var_src /
    var_rot / nterms: lists; exps / coefs: bytes; values[m][j]: variable j's n values for member m (None: absent);
    constraints[c]: [(exponents, coefficient)]; expected[m][c]: n integers; pad: ld_out - n"""


def _constraints(rng, nvars, usable):
    """the five kinds over the usable variables (indices), as [(exponent tuple, coefficient)]"""
    def term(fixed, low=0, high=5):
        e = [0] * nvars
        for j in usable:
            e[j] = rng.randint(low, high)
        for j, v in fixed.items():
            e[j] = v
        return tuple(e)
    coefficient = lambda: rng.choice([1, P - 1, rng.randrange(1, P), rng.randrange(1, P)])
    big = usable[len(usable) // 2]
    horner = [(term({big: e}), coefficient()) for e in (40, 78, 3, 77, 40, 3, 78, 12)]       # unsorted, with repeats and gaps; minimum 3
    horner.append((term({big: 50}), 0))                                                          # a zero coefficient is a term like any other
    if len(usable) >= 2:
        a, b = usable[0], usable[-1]
        tie = [(term({a: 5, b: 2}), coefficient()), (term({a: 1, b: 5}), coefficient()), (term({a: 0, b: 0}), coefficient()), (term({a: 5, b: 5}), coefficient())]
    else:
        tie = [(term({usable[0]: 5}), coefficient()), (term({usable[0]: 5}), coefficient())]
    constant = [((0,) * nvars, rng.randrange(1, P))]
    tall_var = usable[-1]
    tall = [(term({tall_var: e}, 0, 1), coefficient()) for e in (128, 255, 0)]
    return [horner, tie, constant, [], tall]


def _build(name, nvars, n, members, turned, seed, constraints=None):
    rng = random.Random(seed)
    case = Case()
    case.name, case.nvars, case.n, case.members = name, nvars, n, members
    # roles: variable 0 is shared by all members (X) when there are two or more, the last one is absent when there are four or
    # more, and with `turned` the one before the absent one (or the last) is read off variable 1 (or 0), three places on
    role = ["stored"] * nvars
    if nvars >= 2:
        role[0] = "shared"
    if nvars >= 4:
        role[-1] = "absent"
    source = None
    if turned:
        at = nvars - 2 if nvars >= 4 else nvars - 1
        source = 1 if at > 1 else 0
        role[at] = "turned"
    case.role = role
    usable = [j for j in range(nvars) if role[j] != "absent"]
    case.constraints = constraints if constraints is not None else _constraints(rng, nvars, usable)
    # the buffer: shared rows and per-member matrices (row stride above n) one after the other, gaps in between
    elements, var_base, var_ld, rows = [], [0] * nvars, [0] * nvars, {}
    special = [0, 1, P - 1]
    for j in range(nvars):
        if role[j] in ("absent", "turned"):
            var_base[j], var_ld[j] = 1 << 40, 1 << 40             # never read
            continue
        elements += [SENTINEL] * rng.randint(0, 3)
        var_base[j] = len(elements)
        count = 1 if role[j] == "shared" else members
        var_ld[j] = 0 if role[j] == "shared" else n + rng.randint(0, 2)
        for m in range(count):
            row = [rng.randrange(P) for _ in range(n)]
            row[rng.randrange(n)] = special[(j + m) % 3]
            rows[(j, m)] = row
            elements += row + [SENTINEL] * (var_ld[j] - n if count > 1 or var_ld[j] else 0)
    elements += [SENTINEL] * 2
    case.buf = pack(elements)
    case.var_base, case.var_ld = var_base, var_ld
    rot = 3
    if turned:
        case.var_src = [ABSENT if r == "absent" else (source if r == "turned" else j) for j, r in enumerate(role)]
        case.var_rot = [rot if r == "turned" else 0 for r in role]
    elif "absent" in role:
        case.var_src = [ABSENT if r == "absent" else j for j, r in enumerate(role)]
        case.var_rot = [0] * nvars
    else:
        case.var_src = case.var_rot = None
    case.values = []
    for m in range(members):
        per = []
        for j, r in enumerate(role):
            if r == "absent":
                per.append(None)
            elif r == "turned":
                src = rows[(source, 0 if role[source] == "shared" else m)]
                per.append([src[(i + rot) % n] for i in range(n)])
            else:
                per.append(rows[(j, 0 if r == "shared" else m)])
        case.values.append(per)
    case.nterms = [len(c) for c in case.constraints]
    case.exps = bytes(e for c in case.constraints for k, _ in c for e in k)
    case.coefs = pack([v for c in case.constraints for _, v in c])
    case.pad = 1 + seed % 3
    case.expected = [[[_evaluate(c, per, i) for i in range(n)] for c in case.constraints] for per in case.values]
    return case


def _evaluate(terms, per, i):
    total = 0
    for k, coefficient in terms:
        product = coefficient
        for j, e in enumerate(k):
            if e:
                product = product * pow(per[j][i], e, P) % P
        total += product
    return total % P


@functools.lru_cache(maxsize=None)
def case(name):
    if name == MANY_PAIRS:
        constraints = [[((2, 1), 5), ((0, 3), P - 1), ((0, 0), 7)], [((1, 0), 1), ((4, 4), 3)]]
        return _build(name, 2, 1, 32769, False, 99, constraints)
    index = NAMES.index(name)
    return _build(*SHAPES[index], seed=100 + index)


def horner_variable(terms, nvars):
    """the used variable with the largest maximum exponent, the lowest index on a tie; None: no variable is used"""
    tops = [max((k[j] for k, _ in terms), default=0) for j in range(nvars)]
    best = max(tops, default=0)
    return tops.index(best) if best else None


def products(terms, nvars):
    """(the plan's products per point: max e_h + the other variables' exponents, the term-by-term count: all exponents)"""
    h = horner_variable(terms, nvars)
    flat = sum(sum(k) for k, _ in terms)
    if h is None:
        return 0, flat
    return max(k[h] for k, _ in terms) + sum(sum(k) - k[h] for k, _ in terms), flat

"""The operands the division tests share (tests/test_poly_divide_model.py on the host, tests/test_gpu_poly_divide.py on the device):
for every shape (m, nb) -- m quotient coefficients, a divisor of nb coefficients, so a numerator of na = m + nb - 1 -- one list of
(label, a, b) with a of na and b of nb canonical residues and b[nb-1] != 0.  Test-only."""
from oracle import py_oracle as po
import synth

P = po.P
M_GRID = (1, 2, 3, 4, 5, 31, 32, 33, 64, 65)
NB_GRID = (1, 2, 3, 31, 32, 33, 100)
EDGES = (0, 1, P - 1, 1 << 64, (1 << 119) + 1)


def _nonzero_top(values):
    values[-1] = values[-1] or 1
    return values


def operands(m, nb):
    na = m + nb - 1
    seed = 7000 + 131 * m + nb
    a = synth.synth_ints(seed, na)
    b = _nonzero_top(synth.synth_ints(seed + 1, nb))
    out = [("general", a, b)]
    out.append(("leading p-1", a, b[:-1] + [P - 1]))
    out.append(("leading 2", a, b[:-1] + [2]))
    if nb > 1:
        out.append(("zero constant term", a, [0] + b[1:]))
    out.append(("monomial", a, [0] * (nb - 1) + [1]))
    out.append(("numerator with two zero top coefficients", a[:max(na - 2, 0)] + [0] * min(2, na), b))
    q = synth.synth_ints(seed + 2, m)
    exact = po.schoolbook_mul(q, b)
    assert len(exact) == na
    out.append(("exact product", exact, b))
    if m == 1:
        out.append(("a == b", list(b), b))
    ea = [EDGES[(i + m) % 5] if i % 3 == 0 else v for i, v in enumerate(a)]
    eb = [EDGES[(i + nb) % 5] if i % 2 == 0 else v for i, v in enumerate(b)]
    eb[-1] = eb[-1] or P - 1
    out.append(("edge residues", ea, eb))
    return out


def expected(a, b):
    """(q, r) of po.schoolbook_divmod in the device's lengths: len(a) - len(b) + 1 and len(b) - 1 coefficients (the oracle sizes the
    quotient by the numerator's DEGREE and keeps the whole running remainder, whose entries from len(b) - 1 on are zero)"""
    m, nr = len(a) - len(b) + 1, len(b) - 1
    q, r = po.schoolbook_divmod(a, b)
    assert len(q) <= m and not any(r[nr:])
    return q + [0] * (m - len(q)), (r + [0] * nr)[:nr]

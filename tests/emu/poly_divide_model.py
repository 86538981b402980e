"""Executable model of the device algorithm behind sc_poly_divmod* (csrc/polydiv.cuh, polydiv_columns in csrc/polytree_geo.hip):
division with remainder of code/univariate.py:80-97 through the reversed polynomials.

The reference subtracts one multiple of the divisor per quotient coefficient; quotient and remainder are unique, so the device is
free to compute them another way.  For a of na and b of nb coefficients, b[nb-1] != 0, m = na - nb + 1:

  1. h = rev(b)^-1 mod y^m: h_0 = 1 / b[nb-1], then Newton steps h <- h (2 - G h) that double the precision up to P = 2^ceil(log2 m),
     the step from `have` to 2 * have coefficients at transform size 4 * have; only G = rev(b)[0 .. min(nb, m)) is ever loaded;
  2. rev(q) = rev(a)[0..m) * h[0..m) mod y^m at transform size n2 = 2^ceil(log2(2m - 1)) (at least 2);
  3. r = (a - q b) mod (x^n3 - 1), first nb - 1 entries, n3 = 2^ceil(log2 nb) (at least 2): q and a folded to n3 entries, one cyclic
     product at the divisor's size.

Every array operation below corresponds to one kernel launch or transform of the device code, with the same truncation lengths
(`in_limit`) and transform sizes.  Test-only.
"""
from oracle import py_oracle as po

P = po.P


def _log2_ceil(n):
    return max(0, (n - 1).bit_length())


def shape(na, nb):
    """PolyDivShape: (m, nr, g, logP, log2, log3)"""
    m = na - nb + 1
    return m, nb - 1, min(nb, m), _log2_ceil(m), max(1, _log2_ceil(2 * m - 1)), max(1, _log2_ceil(nb))


def transform(values, limit, n, inverse=False):
    """ntt_device at size n with in_limit = limit: the input behind `limit` reads as zero; the inverse does not scale"""
    padded = [v % P for v in values[:limit]] + [0] * (n - min(limit, len(values)))
    if inverse:
        return [v * n % P for v in po.intt(po.primitive_nth_root(n), padded)]
    return po.ntt(po.primitive_nth_root(n), padded)


def inverse_series(b, na):
    """polydiv_inverse_series: the buffer h of 2P entries (P >= m of them valid; a constant divisor: one entry)"""
    nb = len(b)
    m, _, g, logP, _, _ = shape(na, nb)
    h = [po.inv(b[nb - 1])] + [0] * (2 * (1 << logP) - 1)           # pt_fill_kernel on entry 0 (the zeros are never read)
    if nb == 1:
        return h
    G = [b[nb - 1 - t] for t in range(g)]                           # pd_rev_kernel
    for lm in range(logP):
        have, n = 1 << lm, 4 << lm
        H = transform(h, have, n)
        T = transform(G, min(2 * have, g), n)
        ninv = po.inv(n)
        H = [ninv * x * ((2 - t * x) % P) % P for x, t in zip(H, T)]   # pt_newton_kernel (carries the inverse transform's n^-1)
        h[:n] = transform(H, n, n, inverse=True)
    return h


def divmod_model(a, b, want_q=True, want_r=True):
    """(q, r) as sc_poly_divmod_dev stores them: na - nb + 1 and nb - 1 coefficients (None for an output not asked for)"""
    na, nb = len(a), len(b)
    assert nb >= 1 and na >= nb and b[nb - 1] % P != 0
    m, nr, g, logP, log2, log3 = shape(na, nb)
    n2, n3 = 1 << log2, 1 << log3
    h = inverse_series(b, na)
    Hf = transform(h, 1 if nb == 1 else m, n2)
    X = [a[na - 1 - t] for t in range(m)]                            # pd_rev_kernel: rev(a)[0..m)
    Y = transform(X, m, n2)
    c = po.inv(n2)
    Y = [c * y * t % P for y, t in zip(Y, Hf)]                       # pd_mul_tab_kernel
    X = transform(Y, n2, n2, inverse=True)                           # X[0..m) = rev(q)
    q = [X[m - 1 - i] for i in range(m)]
    if not (want_r and nr):
        return (q if want_q else None), ([] if want_r else None)    # pd_rev_kernel stores q
    nf = min(m, n3)
    fold = [sum(X[m - 1 - i] for i in range(j, m, n3)) % P for j in range(nf)]   # pd_fold_rev_kernel (stores q on the way)
    Bf = transform(b, nb, n3)
    Z = transform(fold, nf, n3)
    c = po.inv(n3)
    Z = [c * z * t % P for z, t in zip(Z, Bf)]                       # pd_mul_tab_kernel
    prod = transform(Z, n3, n3, inverse=True)
    r = [(sum(a[i] for i in range(j, na, n3)) - prod[j]) % P for j in range(nr)]   # pd_remainder_kernel
    return (q if want_q else None), r

"""Executable model of the COLUMN forms of the subproduct-tree kernels (csrc/polytree.cuh, the *_cols kernels behind
sc_polytree_evaluate_columns_dev / sc_polytree_interpolate_columns_dev), on top of polytree_model.Tree.

A set of C' = 2^logC columns goes through the tree with the column index INNERMOST: a level is the flat array [2^l][K >> l][C'],
so its transform is the same column transform with a batch of (K >> l) * C', "the first K entries" become the first K * C', and
every elementwise step indexes the tree's own tables (Zf, the inverse series, the weights) by flat >> logC and the data by flat.
Each function below is one kernel, written thread by thread over the flat index with the kernel's own index arithmetic; lanes
c >= cols of a set are padding (loaded as zeros, never stored).  Test-only.
"""
from oracle import py_oracle as po

import polytree_model as pm

P = po.P


def lanes_log(cols):
    """log2 of the lanes of a set that holds `cols` columns: the power of two >= cols"""
    return (cols - 1).bit_length() if cols > 1 else 0


def rev_poly_cols(columns, m, K, logC, total):
    """pt_rev_poly_cols_kernel: F[t][c] = f_c[K-1-t] for t < K, zero above and where the column has no such coefficient"""
    mask = (1 << logC) - 1
    F = [0] * total
    for i in range(total):
        t, c = i >> logC, i & mask
        if t < K and K - 1 - t < m and c < len(columns):
            F[i] = columns[c][K - 1 - t] % P
    return F


def mul_tab_cols(a, tab, logC):
    """pt_mul_tab_cols_kernel (without the transform's n^-1, which the model's intt applies)"""
    return [a[i] * tab[i >> logC] % P for i in range(len(a))]


def corr_cols(C, zf, n, logB2, logC):
    """pt_corr_cols_kernel on [n][B][C'] and the tree's [n][2B]"""
    mask, bmask = (1 << logC) - 1, (1 << logB2) - 1
    D = [0] * (n << (logB2 + logC))
    for t in range(len(D)):
        c, u = t & mask, t >> logC
        f, i = u >> logB2, u & bmask
        nf = (n - f) & (n - 1)
        D[t] = C[(((f << (logB2 - 1)) + (i >> 1)) << logC) + c] * zf[(nf << logB2) + (i ^ 1)] % P
    return D


def expand_cols(a, half):
    """pt_expand_cols_kernel: [n][B][C'] -> [2n][B][C'], zeros above"""
    return [a[i] if i < half else 0 for i in range(2 * half)]


def comb_cols(Ph, zf, total_out, logC):
    """pt_comb_cols_kernel"""
    mask = (1 << logC) - 1
    E = [0] * total_out
    for i in range(total_out):
        c, u = i & mask, i >> logC
        pl, pr = Ph[((2 * u) << logC) + c], Ph[((2 * u + 1) << logC) + c]
        E[i] = (pl * zf[2 * u + 1] + pr * zf[2 * u]) % P
    return E


def weights_cols(columns, winv, k, logC, total):
    """pt_weights_cols_kernel: W[i][c] = v_c[i] / Z'(d_i), zero on padding leaves and padding lanes"""
    mask = (1 << logC) - 1
    W = [0] * total
    for t in range(total):
        i, c = t >> logC, t & mask
        if i < k and c < len(columns):
            W[t] = columns[c][i] * winv[i] % P
    return W


def store_cols(src, logC, off, k, cols):
    """pt_store_cols_kernel: column c's k entries from row `off` on"""
    out = [[0] * k for _ in range(cols)]
    for t in range(k * cols):
        c = t // k
        i = t - c * k
        out[c][i] = src[((off + i) << logC) + c]
    return out


def horner_cols(acc, y, e, logC, k):
    """pt_horner_cols_kernel: acc_c[i] = acc_c[i] * y[i] + e[i][c]"""
    for t in range(k * len(acc)):
        c = t // k
        i = t - c * k
        acc[c][i] = (acc[c][i] * y[i] + e[(i << logC) + c]) % P
    return acc


class ColumnTree(pm.Tree):
    def __init__(self, points):
        super().__init__(points)
        self.points = [x % P for x in points]
        self.winv = None

    def _evaluate_all_cols(self, columns, m, logC):
        """polytree_evaluate_all_cols: the values at all K leaves, interleaved [K][C']"""
        K, L = self.K, self.L
        if L == 0:
            return rev_poly_cols(columns, m, K, logC, K << logC)
        by = rev_poly_cols(columns, m, K, logC, (2 * K) << logC)
        bx = pm.ntt_cols(by, 2 * K, 1 << logC)
        invg_f = pm.ntt_cols(self._inverse_series() + [0] * K, 2 * K, 1)
        bx = mul_tab_cols(bx, invg_f, logC)
        by = pm.ntt_cols(bx, 2 * K, 1 << logC, inverse=True)
        for l in range(L, 0, -1):
            n, logB = 1 << l, L - l
            tk = pm.ntt_cols(by[:K << logC], n, 1 << (logB + logC))
            bx = corr_cols(tk, self.Zf[l - 1], n, logB + 1, logC)
            by = pm.ntt_cols(bx, n, 1 << (logB + 1 + logC), inverse=True)
        return by[:K << logC]

    def evaluate_columns(self, columns, m):
        """columns: `cols` coefficient lists of m entries each (any m: chunks of K, Horner over x^K) -> `cols` lists of k values"""
        k, K = self.k, self.K
        cols, logC = len(columns), lanes_log(len(columns))
        chunks = (m + K - 1) // K if m > K else 1
        y = [pow(x, K, P) for x in self.points]
        out = None
        for j in reversed(range(chunks)):
            length = m - j * K if j == chunks - 1 else K
            by = self._evaluate_all_cols([c[j * K:] for c in columns], length, logC)
            out = store_cols(by, logC, 0, k, cols) if j == chunks - 1 else horner_cols(out, y, by, logC, k)
        return out

    def _weights(self):
        if self.winv is None:
            zr = self.zerofier()
            der = [(t + 1) * zr[t + 1] % P for t in range(self.k)]
            e = self.evaluate(der)
            assert all(x != 0 for x in e), "divide by zero"
            self.winv = [po.inv(x) for x in e]
        return self.winv

    def interpolate_columns(self, columns):
        """columns: `cols` lists of k values -> `cols` lists of k coefficients"""
        k, K, L, pad = self.k, self.K, self.L, self.pad
        cols, logC = len(columns), lanes_log(len(columns))
        half = K << logC
        if L == 0:
            cur = rev_poly_cols(columns, 1, K, logC, half)
        else:
            cur = weights_cols(columns, self._weights(), k, logC, half)
        for l in range(L):
            bx = expand_cols(cur, half)
            by = pm.ntt_cols(bx, 2 << l, 1 << (L - l + logC))
            bx = comb_cols(by, self.Zf[l], half, logC)
            cur = pm.ntt_cols(bx, 2 << l, 1 << (L - l - 1 + logC), inverse=True)
        return store_cols(cur, logC, pad, k, cols)

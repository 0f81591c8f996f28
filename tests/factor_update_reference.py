"""50-digit reference of the rank-one step of the proposal factor (TAMCMC_OPT_FACTOR_REFRESH; csrc/factor_update.h), on the Decimal
algebra of tests/sampler_reference.py.  It shares no line with csrc/.

    rank_one(L, w, beta2)     the exact lower Cholesky factor of  M = beta2 L L^T + w w^T,  M formed in Decimal from the double inputs and
                              factored by the algorithm of sampler_reference.cholesky (cholesky_exact is that algorithm on Decimal
                              entries: R.cholesky itself converts its input from double; test_factor_update.py holds the two against
                              each other on double matrices), with the rounding bound of a computed update
    closed_form(L, w, beta2)  L G with G = chol(beta2 I + p p^T), p = L^-1 w, written from its formula: the formulation the product uses
    law_matrix(...)           sigma (Sigma + eps2 rho I), rho = prod (1 - g_j): the law of the factor after rank-one steps with gains g_j

The rounding bound, in Higham's form (the way tests/test_sampler_reference.py writes the factorisation's): the computed factor L^ has
L^ L^^T = M + dM, and to first order |dL| <= |L'| tril(|L'^-1| |dM| |L'^-T|) with L' the exact factor.  dM counts the roundings of the
formulation that was built -- solve, then scale (u = 2^-53, n the size; nothing below is fitted to a result):

  solve     p^ solves (L + dL) p^ = w, |dL| <= (n + 2) u |L|: row i is a sum of at most n terms, the product with the reciprocal pivot
            adds two roundings.  The update then factors beta2 L L^T + (L p^)(L p^)^T, and L p^ = w - dL p^, so to first order
                |dM_1| <= K1 u S1,   K1 = n + 2,   S1 = |w| q^T + q |w|^T,   q = |L| |p|
  scale     alpha_k = beta2 + sum_{j<=k} p_j^2 is a sum of at most n + 1 positive terms, each a rounded square: relative error
            (n + 2) u.  t = beta / sqrt(alpha_k alpha_k-1): the square root halves the two alphas' errors ((n + 2) u together); beta,
            the product, its root and the division add four roundings: (n + 6) u.  b_k = p_k t: (n + 7) u.  a_k = alpha_k t carries
            alpha_k's error once more: (2 n + 9) u.  Taken as |dG| <= (2 n + 10) u |G|.  L' = L G:
                |dM_2| <= 2 (2 n + 10) u |L| |G| |G|^T |L|^T
  sweep     L'_ik = L_ik a_k + s_ik b_k with s_ik a sum of at most n products, then two products and a sum: n + 2 roundings on
            (|L| |G|)_ik; the error enters M from either side: |dM_3| <= 2 (n + 2) u |L| |G| |G|^T |L|^T
                |dM_2| + |dM_3| <= K2 u S2,   K2 = 6 n + 24,   S2 = |L| |G| |G|^T |L|^T
  inputs    (an engine's step only) w = sqrt(g sigma') (x - mu') and beta2 = (1 - g) sigma' / sigma are formed in double from the
            doubles the test reads: g one rounding, the product and its square root two, the deviation one, the product with it one --
            5 u relative on w, 10 u on w w^T; beta2 four roundings beside g's, whose error (1 - g) magnifies by g / (1 - g) <= 1 for
            g <= 1/2: 6 u.  Since S2 >= |w| |w|^T + beta2 |L| |L|^T element by element, K_IN = 16 on S2 covers both.  The tests'
            gains are c0 / (1 + i) <= 2 / 51.

Everything on the right is the reference's own: p, G, L' from the exact computation, rounded to double for the scales (which need two
digits, not fifty: sampler_reference.py).  A comparison is |got - ref| <= 1.01 bound (the first-order form, as in
test_sampler_reference.py).
"""
from decimal import Decimal

import numpy as np

import sampler_reference as R

U = 2.0 ** -53
K_IN = 16


def K1(n):
    return n + 2


def K2(n):
    return 6 * n + 24


def cholesky_exact(M):
    """sampler_reference.cholesky on Decimal entries (rows of the lower triangle at least); None when a pivot is <= 0."""
    n = len(M)
    with R._ctx():
        L = []
        for i in range(n):
            ai = M[i]
            row = []
            for j in range(i):
                lj = L[j]
                s = ai[j]
                for k in range(j):
                    s -= row[k] * lj[k]
                row.append(s / lj[j])
            d = ai[i]
            for k in range(i):
                d -= row[k] * row[k]
            if not d > 0:
                return None
            row.append(d.sqrt())
            L.append(row)
    return L


def matrix(L, w, beta2):
    """Lower triangle of beta2 L L^T + w w^T in Decimal, from the doubles L (its lower triangle), w, beta2."""
    n = len(w)
    with R._ctx():
        Ld = [[R.dec(L[i][k]) for k in range(i + 1)] for i in range(n)]
        wd = [R.dec(v) for v in w]
        b2 = R.dec(beta2)
        M = []
        for i in range(n):
            li = Ld[i]
            row = []
            for j in range(i + 1):
                lj = Ld[j]
                s = R.ZERO
                for k in range(j + 1):
                    s += li[k] * lj[k]
                row.append(b2 * s + wd[i] * wd[j])
            M.append(row)
    return M


def solve(L, w):
    """p = L^-1 w in Decimal from the doubles."""
    n = len(w)
    with R._ctx():
        Ld = [[R.dec(L[i][k]) for k in range(i + 1)] for i in range(n)]
        return R.solve_lower(Ld, [R.dec(v) for v in w])


def g_factor(p, beta2):
    """G = chol(beta2 I + p p^T) from its closed form (Decimal rows): alpha_k = beta2 + sum_{j<=k} p_j^2, alpha_-1 = beta2,
    G_kk = beta sqrt(alpha_k / alpha_k-1), G_ik = beta p_i p_k / sqrt(alpha_k alpha_k-1)."""
    n = len(p)
    with R._ctx():
        b2 = R.dec(beta2)
        beta = b2.sqrt()
        alpha, prev = [], b2
        for v in p:
            prev = prev + v * v
            alpha.append(prev)
        G = []
        for i in range(n):
            row = []
            for k in range(i + 1):
                ap = alpha[k - 1] if k else b2
                if k == i:
                    row.append(beta * (alpha[k] / ap).sqrt())
                else:
                    row.append(beta * p[i] * p[k] / (alpha[k] * ap).sqrt())
            G.append(row)
    return G


def closed_form(L, w, beta2):
    """L G, Decimal rows."""
    n = len(w)
    G = g_factor(solve(L, w), beta2)
    with R._ctx():
        return [[sum((R.dec(L[i][j]) * G[j][k] for j in range(k, i + 1)), R.ZERO) for k in range(i + 1)] for i in range(n)]


class Update:
    """L: the exact factor (Decimal rows); Lf: rounded to double; S1, S2: the matrices of the bound (float); dM(k_in), bound(k_in): the
    bound on the matrix and on the factor, element by element (float), k_in = K_IN for an engine's step, 0 for exact inputs."""

    def dM(self, k_in=0):
        return U * (K1(self.n) * self.S1 + (K2(self.n) + k_in) * self.S2)

    def bound(self, k_in=0):
        Li = R.abs_inverse(self.Lf)
        return np.abs(self.Lf) @ np.tril(Li @ self.dM(k_in) @ Li.T)


def magnitudes(Lf, w, beta2):
    """(S1, S2) in float64 from the double factor before the step: the scales need two digits."""
    Lf = np.tril(np.asarray(Lf, dtype=np.float64))
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    p = np.zeros(n)
    for i in range(n):
        p[i] = (w[i] - Lf[i, :i] @ p[:i]) / Lf[i, i]
    alpha = beta2 + np.cumsum(p * p)
    ap = np.concatenate(([beta2], alpha[:-1]))
    t = np.sqrt(beta2) / np.sqrt(alpha * ap)
    G = np.tril(np.outer(p, p * t), -1) + np.diag(alpha * t)
    q = np.abs(Lf) @ np.abs(p)
    S1 = np.outer(np.abs(w), q) + np.outer(q, np.abs(w))
    LG = np.abs(Lf) @ np.abs(G)
    return S1, LG @ LG.T


def rank_one(L, w, beta2):
    """The exact factor of beta2 L L^T + w w^T from the double inputs, with its bound; None when the matrix has a pivot <= 0."""
    Lx = cholesky_exact(matrix(L, w, beta2))
    if Lx is None:
        return None
    out = Update()
    out.n = len(w)
    out.L = Lx
    out.Lf = R.factor_float(Lx)
    out.S1, out.S2 = magnitudes(L, w, beta2)
    return out


def ratio(got, upd, k_in=0):
    """max over the lower triangle of |got - exact| / (1.01 bound); got: the doubles of a computed factor."""
    n = upd.n
    b = 1.01 * upd.bound(k_in)
    worst = 0.0
    with R._ctx():
        for i in range(n):
            for k in range(i + 1):
                diff = abs(R.dec(got[i][k]) - upd.L[i][k])
                if diff == 0:
                    continue
                if b[i, k] == 0.0 or not np.isfinite(got[i][k]):
                    return float("inf")
                worst = max(worst, float(diff / R.dec(b[i, k])))
    return worst


def law_matrix(cov, sigma, eps2, gains):
    """sigma (Sigma + eps2 rho I) in Decimal (full rows), rho = prod (1 - g_j) over the rank-one steps since the last full step."""
    n = len(cov)
    with R._ctx():
        rho = R.ONE
        for g in gains:
            rho *= R.ONE - (g if isinstance(g, Decimal) else R.dec(g))
        s, e = R.dec(sigma), R.dec(eps2) * rho
        return [[s * (R.dec(cov[i][j]) + (e if i == j else R.ZERO)) for j in range(n)] for i in range(n)], rho

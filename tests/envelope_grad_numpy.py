"""Long-double numpy gradient of S(theta) = sum_i (y_i / M_i + ln M_i) for the Gaussian-envelope fits (ids 0, 1): the yardstick of
tests/test_gpu_envelope_gradient.py above the sizes the 50-digit reference (tests/envelope_grad_reference.py) is run at, and the budget
B_j of every component.  tests/test_envelope_gradient.py holds this yardstick to the 50-digit reference.

The formulas are those of include/tamcmc_hip.h (tamcmc_hip_envelope_gradient_sums): per bin the derivative of M with respect to each ROW
QUANTITY, then the chain rule to the parameters.  With W_i = 1/M_i + 2 y_i/M_i^2 (what a relative error of M costs the term r_i dM_i) and M
stated to 1e-12 per bin,
    B_j = 1e-12 sum_q |J_qj| sum_i |dM_i/drow_q| W_i      (q: the chain-rule branches of theta_j).
Conventions as in the header: d|p|/dp = copysign(1, p); a bin adds 0 to the lna / pw / ln b / c sums where D = 0 or its ln x term is not
finite; pw = 0 gives L = 1/2; the tc of a switched-off Harvey term has no finite component (NaN here)."""
import numpy as np

LD = np.longdouble
NROW = 13


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _logistic(expo, u):
    """L = 1 / (1 + exp(expo u)) with (.)^0 = 1 also where u is not finite, and D = L (1 - L)."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.ones_like(u) if expo == 0 else np.exp(expo * u)
        L = LD(1) / (LD(1) + e)
        D = np.where(e < 1, L * (e * L), L * (LD(1) - L))
    return L, D


def _guard(D, u):
    """D and D u with the bins the convention leaves out set to exactly 0."""
    live = (D != 0) & np.isfinite(u)
    with np.errstate(invalid="ignore"):
        return np.where(live, D, LD(0)), np.where(live, D * np.where(live, u, LD(0)), LD(0))


def _sgn(v):
    return LD(np.copysign(1.0, float(v)))


def row_derivatives(model_id, params, x):
    """(M [Nx], dM [13 x Nx] = dM_i/d(row quantity q), J [13 x Np] = d(row quantity)/d(parameter)), long double."""
    p, x = _ld(params), _ld(x)
    n = x.size
    with np.errstate(divide="ignore"):
        lx = np.log(x)
    dM = np.zeros((NROW, n), dtype=LD)
    if model_id == 1:
        J = np.zeros((NROW, 10), dtype=LD)
        A, nu, s2, N0 = np.abs(p[7]), p[8], np.abs(p[9]) ** 2, np.abs(p[6])
        d = x - nu
        g = np.exp(LD(-0.5) * d * d / s2)
        M = A * g
        dM[0], dM[1], dM[2], dM[3] = g, A * g * d / s2, A * g * d * d / (2 * s2 * s2), LD(1)
        J[0, 7], J[1, 8], J[2, 9], J[3, 6] = _sgn(p[7]), 1, 2 * p[9], _sgn(p[6])
        for q in range(2):
            Hq, tc, pw = np.abs(p[3 * q]), np.abs(p[3 * q + 1]), np.abs(p[3 * q + 2])
            J[4 + q, 3 * q], J[8 + q, 3 * q + 2] = _sgn(p[3 * q]), _sgn(p[3 * q + 2])
            if tc == 0:
                J[6 + q, 3 * q + 1] = LD(np.nan)
                continue
            J[6 + q, 3 * q + 1] = LD(1) / p[3 * q + 1]
            u = np.log(LD(1e-3) * tc) + lx
            L, D = _logistic(pw, u)
            D0, Du = _guard(D, u)
            M = M + Hq * L
            dM[4 + q], dM[6 + q], dM[8 + q] = L, -Hq * D0 * pw, -Hq * Du
        return M + N0, dM, J
    J = np.zeros((NROW, 19), dtype=LD)
    A, nu, s2, N0, mu = np.abs(p[14]), np.abs(p[15]), np.abs(p[16]) ** 2, np.abs(p[13]), p[17]
    s15 = _sgn(p[15])
    xn = x.max()
    a = LD(0.5) * LD(np.pi) * x / xn
    with np.errstate(invalid="ignore", divide="ignore"):
        eta2 = (np.sin(a) / a) ** 2
    if x[0] == 0:
        eta2[0] = 1
    d = x - nu
    g = eta2 * np.exp(LD(-0.5) * d * d / s2)
    M = A * g + N0
    dM[0], dM[1], dM[2], dM[3] = g, A * g * d / s2, A * g * d * d / (2 * s2 * s2), LD(1)
    J[0, 14], J[1, 15], J[2, 16], J[3, 13] = _sgn(p[14]), s15, 2 * p[16], _sgn(p[13])
    a2 = [(p[0] * nu ** p[1]) ** 2, p[5] ** 2, p[6] ** 2]
    J[4, 0], J[4, 1], J[4, 15] = 2 * p[0] * nu ** (2 * p[1]), a2[0] * 2 * np.log(nu), a2[0] * 2 * p[1] / nu * s15
    J[5, 5], J[6, 6] = 2 * p[5], 2 * p[6]
    nm = nu + mu
    h = x[1] - x[0]
    w = np.ones(n, dtype=LD)
    w[0] = w[-1] = LD(0.5)
    for k, (i, j, ic) in enumerate(((2, 3, 4), (7, 8, 9), (10, 11, 12))):
        with np.errstate(divide="ignore"):
            lnb = np.log(np.abs(p[i])) + p[j] * np.log(np.abs(nm))
        c = np.abs(p[ic])
        J[7 + k, i], J[7 + k, j], J[7 + k, 15], J[7 + k, 17] = LD(1) / p[i], np.log(np.abs(nm)), p[j] / nm * s15, p[j] / nm
        J[10 + k, ic] = _sgn(p[ic])
        u = lx - lnb
        L, D = _logistic(c, u)
        D0, Du = _guard(D, u)
        I, Ib, Ic = np.sum(w * L), np.sum(w * c * D0), -np.sum(w * Du)
        Ck = a2[k] / (h * I)
        M = M + Ck * L
        dM[4 + k] = L / (h * I)
        dM[7 + k] = Ck * (c * D0 - L * Ib / I)
        dM[10 + k] = Ck * (-Du - L * Ic / I)
    return M, dM, J


def gradient_and_budget(model_id, params, x, y):
    """(dS/dtheta [Np], B [Np], dS/d(row quantity) [13]) in long double."""
    M, dM, J = row_derivatives(model_id, params, x)
    y = _ld(y)
    r = LD(1) / M - y / (M * M)
    W = LD(1) / M + 2 * y / (M * M)
    rows = dM @ r
    brow = np.abs(dM) @ W
    with np.errstate(invalid="ignore"):
        grad = np.array([np.sum([rows[q] * J[q, j] for q in range(NROW) if J[q, j] != 0] + [LD(0)]) for j in range(J.shape[1])], dtype=LD)
        B = LD(1e-12) * np.array([np.sum([brow[q] * np.abs(J[q, j]) for q in range(NROW) if J[q, j] != 0] + [LD(0)]) for j in range(J.shape[1])], dtype=LD)
    return grad, B, rows


def chain_rule(model_id, params, rows):
    """Row-space sums (dS/d(row quantity), 13 values) -> dS/dtheta with the Jacobian above: what the host does in long double."""
    J = row_derivatives(model_id, params, np.array([1.0, 2.0]))[2]
    rows = _ld(rows)
    with np.errstate(invalid="ignore"):
        g = np.array([np.sum([rows[q] * J[q, j] for q in range(NROW) if J[q, j] != 0] + [LD(0)]) for j in range(J.shape[1])], dtype=LD)
        mag = np.array([np.sum([np.abs(rows[q] * J[q, j]) for q in range(NROW) if J[q, j] != 0] + [LD(0)]) for j in range(J.shape[1])], dtype=LD)
    return g, mag

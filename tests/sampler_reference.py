"""50-digit restatement of the sampler's own algebra, for the parity tests of the host and the device engine.

What one iteration of the adaptive, parallel-tempered Metropolis / Langevin sampler computes besides the model, written from its
definition (MALA.cpp:296-319, :339-369, :397-461, :490-551; the Langevin step the reference leaves as stubs as DESIGN.md states it) with
`decimal` at 50 significant digits and plain Python integers.  It shares no line with csrc/ or oracle/.

    draws        Philox4x32-10 (Salmon et al. 2011), the (iteration lo, iteration hi, index, purpose << 16 | chain) / (seed lo, seed hi)
                 addressing, the 53-bit uniform in (0, 1), Box-Muller z = rho (cos, sin)(2 pi u1), rho = sqrt(-2 ln u0), with the sine and
                 cosine summed from their Taylor series after reduction to [-pi/4, pi/4]
    factor       A = fl(fl(Sigma_ij + eps2 delta_ij) sigma) formed in double, as both engines form it; its exact lower Cholesky factor,
                 or None when a pivot is <= 0
    drift        (1/2) sigma s (Sigma + eps2 I) g,  s = delta / |g| when delta > 0 and |g| > delta;  zero when |g| is not finite
    proposal     x + d + L z
    density      w = L^-1 b, lq = -|w|^2 / 2 for the forward move b = x' - x - d(x) and the reverse move b = x - x' - d(x')
    mh_test      r = min(1, exp(logPost' - logPost + lq_r - lq_f)) with the -inf / NaN rules; acceptance is u <= r
    adapt        Robbins-Monro with gain c0 / (1 + i): mu (clipped to norm A1), the deviation from the UPDATED mu, the covariance (clipped
                 to Frobenius norm A1), sigma clipped to [eps1, A1]
    swap         r_T and what either side holds afterwards (both rules for chain B's stored posterior), the carried gradient
                 (g - g_prior) T_src / T_m + g_prior

Inputs are doubles and are converted exactly (Decimal(float)).  Every result comes with its ERROR SCALE: the magnitude a rounding error
of the double computation is proportional to, computed from the same inputs.  A comparison is |got - ref| <= K 2^-52 scale.  The scales
need two digits, not fifty, and are computed in float64 with numpy (|L^-1| by forward substitution of the rounded factor).

    proposal     |x_i| + |d_i| + sum_k |L_ik| rho_k          (rho, not |z|: the error of rho cos is proportional to rho)
    w = L^-1 b   e = |L^-1| (|L| |w| + |x' - x| + (1/2) sigma s (|Sigma| + eps2 I) |g|)
    lq           sum_i |w_i| e_i
    ln r         |logPost'| + |logPost| + scale(lq_f) + scale(lq_r)
    mu'          |mu| + gamma |x - mu|
    cov'_ij      |c_ij| + gamma (|d_i d_j| + |c_ij|)
    sigma'       |sigma| + gamma |r - target|
    carried g    |g - g_p| T_src / T_m + |g_p|
"""
import math
from decimal import Context, Decimal, localcontext

import numpy as np

PREC = 50
WORK = 64                                   # digits of the series (their largest term is ~1: nothing is lost to cancellation)
PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899862803")
PURPOSE = {"proposal": 1, "accept": 2, "swap": 3, "noise": 4}
ZERO, ONE, HALF = Decimal(0), Decimal(1), Decimal("0.5")


def dec(x):
    return Decimal(float(x))


def _ctx():
    return localcontext(Context(prec=PREC))


# ---------------------------------------------------------------------------------------------------------------- draws

def philox4x32(ctr, key, rounds=10):
    """Philox4x32: counter (c0..c3), key (k0, k1) -> four 32-bit words."""
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def words(seed, purpose, chain, iteration, idx):
    """The block of (seed) x (purpose, chain) x (iteration, index)."""
    M = 0xFFFFFFFF
    return philox4x32((iteration & M, (iteration >> 32) & M, idx & M, ((purpose << 16) | (chain & 0xFFFF)) & M), (seed & M, (seed >> 32) & M))


def u01(hi, lo):
    """(b + 1/2) 2^-53 of the upper 53 bits b, rounded to the nearest double (ties to even); the one word that rounds to 1 gives the
    largest double below 1: never 0, never 1."""
    b = ((hi << 32) | lo) >> 11
    u = (2 * b + 1) / (1 << 54)             # integer true division is correctly rounded
    return u if u < 1.0 else 1.0 - 2.0 ** -53


def uniform2(seed, purpose, chain, iteration, idx):
    w = words(seed, purpose, chain, iteration, idx)
    return u01(w[0], w[1]), u01(w[2], w[3])


def _sincos_small(x):
    """sin, cos of |x| <= pi/4 + a little, Taylor series in the current context."""
    x2 = x * x
    s, c, ts, tc, k = x, ONE, x, ONE, 0
    eps = Decimal(10) ** -(WORK + 2)
    while True:
        k += 2
        tc = -tc * x2 / ((k - 1) * k)
        ts = -ts * x2 / (k * (k + 1))
        c += tc
        s += ts
        if abs(tc) < eps and abs(ts) < eps:
            return s, c


def sincos_2pi(u):
    """(sin, cos)(2 pi u) for a double u in [0, 1]: angle = n pi/2 + x with n = round(4 u) found exactly, the series sees |x| <= pi/4."""
    with localcontext() as c:
        c.prec = WORK
        n = int((dec(u) * 4 + HALF) // 1)
        x = (dec(u) * 4 - n) * PI / 2
        s, co = _sincos_small(x)
        q = n % 4
        s, co = ((s, co), (co, -s), (-s, -co), (-co, s))[q]
    with _ctx():
        return +s, +co


def normal2(seed, purpose, chain, iteration, idx):
    """(z0, z1, rho) of one Philox block: z = rho (cos, sin)(2 pi u1), rho = sqrt(-2 ln u0)."""
    u0, u1 = uniform2(seed, purpose, chain, iteration, idx)
    with _ctx():
        rho = (-2 * dec(u0).ln()).sqrt()
        s, c = sincos_2pi(u1)
        return rho * c, rho * s, rho


def normals(seed, chain, iteration, nvars):
    """z [nvars] and rho [nvars] of a chain's proposal at `iteration` (pair k/2 of purpose `proposal`: variables k, k+1)."""
    z, rho = [], []
    for k in range(0, nvars, 2):
        z0, z1, r = normal2(seed, PURPOSE["proposal"], chain, iteration, k // 2)
        z += [z0, z1]
        rho += [r, r]
    return z[:nvars], rho[:nvars]


def accept_uniform(seed, chain, iteration):
    return uniform2(seed, PURPOSE["accept"], chain, iteration, 0)[0]


def swap_draw(seed, nchains, iteration):
    """(first chain A of the pair (A, A+1), the uniform of the swap test)."""
    u, u2 = uniform2(seed, PURPOSE["swap"], 0, iteration, 0)
    return min(int(u2 * (nchains - 1)), nchains - 2), u


# ---------------------------------------------------------------------------------------------------------------- the factor

def matrix_to_factor(cov, eps2, sigma):
    """A = fl(fl(Sigma_ij + eps2 delta_ij) sigma) in double [n x n]."""
    A = np.array(cov, dtype=np.float64, copy=True)
    n = A.shape[0]
    A[np.arange(n), np.arange(n)] += np.float64(eps2)
    return A * np.float64(sigma)


def cholesky(A):
    """Exact (50-digit) lower Cholesky factor of the double matrix A (its lower triangle), rows as lists of Decimal; None when a pivot
    is <= 0: not positive definite."""
    n = len(A)
    with _ctx():
        L = []
        for i in range(n):
            ai = A[i]
            row = []
            for j in range(i):
                lj = L[j]
                s = dec(ai[j])
                for k in range(j):
                    s -= row[k] * lj[k]
                row.append(s / lj[j])
            d = dec(ai[i])
            for k in range(i):
                d -= row[k] * row[k]
            if not d > 0:
                return None
            row.append(d.sqrt())
            L.append(row)
    return L


def factor_float(L):
    """The factor rounded to double, full lower-triangular matrix."""
    n = len(L)
    F = np.zeros((n, n))
    for i, row in enumerate(L):
        F[i, :i + 1] = [float(v) for v in row]
    return F


def abs_inverse(Lf):
    """|L^-1| in float64 (a scale): row-by-row forward substitution on the identity."""
    n = Lf.shape[0]
    X = np.zeros((n, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        X[i] = (e - Lf[i, :i] @ X[:i]) / Lf[i, i]
    return np.abs(X)


# ---------------------------------------------------------------------------------------------------------------- drift, proposal

class Drift:
    """d [n] Decimal; spread [n] float = (1/2) sigma s (|Sigma| + eps2 I) |g| (the error scale of d's own sum); truncated: s < 1."""

    def __init__(self, d, spread, truncated, s):
        self.d, self.spread, self.truncated, self.s = d, spread, truncated, s


def drift(cov, sigma, eps2, delta, g):
    n = len(g)
    g = np.asarray(g, dtype=np.float64)
    if not np.all(np.isfinite(g)):
        return Drift([ZERO] * n, np.zeros(n), False, ONE)
    with _ctx():
        gd = [dec(v) for v in g]
        nrm = sum((v * v for v in gd), ZERO).sqrt()
        if nrm.is_infinite() or nrm.is_nan():
            return Drift([ZERO] * n, np.zeros(n), False, ONE)
        s, trunc = ONE, False
        if delta > 0 and nrm > dec(delta):
            s, trunc = dec(delta) / nrm, True
        f = HALF * dec(sigma) * s
        e2 = dec(eps2)
        d = []
        for i in range(n):
            ci = cov[i]
            acc = ZERO
            for j in range(n):
                if ci[j] != 0.0 and g[j] != 0.0:
                    acc += dec(ci[j]) * gd[j]
            d.append(f * (acc + e2 * gd[i]))
    spread = float(f) * (np.abs(np.asarray(cov, dtype=np.float64)) @ np.abs(g) + float(eps2) * np.abs(g))
    return Drift(d, spread, trunc, s)


def proposal(x, d, L, z, rho, Lf=None):
    """(x' [n] Decimal, scale [n] float): x + d + L z.  Lf: the factor rounded to double, when the caller has it."""
    n = len(x)
    with _ctx():
        xp = []
        for i in range(n):
            s = ZERO
            li = L[i]
            for k in range(i + 1):
                s += li[k] * z[k]
            xp.append(dec(x[i]) + d[i] + s)
    Lf = factor_float(L) if Lf is None else Lf
    scale = np.abs(np.asarray(x, dtype=np.float64)) + np.abs([float(v) for v in d]) + np.abs(Lf) @ np.array([float(r) for r in rho])
    return xp, scale


# ---------------------------------------------------------------------------------------------------------------- densities, test

def solve_lower(L, b):
    n = len(b)
    with _ctx():
        w = []
        for i in range(n):
            s = b[i]
            li = L[i]
            for k in range(i):
                s -= li[k] * w[k]
            w.append(s / li[i])
    return w


class Density:
    """lq = -|w|^2 / 2 (Decimal), w [n] Decimal, e [n] float (error scale of w), scale float (error scale of lq)."""

    def __init__(self, lq, w, e, scale):
        self.lq, self.w, self.e, self.scale = lq, w, e, scale


def density(L, x_from, x_to, dr, Lf=None, Linv_abs=None):
    """log q(x_to | x_from) up to the constant: w = L^-1 (x_to - x_from - d(x_from)); dr = drift at x_from (a Drift)."""
    n = len(x_from)
    with _ctx():
        b = [dec(x_to[i]) - dec(x_from[i]) - dr.d[i] for i in range(n)]
        w = solve_lower(L, b)
        lq = -HALF * sum((v * v for v in w), ZERO)
    Lf = factor_float(L) if Lf is None else Lf
    Linv_abs = abs_inverse(Lf) if Linv_abs is None else Linv_abs
    wf = np.array([float(v) for v in w])
    step = np.abs(np.asarray(x_to, dtype=np.float64) - np.asarray(x_from, dtype=np.float64))
    e = Linv_abs @ (np.abs(Lf) @ np.abs(wf) + step + dr.spread)
    return Density(lq, w, e, float(np.abs(wf) @ e))


class Test:
    """r (Decimal in [0, 1]); ln_r = the exponent (Decimal, None where a rule sets r = 0); scale of ln r; accepted for a comparator u."""

    def __init__(self, r, ln_r, scale):
        self.r, self.ln_r, self.scale = r, ln_r, scale

    def accepts(self, u):
        return dec(u) <= self.r


def mh_test(logL_new, logPr_new, logPost_new, logPost_cur, lq_fwd=None, lq_rev=None):
    """MALA.cpp:490-551 with the proposal densities: a NaN likelihood or a prior of -inf / NaN gives r = 0, a NaN ratio gives r = 0.
    logPost_new = the double the engine holds (logL + logPr); lq_*: Density or None (random walk: the densities cancel)."""
    scale = abs(logPost_new) + abs(logPost_cur) + (lq_fwd.scale + lq_rev.scale if lq_fwd is not None else 0.0)
    if math.isnan(logL_new) or math.isnan(logPr_new) or logPr_new == -math.inf or logPost_new == -math.inf:
        return Test(ZERO, None, scale)
    if math.isnan(logPost_new) or math.isnan(logPost_cur) or (math.isinf(logPost_new) and math.isinf(logPost_cur)):
        return Test(ZERO, None, scale)      # exp(NaN)
    with _ctx():
        if logPost_cur == -math.inf or logPost_new == math.inf:
            return Test(ONE, Decimal("Infinity"), scale)
        e = dec(logPost_new) - dec(logPost_cur)
        if lq_fwd is not None:
            e += lq_rev.lq - lq_fwd.lq
        r = ONE if e >= 0 else (e.exp() if e > -2500 else ZERO)
    return Test(r, e, scale)


# ---------------------------------------------------------------------------------------------------------------- Robbins-Monro

class Law:
    """mu [n], cov [n][n], sigma as Decimal; their error scales as float arrays; gamma (Decimal); dev = x - mu' (Decimal)."""


def adapt(mu, cov, sigma, x, r, iteration, c0, target, eps1, A1, mu_new_given=None):
    """MALA.cpp:296-319 at position x with move probability r.  mu_new_given: the doubles an engine holds as its updated mean; the
    deviation is then taken from them (the engine's deviation x - mu' inherits the rounding of mu', a relative error of
    2^-53 |mu'| / |x - mu'| that is no property of the covariance update: mu' is compared on its own)."""
    n = len(mu)
    out = Law()
    with _ctx():
        gam = dec(c0) / (1 + Decimal(int(iteration)))
        a1 = dec(A1)
        v = [dec(mu[k]) + gam * (dec(x[k]) - dec(mu[k])) for k in range(n)]
        nrm = sum((t * t for t in v), ZERO).sqrt()
        if not nrm <= a1:
            v = [t * a1 / nrm for t in v]
        out.mu = v
        base = v if mu_new_given is None else [dec(t) for t in mu_new_given]
        d = [dec(x[k]) - base[k] for k in range(n)]
        out.dev = d
        C = [[dec(cov[i][j]) + gam * (d[i] * d[j] - dec(cov[i][j])) for j in range(n)] for i in range(n)]
        nrm = sum((t * t for row in C for t in row), ZERO).sqrt()
        if not nrm <= a1:
            C = [[t * a1 / nrm for t in row] for row in C]
        out.cov = C
        s = dec(sigma) + gam * (dec(r) - dec(target))
        out.sigma = min(max(s, dec(eps1)), a1)
        out.gamma = gam
    g = float(gam)
    mu_f, x_f, cov_f = (np.asarray(a, dtype=np.float64) for a in (mu, x, cov))
    d_f = np.array([float(t) for t in d])
    out.mu_scale = np.abs(mu_f) + g * np.abs(x_f - mu_f)
    out.cov_scale = np.abs(cov_f) + g * (np.abs(np.outer(d_f, d_f)) + np.abs(cov_f))
    out.sigma_scale = abs(float(sigma)) + g * abs(float(r) - float(target))
    return out


# ---------------------------------------------------------------------------------------------------------------- swap

class Swap:
    """r_T (Decimal), ln_rT, swapped for the comparator; A / B = (logL, logPr, logPost) each side holds afterwards (Decimal)."""


def resolve_swap(statA, statB, TA, TB, u, swap_rule=0):
    """MALA.cpp:397-461 on the tempered log-likelihoods: r_T = min(1, exp(LA TA/TB + LB TB/TA - LA - LB)); on a swap A receives B's
    position re-tempered to T_A and vice versa.  swap_rule 1: B's stored posterior carries B's own old prior (MALA.cpp:444 as executed)."""
    out = Swap()
    with _ctx():
        LA, prA = dec(statA[0]), dec(statA[1])
        LB, prB = dec(statB[0]), dec(statB[1])
        ta, tb = dec(TA), dec(TB)
        LA_TB, LB_TA = LA * ta / tb, LB * tb / ta
        e = LA_TB + LB_TA - LA - LB
        out.ln_rT = e
        out.rT = ONE if e >= 0 else (e.exp() if e > -2500 else ZERO)
        out.scale = float(abs(LA_TB) + abs(LB_TA) + abs(LA) + abs(LB))
        out.swapped = dec(u) <= out.rT
        if out.swapped:
            out.A = (LB_TA, prB, LB_TA + prB)
            out.B = (LA_TB, prA, LA_TB + (prB if swap_rule == 1 else prA))
        else:
            out.A = tuple(dec(v) for v in statA)
            out.B = tuple(dec(v) for v in statB)
    return out


def carried_gradient(g, gp, T_src, T_m):
    """(gradient [n] Decimal, scale [n] float) of a position that moves from temperature T_src to T_m: the likelihood share re-tempered."""
    with _ctx():
        t = dec(T_src) / dec(T_m)
        out = [(dec(a) - dec(b)) * t + dec(b) for a, b in zip(g, gp)]
    g, gp = np.asarray(g, dtype=np.float64), np.asarray(gp, dtype=np.float64)
    return out, np.abs(g - gp) * float(T_src) / float(T_m) + np.abs(gp)


# ---------------------------------------------------------------------------------------------------------------- comparison

def ratio(got, ref, scale):
    """max over the elements of |got - ref| / (2^-52 scale); got: doubles, ref: Decimals, scale: floats (a zero scale with a zero
    difference counts as 0)."""
    got = np.asarray(got, dtype=np.float64).ravel()
    scale = np.asarray(scale, dtype=np.float64).ravel()
    ref = list(ref) if not isinstance(ref, Decimal) else [ref]
    worst = 0.0
    with _ctx():
        for a, b, s in zip(got, ref, scale):
            diff = abs(dec(a) - b)
            if diff == 0:
                continue
            if s == 0.0 or not math.isfinite(a):
                return math.inf
            worst = max(worst, float(diff / (dec(s) * Decimal(2) ** -52)))
    return worst

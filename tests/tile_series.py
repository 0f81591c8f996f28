"""The FAST tile's two truncated series restated in Python doubles, and the bounds their truncation obeys.

Restated statement for statement from csrc/bg_series.h (harvey_term_series) and csrc/loglike_tile.h (far_seed, far_coefs<EARLY_STOP>,
far_coefs_asym, asym_poly, horner); the device's reciprocal-with-Newton-steps is a plain division here and its fma an unfused a*b+c:
both differ by rounding only, which is not what the bounds below are about.  test_tile_bounds.py checks every bound against the
50-digit definition (tile_reference.py); test_gpu_tile_reference.py imports TAU_FAR, TAU_ASYM and HARVEY_BUDGET and no other tolerance.

Far field.  One component on a tile, with s = (x - x_c)/h in [-1, 1], beta = 2h/gamma, A = 2(nu - x_c)/gamma:
    f(s) = hv / (1 + (beta s - A)^2) = -hv Im(u / (1 - q s)) = sum_k c_k s^k,   u = 1/(A + i), q = beta u, |q| = rho,
    c_k = -hv Im(u q^k).
Deep in the wing (A >> 1) u and q are almost real and f(s) ~ hv / (A^2 (1 - rho s)^2), a DOUBLE pole: c_k ~ hv (k + 1) rho^k / A^2.
Its tail after n coefficients, relative to f itself, is largest at the end of the tile nearest the pole:
    sum_{k >= n} (k + 1) rho^k (1 - rho)^2 = rho^n (n + 1 - n rho)   at s = +1 (pole side),
    |sum_{k >= n} (k + 1) (-rho)^k| (1 + rho)^2 = rho^n (n + 1 + n rho)   at s = -1 (far side: the term is smallest there).
So   tau(rho, n) = rho^n (n + 1 + n rho)   bounds the truncation relative to the far term at every bin of the tile, for every A:
for smaller A the pole pair 1/q, 1/conj(q) separates and the coefficients -hv Im(u q^k) only lose against the double pole's.
(The simple-pole figure rho^n / (1 - rho) that the headers quoted until now omits the factor ~ n + 1.)
"""
import math

NC = 16                      # coefficients of the tile polynomial
NH = 8                       # coefficients of a Harvey term's series
RHO_MAX2 = 1.0 / 36.0        # the far gate: rho <= 1/6
RHO_MAX2_ASYM = 1.0 / 64.0   # rows with asymmetry: rho <= 1/8
# far_coefs<EARLY_STOP>: (threshold on q2 = rho^2, number of coefficients kept when q2 <= threshold)
EARLY_STOP = ((1.39e-2, 14), (6.8e-3, 12), (2.5e-3, 10), (5.6e-4, 8), (4.6e-5, 6))


def tau(rho, n):
    """Truncation of the far series after n coefficients, relative to the far term, at any bin of the tile (derivation above)."""
    return rho ** n * (n + 1 + n * rho)


TAU_FAR = tau(1.0 / 6.0, NC)   # 6.96e-12: what FAST may add per bin, times F(x) = sum of the |far components| there
assert 6.9e-12 < TAU_FAR < 7.0e-12

# Rows with asymmetry.  The component times the quadratic Q(s) = A0 + A1 s + A2 s^2 = (p0 + p1 s)^2 + c2^2, cut after NC coefficients.  What
# is cut is Q(s) tail_NC(s) plus the terms the quadratic feeds back across the cut, A1 c_{NC-1} s^NC + A2 (c_{NC-1} s^(NC+1) + c_{NC-2} s^NC);
# relative to Q f the first part is tau(1/8, NC) = 6.8e-14.  The rest has no closed form relative to the far term: Q can come close to zero on
# the tile (asym (x / nu_c - 1) = -1), and where it is small the sum A0 c_k + A1 c_{k-1} + A2 c_{k-2} cancels, so the double rounding of the
# coefficients, not the truncation, sets the error relative to the term.  Measured instead: worst |restatement - definition| / |far term|
# over asym in {-100, -30, 5, 30, 100}, A in {0, .5, 1, 3, 10, 100, 1e4} on either side of the tile, rho^2 = 1/64, gamma = 2, x_c = 2000,
# nu_c = nu, 41 values of s (test_tile_bounds.py::test_asymmetric_far_series): 6.90e-13 (at asym = 30, A = 100, where
# asym (x / nu_c - 1) passes -1.5 on the tile; 2.9e-13 at asym = -30, A = 100; 2.4e-13 at asym = -100, A = 10; 3.6e-15, the figure
# the header quoted, at A = 0).  TAU_ASYM = 4 x the worst.
TAU_ASYM_MEASURED = 6.90e-13
TAU_ASYM = 4.0 * TAU_ASYM_MEASURED

# Background series.  A Harvey term T(x) = H / (1 + u), u = (a x)^p, deep in its decline (a x_c >> 1) is H (a x_c)^-p (1 + eps s)^-p, whose
# k-th coefficient is C(p + k - 1, k) eps^k in magnitude (all of one sign at s = -1, where the term itself is (1 - eps)^-p >= 1 of its
# value at the centre): the tail after NH = 8 coefficients is at most C(p + 7, 8) eps^8 / (1 - (p + 8)/9 eps) of the term at the same
# bin.  For a x_c <~ 1 the term flattens and the tail shrinks.  The gate admits a tile when C(p_max + 7, 8) eps^8 <= SERIES_BUDGET = 2e-13
# and eps <= EPS_MAX; 1 / (1 - (p + 8)/9 eps) <= 1.12 wherever that holds for a p <= 40 ((p + 8)/9 eps is largest at the gate's
# largest eps, 0.02 at p <= 1.8: 0.022; p = 8: 0.015; p = 40: 0.03), and the double rounding of eight coefficients and their Horner
# sum adds at most 64 x 2^-53.  Every term of an evaluation keeps HARVEY_BUDGET relative to ITSELF, so the sum of the terms' errors is
# <= HARVEY_BUDGET x M = 0.23e-12 M however many terms there are: the rest of the FAST statement's 1e-12 M stays for rounding.
SERIES_BUDGET = 2e-13
HARVEY_BUDGET = 1.12 * SERIES_BUDGET + 64 * 2.0 ** -53
EPS_MAX = 0.02


def binom_rising(p, n=NH):
    c = 1.0
    for k in range(n):
        c *= (p + k) / (k + 1.0)
    return c


def eps_at_gate(p):
    """The largest eps = h / x_c the background gate admits for exponent p."""
    return min(EPS_MAX, (SERIES_BUDGET / binom_rising(p)) ** 0.125)


# ---------------------------------------------------------------- csrc/bg_series.h ----------------------------------------------------------------
def harvey_term_series(Hh, tau_, pw, xc, h):
    f = [0.0] * NH
    if tau_ != 0.0:
        eps = h / xc
        u = [0.0] * NH
        u[0] = math.exp(pw * math.log(1e-3 * tau_ * xc))
        for k in range(NH - 1):
            u[k + 1] = u[k] * eps * (pw - float(k)) * (1.0 / float(k + 1))
        iv0 = 1.0 / (1.0 + u[0])
        f[0] = Hh * iv0
        for k in range(1, NH):
            acc2 = 0.0
            for jj in range(1, k + 1):
                acc2 = u[jj] * f[k - jj] + acc2
            f[k] = -acc2 * iv0
    return f


# ---------------------------------------------------------------- csrc/loglike_tile.h ----------------------------------------------------------------
def far_seed(hv, A, beta):
    inv = 1.0 / (A * A + 1.0)
    return hv * inv, 2.0 * beta * A * inv, beta * beta * inv   # c0, two_req, q2


def n_terms(q2):
    return 16 if q2 > 1.39e-2 else 14 if q2 > 6.8e-3 else 12 if q2 > 2.5e-3 else 10 if q2 > 5.6e-4 else 8 if q2 > 4.6e-5 else 6


def far_coefs(seed, early_stop, wave_nt=None):
    """The NC coefficients of one component.  early_stop: the loop ends where the device's ends when every lane of the wave has
    n_terms <= wave_nt (default: this component's own) -- the break is tested at even k >= 6."""
    c0, two_req, q2 = seed
    fc = [0.0] * NC
    cm, cc = c0, c0 * two_req
    fc[0], fc[1] = cm, cc
    nt = NC
    if early_stop:
        nt = n_terms(q2) if wave_nt is None else wave_nt
    for k in range(2, NC):
        if early_stop and (k & 1) == 0 and k >= 6 and not (k < nt):
            break
        cn = two_req * cc + (-q2 * cm)
        fc[k] = cn
        cm, cc = cc, cn
    return fc


def asym_poly(fcx, asym, c2sq, xc, h):
    p0, p1 = fcx * xc + (1.0 - asym), fcx * h
    return p0 * p0 + c2sq, 2.0 * p0 * p1, p1 * p1


def far_coefs_asym(seed, P):
    c0, two_req, q2 = seed
    A0, A1, A2 = P
    fc = [0.0] * NC
    c2, c1, c0k = 0.0, 0.0, c0
    nxt = c0 * two_req
    for k in range(NC):
        fc[k] = A0 * c0k + (A1 * c1 + A2 * c2)
        cn = nxt if k == 0 else two_req * c0k + (-q2 * c1)
        c2, c1, c0k = c1, c0k, cn
    return fc


def horner(coef, s):
    P = coef[-1]
    for q in range(len(coef) - 2, -1, -1):
        P = P * s + coef[q]
    return P

"""The likelihood tile's definition at 50 digits, for the parity tests of the FAST / STRICT model rows and log-likelihoods.

Apart from the CPU oracle (C double) and from test_gpu_parity._numpy_table_model (numpy double): it shares no line with either, nor with
csrc/loglike_tile.h or csrc/bg_series.h.  It takes what the table-level entry tamcmc_hip_loglike_batch takes -- the multiplet rows
(MULT_DTYPE), a noise vector with its nh / nn, x, y, T and p -- and every double among them as the exact rational it is.

    model_row_exact / loglike_exact    `decimal` at 50 significant digits (standard library only): the definition
    model_row_ld / loglike_ld          the vectorised numpy.longdouble twin (64-bit significand): what the tests run over every bin
                                       (test_tile_reference.py pins it to the definition within 2^-60)

The model row (build_lorentzian.cpp:131-246 per component on its window, noise_models.cpp:15-39):
    M(x) = sum_rows [i0 <= i < i1] sum_{m < 2l+1} hv_m / (1 + 4 (x - nu_m)^2 / gamma^2) * asy(x)
           + sum_{k < nh, tau_k != 0} H_k / (1 + exp(p_k ln(1e-3 tau_k x))) + noise[nn - 1]
    asy(x) = (1 + asym (x / fc - 1))^2 + (gamma asym / (2 fc))^2  when asym != 0, else 1
logL = -(long)p (sum_i y_i / M_i + sum_i ln M_i) / T   (likelihoods.cpp:17-28; model_def.cpp:399-401).

Beside the definition, the module restates in plain Python the GEOMETRY of the FAST far field -- which (row, tile) pairs the tile
kernel may sum as a polynomial -- so that a test can grant the far-field truncation tau F(x) where, and only where, it applies:
    tile centre and half-width on the regular grid: h = tile_bins step / 2, x_c = x0 + (t0 + tile_bins / 2 - 1/2) step
    a row is FAR on a tile when its window covers the tile's bins and beta^2 <= r2 (A_m^2 + 1) for every component m < 2l+1,
    beta = 2 h / gamma, A_m = 2 (nu_m - x_c) / gamma, r2 = 1/36 (1/64 for a row with asymmetry)
and the gate of the background series (series_gate).
"""
from decimal import Decimal, localcontext

import numpy as np

PREC = 50
LD = np.longdouble
MILLI = 1e-3   # the double the code multiplies tau by (an input like any other: exact)

R2_FAR = 1.0 / 36.0
R2_FAR_ASYM = 1.0 / 64.0
EPS_MAX = 0.02
SERIES_BUDGET = 2e-13


def _D(v):
    return Decimal(float(v))


# ---------------------------------------------------------------- the definition, 50 digits ----------------------------------------------------------------
def component_exact(x, nu, hv, gamma, asym=0.0, fc=1.0):
    """One Lorentzian component (with its asymmetry factor) at one bin: Decimal."""
    with localcontext() as ctx:
        ctx.prec = PREC
        x, nu, hv, g = _D(x), _D(nu), _D(hv), _D(gamma)
        v = hv / (1 + 4 * (x - nu) ** 2 / (g * g))
        if float(asym) != 0.0:
            a, f = _D(asym), _D(fc)
            v = v * ((1 + a * (x / f - 1)) ** 2 + (g * a / (2 * f)) ** 2)
        return v


def harvey_exact(x, H, tau, pw):
    """One Harvey term at one bin: Decimal (0 for tau == 0, noise_models.cpp:29)."""
    with localcontext() as ctx:
        ctx.prec = PREC
        if float(tau) == 0.0:
            return Decimal(0)
        if float(x) == 0.0:   # (a 0)^p = 0 for the positive exponents of a Harvey term
            return _D(H)
        u = (_D(pw) * (_D(MILLI) * _D(tau) * _D(x)).ln()).exp()
        return _D(H) / (1 + u)


def model_row_exact(mults, noise, nh, nn, x, bins=None):
    """{bin: M} (Decimal) at `bins` (default: every bin)."""
    bins = range(len(x)) if bins is None else bins
    out = {}
    with localcontext() as ctx:
        ctx.prec = PREC
        for i in bins:
            i = int(i)
            m = Decimal(0)
            for r in mults:
                if int(r["i0"]) <= i < int(r["i1"]):
                    for k in range(2 * int(r["l"]) + 1):
                        m += component_exact(x[i], r["nu"][k], r["hv"][k], r["gamma"], r["asym"], r["fc"])
            for k in range(int(nh)):
                m += harvey_exact(x[i], noise[3 * k], noise[3 * k + 1], noise[3 * k + 2])
            out[i] = m + _D(noise[int(nn) - 1])
    return out


def loglike_exact(model, y, T=1.0, p=1.0):
    """logL (Decimal) of a model row given as Decimals (or anything Decimal() takes exactly), a restatement of chi22p."""
    with localcontext() as ctx:
        ctx.prec = PREC
        s1 = s2 = Decimal(0)
        for mi, yi in zip(model, y):
            mi = mi if isinstance(mi, Decimal) else _D(mi)
            s1 += _D(yi) / mi
            s2 += mi.ln()
        return -int(p) * (s1 + s2) / _D(T)


# ---------------------------------------------------------------- the longdouble twin ----------------------------------------------------------------
def _row_components_ld(r, xs):
    """[2l+1 x len(xs)] longdouble: the row's components (asymmetry factor included) at xs."""
    g = LD(r["gamma"])
    g2 = g * g
    out = np.empty((2 * int(r["l"]) + 1, xs.size), dtype=LD)
    for k in range(out.shape[0]):
        d = xs - LD(r["nu"][k])
        out[k] = LD(r["hv"][k]) / (LD(1) + LD(4) * (d * d) / g2)
    if float(r["asym"]) != 0.0:
        a, f = LD(r["asym"]), LD(r["fc"])
        # x / fc - 1 as (x - fc) / fc: the same number, without the cancellation against a rounded quotient
        t = LD(1) + a * ((xs - f) / f)
        c2 = g * a / (LD(2) * f)
        out *= t * t + c2 * c2
    return out


def model_row_ld(mults, noise, nh, nn, x):
    """The model row at every bin, numpy.longdouble."""
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    m = np.zeros(xl.size, dtype=LD)
    for r in mults:
        sl = slice(int(r["i0"]), int(r["i1"]))
        m[sl] += _row_components_ld(r, xl[sl]).sum(axis=0)
    for k in range(int(nh)):
        if float(noise[3 * k + 1]) != 0.0:
            ax = LD(MILLI) * LD(noise[3 * k + 1]) * xl
            m += LD(noise[3 * k]) / (LD(1) + np.power(ax, LD(noise[3 * k + 2])))
    return m + LD(noise[int(nn) - 1])


def loglike_ld(model, y, T=1.0, p=1.0):
    """logL (numpy.longdouble) of a model row (any float type; taken exactly), pairwise-summed in longdouble."""
    m = np.asarray(model).astype(LD)
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    return -LD(int(p)) * ((yl / m).sum() + np.log(m).sum()) / LD(T)


# ---------------------------------------------------------------- geometry of the FAST far field ----------------------------------------------------------------
def tile_geometry(tile, tile_bins, x0, step):
    """(x_c, h) of tile `tile` on x[i] = x0 + i step."""
    h = 0.5 * tile_bins * step
    return x0 + (tile * tile_bins + 0.5 * tile_bins - 0.5) * step, h


def row_is_far(r, t0, t1, xc, h):
    """The geometric far rule of one row on one tile [t0, t1)."""
    if not (int(r["i0"]) <= t0 and int(r["i1"]) >= t1):
        return False
    g = float(r["gamma"])
    beta2 = (2.0 * h / g) ** 2
    r2 = R2_FAR_ASYM if float(r["asym"]) != 0.0 else R2_FAR
    for k in range(2 * int(r["l"]) + 1):
        A = 2.0 * (float(r["nu"][k]) - xc) / g
        if not beta2 <= r2 * (A * A + 1.0):   # (also near for NaN)
            return False
    return True


def far_map(mults, nx, tile_bins, x0, step):
    """[(row index, tile)] of the far (row, tile) pairs."""
    out = []
    ntiles = (nx + tile_bins - 1) // tile_bins
    for t in range(ntiles):
        t0, t1 = t * tile_bins, min((t + 1) * tile_bins, nx)
        xc, h = tile_geometry(t, tile_bins, x0, step)
        for j, r in enumerate(mults):
            if int(r["i0"]) < t1 and int(r["i1"]) > t0 and row_is_far(r, t0, t1, xc, h):
                out.append((j, t))
    return out


def far_abs_sum(mults, x, tile_bins, x0=None, step=None):
    """(F, F_asym) per bin, longdouble: the sums of |exact far component| there, of the rows without / with asymmetry."""
    x = np.asarray(x, dtype=np.float64)
    x0 = float(x[0]) if x0 is None else x0
    step = float(x[1] - x[0]) if step is None else step
    xl = x.astype(LD)
    F = np.zeros(x.size, dtype=LD)
    Fa = np.zeros(x.size, dtype=LD)
    for j, t in far_map(mults, x.size, tile_bins, x0, step):
        sl = slice(t * tile_bins, min((t + 1) * tile_bins, x.size))
        v = np.abs(_row_components_ld(mults[j], xl[sl])).sum(axis=0)
        if float(mults[j]["asym"]) != 0.0:
            Fa[sl] += v
        else:
            F[sl] += v
    return F, Fa


def binom_rising(p, n=8):
    """C(p + n - 1, n) = p (p + 1) .. (p + n - 1) / n!: |n-th binomial coefficient| of (1 + z)^-p."""
    c = 1.0
    for k in range(n):
        c *= (p + k) / (k + 1.0)
    return c


def series_gate(noise, nh, xc, h):
    """The background series may stand for the evaluation's Harvey terms on this tile: x_c > 0, eps = h / x_c <= EPS_MAX and
    C(p_max + 7, 8) eps^8 <= SERIES_BUDGET, p_max the largest exponent among the terms with tau != 0 (0 when there is none)."""
    pmax = 0.0
    for k in range(int(nh)):
        if float(noise[3 * k + 1]) != 0.0:
            pmax = max(pmax, abs(float(noise[3 * k + 2])))
    if not (xc > 0.0 and abs(h) <= EPS_MAX * abs(xc)):
        return False
    eps = abs(h / xc)
    return binom_rising(pmax) * eps ** 8 <= SERIES_BUDGET

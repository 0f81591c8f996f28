"""numpy restatement of the height-per-m models (test helper): parameter vector -> multiplet rows, following the reference line by line
   model_MS_Global_a1etaa3_HarveyLike_Classic_v2  tamcmc/sources/models.cpp:2128-2330  (id 12)
   model_MS_Global_a1etaa3_HarveyLike_Classic_v3  tamcmc/sources/models.cpp:2338-2553  (id 13)
   model_MS_local_Hnlm                            tamcmc/sources/models.cpp:3198-3336  (id 14)
with their offset quirks (ids 13, 14: the position of a degree's heights is counted as the model functions count it, not as the loaders
lay the block out).  Independent of the library's builder: its own polynomials, interpolation, eta0 and window; long double where the
reference's expression is long double.  The rows are evaluated by strict_numpy.eval_table.  Also the long-double restatement of the prior
that goes with id 12 (priors_MS_Global with impose_normHnlm = 1, priors_calc.cpp:223-243)."""
import numpy as np

LD = np.longdouble
PI_LD = LD("3.141592653589793238462643383279502884")
MULT_DTYPE = np.dtype([("l", "<i4"), ("i0", "<i4"), ("i1", "<i4"), ("flags", "<i4"), ("fc", "<f8"), ("gamma", "<f8"),
                       ("asym", "<f8"), ("nu", "<f8", (7,)), ("hv", "<f8", (7,))])


def qlm(l, m):  # build_lorentzian.cpp:583-592
    return float(LD((l * (l + 1) - 3.0 * m * m) / ((2 * l - 1) * (2 * l + 3))) * (LD(2.0) / LD(3.0)))


def p3lm(l, m):  # acoefs.cpp, s = 3
    return (5.0 * m ** 3 - (3 * l * (l + 1) - 1) * m) / ((l - 1) * (2 * l - 1)) if l > 1 else 0.0


def lin_interpol(x, y, xi):  # interpol.cpp:13-43
    n = len(x)
    if x[0] <= xi <= x[-1]:
        i = 0
        while i < n - 2 and (xi < x[i] or xi > x[i + 1]):
            i += 1
    elif xi < x[0]:
        i = 0
    else:
        i = n - 2
    a = (y[i + 1] - y[i]) / (x[i + 1] - x[i])
    return a * xi + (y[i] - a * x[i])


def eta0_fct(fl0):  # models.cpp:6065-6084 with linfit.cpp:17-35
    n = len(fl0)
    t = np.arange(n, dtype=np.float64)
    sx, sy = 0.0, 0.0
    for v in t:
        sx += v
    for v in fl0:
        sy += v
    mx = sx / n
    sty = stt = 0.0
    for i in range(n):
        sty += (t[i] - mx) * fl0[i]
    for i in range(n):
        stt += (t[i] - mx) * (t[i] - mx)
    dnu = sty / stt
    G, dnu_sun, r_sun, m_sun = 6.667e-8, 135.1, 6.96342e5, 1.98855e30
    rho_sun = m_sun * 1e3 / (4 * 3.14159265358979323846 * (r_sun * 1e5) ** 3 / 3)
    rho = (dnu / dnu_sun) ** 2 * rho_sun
    return 3.0 * 3.14159265358979323846 / (rho * G)


def window(x, l, fc, gamma, f_s, c, step):  # build_lorentzian.cpp:595-676
    if not (np.isfinite(gamma) and np.isfinite(f_s)):
        raise ValueError("NaN window")
    h = None  # the four overlapping regimes, later ones overriding earlier ones
    if gamma >= 1 and f_s >= 1:
        h = c * (l * f_s + gamma) if l != 0 else c * gamma * 2.2
    if gamma <= 1 and f_s >= 1:
        h = c * (l * f_s + 1) if l != 0 else c * 2.2
    if gamma >= 1 and f_s <= 1:
        h = c * (l + gamma) if l != 0 else c * 2.2 * gamma
    if gamma <= 1 and f_s <= 1:
        h = c * (l + 1) if l != 0 else c * 2.2
    lo, hi = fc - h, fc + h
    if hi - step < x[0]:
        hi = x[0] + c
    if lo + step >= x[-1]:
        lo = x[-1] - c
    i0 = max(int(np.floor((lo - x[0]) / step)), 0)
    i1 = min(int(np.ceil((hi - x[0]) / step)), x.size)
    return i0, i1


def layout(pl):
    nmax, lmax, nfl = int(pl[0]), int(pl[1]), [int(v) for v in pl[2:6]]
    o_f0 = nmax + lmax
    o_split = o_f0 + sum(nfl)
    o_width = o_split + int(pl[6])
    o_noise = o_width + int(pl[7])
    o_inc = o_noise + int(pl[8])
    return nmax, lmax, nfl, o_f0, o_split, o_width, o_noise, o_inc, o_inc + int(pl[9])


def _row(x, l, f, W, a1, eta0, a3, asym, hv, c, step):
    r = np.zeros((), dtype=MULT_DTYPE)
    r["l"], r["fc"], r["gamma"], r["asym"] = l, f, W, asym
    r["i0"], r["i1"] = window(x, l, f, W, a1, c, step)
    for k in range(2 * l + 1):
        m = k - l
        if l == 0:
            r["nu"][k] = f
        else:
            t = f * (1.0 + eta0 * (a1 * 1e-6) ** 2 * qlm(l, m)) + m * a1
            r["nu"][k] = float(LD(t) + LD(p3lm(l, m)) * LD(a3))
        r["hv"][k] = hv[k]
    return r


def _component_heights(p, base, l, W, do_amp):
    """Hl = params[base + |m|] (/ (pi W): an Eigen vector over a scalar -- the long double product rounded to double, a double division)."""
    v = np.array([p[base + abs(k - l)] for k in range(2 * l + 1)])
    if do_amp:
        v = v / float(PI_LD * LD(W))
    return np.abs(v)


def rows(model_id, p, pl, x):
    """(rows, |noise|, nharvey) of ids 12, 13 (n-major) and 14 (l-major)."""
    p = np.asarray(p, dtype=np.float64)
    nmax, lmax, nfl, o_f0, o_split, o_width, o_noise, o_inc, o_cfg = layout(pl)
    c, do_amp, step = p[o_cfg], p[o_cfg + 1] != 0, x[1] - x[0]
    a1, a3, asym = abs(p[o_split]), p[o_split + 2], p[o_split + 5]
    out = []

    def h0(v, W):
        return float(abs(LD(v) / (PI_LD * LD(W)))) if do_amp else abs(v)

    if model_id in (12, 13):
        fl0, wl0 = p[o_f0:o_f0 + nfl[0]], p[o_width:o_width + nmax]
        eta0 = eta0_fct(fl0)
        V = {1: abs(p[o_inc + np.array([1, 0, 1])]), 2: abs(p[o_inc + np.array([4, 3, 2, 3, 4])]),
             3: abs(p[o_inc + np.array([8, 7, 6, 5, 6, 7, 8])])} if model_id == 12 else None
        for n in range(nmax):
            W = abs(wl0[n])
            out.append(_row(x, 0, fl0[n], W, a1, eta0, a3, asym, [h0(p[n], W)], c, step))
            for l in range(1, min(lmax, 3) + 1):
                f = p[o_f0 + sum(nfl[:l]) + n]
                W = abs(lin_interpol(fl0, wl0, f))
                if model_id == 12:
                    vis = abs(p[nmax + l - 1])
                    H = float(abs(LD(p[n]) / (PI_LD * LD(W))) * LD(vis)) if do_amp else abs(p[n] * vis)
                    hv = H * V[l]
                else:
                    hv = _component_heights(p, o_inc + (l + 1) * n, l, W, do_amp)  # pos0 = 2n, 3n, 4n from the START of the block
                out.append(_row(x, l, f, W, a1, eta0, a3, asym, hv, c, step))
        nharvey = (int(pl[8]) - 1) // 3
    elif model_id == 14:
        eta0 = p[o_split + 1]
        for l in range(4):
            off = sum(nfl[:l])
            for n in range(nfl[l]):
                f, W = p[o_f0 + off + n], abs(p[o_width + off + n])
                hv = [h0(p[n], W)] if l == 0 else _component_heights(p, off + (l + 1) * n, l, W, do_amp)
                out.append(_row(x, l, f, W, a1, eta0, a3, asym, hv, c, step))
        nharvey = 0
    else:
        raise ValueError(model_id)
    return np.array(out, dtype=MULT_DTYPE), np.abs(p[o_noise:o_inc]), nharvey


# ---- priors_MS_Global, default (Classic) branch, impose_normHnlm = 1, smoothness and d02 terms included; Uniform / Gaussian / Jeffreys
#      generic priors (what the synthetic stars use) ----
def _generic(kind, a, b, v):
    a, b, v = LD(a), LD(b), LD(v)
    if kind == 0:
        return LD(0)
    if kind == 1:
        return -np.log(abs(b - a)) if a <= v <= b else -LD(np.inf)
    if kind == 2:
        return -np.log(np.sqrt(2 * PI_LD) * b) - LD(0.5) * ((v - a) / b) ** 2
    if kind == 4:
        return np.log((1 / (v + a)) / np.log((b + a) / a)) if (0 < v < b) else -LD(np.inf)
    raise ValueError(kind)


def _gaussian_uniform(bmin, bmax, sigma, v):
    bmin, bmax, sigma, v = LD(bmin), LD(bmax), LD(sigma), LD(v)
    lp = -LD(np.inf) if v > bmax else (LD(0) if v >= bmin else -LD(0.5) * ((v - bmin) / sigma) ** 2)
    return lp - np.log(abs(bmax - bmin) + LD(0.5) * np.sqrt(2 * PI_LD) * sigma)


def log_prior_v2(star, p):
    p = np.asarray(p, dtype=np.float64)
    pl, ex = star.plength, star.extra_priors
    nmax, lmax, nfl, o_f0, o_split, o_width, o_noise, o_inc, _ = layout(pl)
    if (p[nmax:nmax + lmax + 1] < 0).any():  # (one past the visibilities, as the reference's loop bound)
        return -np.inf
    f = LD(0)
    assert int(ex[8]) == 1 and not 0 <= int(ex[9]) <= 9
    q = p[o_inc:o_inc + 9]
    for s in (q[0] + 2 * q[1], q[2] + 2 * q[3] + 2 * q[4], q[5] + 2 * q[6] + 2 * q[7] + 2 * q[8]):
        f = f + _generic(1, 0.0, 1.0 + 1e-10, s)
    sw = star.priors_switch
    for k in (3, 6):
        if sw[o_noise + k] != 0 and (p[o_noise + k:o_noise + k + 3] < 0).any():
            return -np.inf
    if sw[o_split + 9] != 0 and p[o_noise + 9] < 0:
        return -np.inf
    pena = LD(0)
    for i in range(p.size):
        pena = pena + _generic(int(sw[i]), star.priors[0, i], star.priors[1, i], p[i])
    f = f + pena
    fl0 = p[o_f0:o_f0 + nfl[0]]
    t = np.arange(nfl[0], dtype=np.float64)
    dnu = np.sum((t - t.mean()) * fl0) / np.sum((t - t.mean()) ** 2)
    if nfl[0] == nfl[2]:
        for i in range(nfl[0]):
            f = f + _gaussian_uniform(0, dnu / 3.0, 0.015 * dnu, p[o_f0 + i] - p[o_f0 + nfl[0] + nfl[1] + i])
    if int(ex[0]) == 1:
        i0 = 0
        for el in range(min(lmax + 1, 4)):
            y = p[o_f0 + i0:o_f0 + i0 + nfl[el]]
            n = y.size
            for i in range(n):
                d = 0.0 if n < 3 else (y[2] - 2 * y[1] + y[0] if i == 0 else
                                       (y[n - 1] - 2 * y[n - 2] + y[n - 3] if i == n - 1 else y[i + 1] - 2 * y[i] + y[i - 1]))
                f = f + _generic(2, 0.0, ex[1], d)
            i0 += nfl[el]
    return float(f)

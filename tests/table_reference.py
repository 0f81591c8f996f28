"""50-digit restatement of parameter vector -> multiplet table, for the parity tests of the host builder and the three device builders.

What the model functions of the reference project compute before their per-bin loops, written from their definition with `decimal` at 50
significant digits, exact rationals and plain Python integers.  It shares no line with csrc/, oracle/ or hnlm_numpy.py.

    model_MS_Global_aj_HarveyLike                       models.cpp:1195-1408   id 23
    model_MS_Global_a1etaa3_HarveyLike_Classic          models.cpp:1943-2121   id 3
    model_MS_local_basic                                models.cpp:3012-3195   id 11
    model_MS_Global_a1etaa3_HarveyLike_Classic_v2, _v3  models.cpp:2128-2330, :2338-2553   ids 12, 13
    model_MS_local_Hnlm                                 models.cpp:3198-3336   id 14
    Pslm, Qlm        acoefs.cpp:51-110, build_lorentzian.cpp:583-592     exact rationals (fractions.Fraction)
    visibilities     function_rot.cpp:15-101 defines them as squared centre-column elements of the rotation matrix.  Here they are the
                     closed forms in the inclination i (c = cos i, s = sin i), not a Wigner sum:
                         l = 1   c^2 ;  s^2 / 2
                         l = 2   (3 c^2 - 1)^2 / 4 ;  3 c^2 s^2 / 2 ;  3 s^4 / 8
                         l = 3   c^2 (5 c^2 - 3)^2 / 4 ;  3 s^2 (5 c^2 - 1)^2 / 16 ;  15 c^2 s^4 / 8 ;  5 s^6 / 16
                     with sine and cosine from sampler_reference's Taylor series, pi to 50 digits, and (id 11) an arctangent summed here
    interpolation    interpol.cpp:13-43: the segment [x_k, x_k+1] that holds xi (the first one, scanning upwards; segment 0 below the
                     grid, the last one above it), a = (y_k+1 - y_k) / (x_k+1 - x_k), b = y_k - a x_k, value a xi + b
    eta0             linfit.cpp:17-35 against the index, models.cpp:6065-6084: 3 pi / (rho G), rho = (Dnu / 135.1)^2 rho_sun
    window           build_lorentzian.cpp:595-676: the four overlapping regimes (a later one overrides an earlier one), the two clip
                     rules, i0 = floor((lo - x_first) / step), i1 = ceil((hi - x_first) / step) of the EXACT quotients, clamped to [0, Nx]

Inputs are doubles and are converted exactly.  Constants the sources write as decimal literals (1e-3, 1e-6, 2.2, the solar values) are
those decimal numbers.  Every magnitude comes with its ERROR SCALE, the quantity a rounding error of a double evaluation is proportional
to; a comparison is |got - ref| <= K 2^-52 scale:

    nu_k       |f_c| + sum_j |a_j P_j| + |eta term|            (ids 3, 11..14: |f_c| + |f_c eta term| + |m a_1| + |P_3 a_3|)
    hv_k       H_scale x (norm x sum of the magnitudes of the half-angle terms of d^l_m0)^2 -- the terms a double evaluation adds, whose
               sum does not vanish where V does (i = 90 degrees, cos^2 i = 1/3, ...); H_scale = |H| with an interpolated height's and
               width's scales carried through the quotient.  Ids 12..14: the scale of |p| / (pi W)
    width      |a xi| + |b| with |b| <= |y_k| + |a x_k| and a's own |y_k+1| + |y_k| over |x_k+1 - x_k|
    quotients  (|f_c| + |half width| (with the width's scale) + |x_first| + step) / step

Every window edge and clip test also comes with the DISTANCE of the exact deciding quantity from its decision point (the nearest integer
for an edge, zero for a clip test) and that quantity's scale, so a test can tell a rounding-decided window from a wrong one.

`build(..., twin=True)` is the plain-double twin: the same steps in float64 in the straightforward order with libm, except the
visibilities, where it takes the device's formula (the Wigner sum over half-angle powers): more roundings than the closed form.  The twin's
distance from the definition in units of 2^-52 scale, r_twin, is the reference's own figure (tests/test_table_reference.py) and sets K.
"""
import math
from decimal import ROUND_CEILING, ROUND_FLOOR, Context, Decimal, localcontext
from fractions import Fraction

import numpy as np

from sampler_reference import PI, WORK, _sincos_small

PREC = 50
OK, ERR_EMPTY_WINDOW, ERR_NAN_WINDOW, ERR_BAD_MODEL = 0, -2, -3, -4
AJ, CLASSIC, LOCAL, V2, V3, HNLM = 23, 3, 11, 12, 13, 14
IDS = (CLASSIC, LOCAL, V2, V3, HNLM, AJ)
EPS = 2.0 ** -52
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ---------------------------------------------------------------------------------------------------------------- exact rationals

def pslm(s, l, m):
    """Pslm(s, l, m) of acoefs.cpp:51-110 (zero where the source's denominator vanishes or its degree condition fails)."""
    L = l * (l + 1)
    if s == 0:
        return Fraction(l)
    if s == 1:
        return Fraction(m)
    if s == 2:
        return Fraction(3 * m * m - L, 2 * l - 1) if l > 0 else Fraction(0)
    if s == 3:
        return Fraction(5 * m ** 3 - (3 * L - 1) * m, (l - 1) * (2 * l - 1)) if l > 1 else Fraction(0)
    if s == 4:
        h, c = 35 * m ** 4 - 5 * (6 * L - 5) * m * m + 3 * L * (L - 2), 2 * (l - 1) * (2 * l - 1) * (2 * l - 3)
    elif s == 5:
        h = 252 * m ** 5 - 140 * (2 * L - 3) * m ** 3 + (20 * L * (3 * L - 10) + 48) * m
        c = 8 * (4 * l ** 4 - 20 * l ** 3 + 35 * l ** 2 - 25 * l + 6)
    elif s == 6:
        h = 924 * m ** 6 - 420 * m ** 4 * (3 * L - 7) + 84 * m * m * (5 * L * L - 25 * L + 14) - 20 * L * (L * L - 8 * L + 12)
        c = 64 * l ** 5 - 480 * l ** 4 + 1360 * l ** 3 - 1800 * l ** 2 + 1096 * l - 240
    else:
        raise ValueError(s)
    return Fraction(h, c) if c != 0 else Fraction(0)


def qlm(l, m):
    """Qlm of build_lorentzian.cpp:583-592, the factor 2/3 included."""
    return Fraction(2, 3) * Fraction(l * (l + 1) - 3 * m * m, (2 * l - 1) * (2 * l + 3))


# ---------------------------------------------------------------------------------------------------------------- two arithmetics

class Exact:
    """Decimal at 50 digits (the caller holds the context)."""
    twin = False
    pi = PI

    @staticmethod
    def num(x):
        return Decimal(float(x))

    @staticmethod
    def lit(text):
        return Decimal(text)

    @staticmethod
    def frac(q):
        return Decimal(q.numerator) / Decimal(q.denominator)

    @staticmethod
    def floor(q):
        return int(q.to_integral_value(rounding=ROUND_FLOOR))

    @staticmethod
    def ceil(q):
        return int(q.to_integral_value(rounding=ROUND_CEILING))

    @staticmethod
    def sincos_deg(deg):
        """(sin, cos) of an angle in degrees: n quarter turns found exactly, the series sees |x| <= pi/4."""
        with localcontext() as c:
            c.prec = WORK
            n = int((deg / 90 + Decimal("0.5")).to_integral_value(rounding=ROUND_FLOOR))
            s, co = _sincos_small((deg - 90 * n) * PI / 180)
            s, co = ((s, co), (co, -s), (-s, -co), (-co, s))[n % 4]
        return +s, +co

    @staticmethod
    def atan_deg(y, x):
        """atan(y / x) in degrees, x and y doubles (x = 0: +-90 by the sign of y / x as IEEE division gives it)."""
        if x == 0:
            neg = (math.copysign(1.0, x) < 0) != (y < 0)
            return Decimal(-90 if neg else 90)
        with localcontext() as c:
            c.prec = WORK
            t = Decimal(y) / Decimal(x)
            sign, t = (-1 if t < 0 else 1), abs(t)
            inv = t > 1
            if inv:
                t = 1 / t
            k = 0
            while t > Decimal("0.05"):  # atan t = 2 atan(t / (1 + sqrt(1 + t^2)))
                t = t / (1 + (1 + t * t).sqrt())
                k += 1
            a, term, n, t2 = t, t, 1, t * t
            while abs(term) > Decimal(10) ** -(WORK + 2):
                term = -term * t2
                n += 2
                a += term / n
            a = a * (2 ** k)
            if inv:
                a = PI / 2 - a
            a = sign * a * 180 / PI
        return +a

    @classmethod
    def visibilities(cls, l, inc_deg):
        s, c = cls.sincos_deg(inc_deg)
        c2, s2 = c * c, s * s
        if l == 1:
            v = [c2, s2 / 2]
        elif l == 2:
            v = [(3 * c2 - 1) ** 2 / 4, 3 * c2 * s2 / 2, 3 * s2 * s2 / 8]
        else:
            v = [c2 * (5 * c2 - 3) ** 2 / 4, 3 * s2 * (5 * c2 - 1) ** 2 / 16, 15 * c2 * s2 * s2 / 8, 5 * s2 ** 3 / 16]
        return [v[abs(k - l)] for k in range(2 * l + 1)]


def _wigner_terms(l, m1, beta, f=float):
    """The terms of d^l_{m1,0}(beta) as a sum over half-angle powers (function_rot.cpp:60-92) and its normalisation."""
    ch, sh = math.cos(beta / 2.0), math.sin(beta / 2.0)
    terms = []
    for s in range(0, l - m1 + 1):
        t = float(math.comb(l, l - m1 - s) * math.comb(l, s)) * (-1.0) ** (l - m1 - s)
        terms.append(t * ch ** (2 * s + m1) * sh ** (2 * l - 2 * s - m1))
    return terms, math.sqrt(float(math.factorial(l + m1) * math.factorial(l - m1))) / math.sqrt(float(math.factorial(l) ** 2))


class Twin:
    """float64, straightforward order, libm."""
    twin = True
    pi = math.pi

    num = staticmethod(float)
    lit = staticmethod(float)

    @staticmethod
    def frac(q):
        return q.numerator / q.denominator

    @staticmethod
    def floor(q):
        return int(math.floor(q))

    @staticmethod
    def ceil(q):
        return int(math.ceil(q))

    @staticmethod
    def atan_deg(y, x):
        with np.errstate(all="ignore"):
            return float(np.arctan(np.float64(y) / np.float64(x))) * 180.0 / math.pi

    @staticmethod
    def visibilities(l, inc_deg):
        beta = math.pi * inc_deg / 180.0
        d = []
        for m in range(0, l + 1):
            terms, norm = _wigner_terms(l, m, beta)
            acc = 0.0
            for t in terms:
                acc = acc + t
            d.append(acc * norm)
        return [d[abs(k - l)] ** 2 for k in range(2 * l + 1)]


def visibility_scale(l, inc_deg):
    """(norm x sum |half-angle term|)^2 per component: what a rounding error of a double evaluation of V is proportional to."""
    beta = math.pi * float(inc_deg) / 180.0
    d = []
    for m in range(0, l + 1):
        terms, norm = _wigner_terms(l, m, beta)
        d.append(norm * sum(abs(t) for t in terms))
    return [d[abs(k - l)] ** 2 for k in range(2 * l + 1)]


# ---------------------------------------------------------------------------------------------------------------- pieces

class Layout:
    def __init__(self, pl):
        pl = [int(v) for v in pl]
        self.Nmax, self.lmax, self.Nfl = pl[0], pl[1], pl[2:6]
        self.Nsplit, self.Nwidth, self.Nnoise, self.Ninc = pl[6:10]
        self.o_vis = self.Nmax
        self.o_f = [self.Nmax + self.lmax + sum(self.Nfl[:l]) for l in range(4)]
        self.o_split = self.Nmax + self.lmax + sum(self.Nfl)
        self.o_width = self.o_split + self.Nsplit
        self.o_noise = self.o_width + self.Nwidth
        self.o_inc = self.o_noise + self.Nnoise
        self.o_cfg = self.o_inc + self.Ninc


def count_rows(model_id, pl):
    L = Layout(pl)
    if model_id in (AJ, LOCAL, HNLM):
        return sum(L.Nfl)
    return L.Nmax * (1 + min(max(L.lmax, 0), 3))


def _segment(xs, xi):
    """interpol.cpp:20-37 on the doubles themselves (comparisons of doubles are exact in either arithmetic)."""
    n = len(xs)
    if xi < xs[0]:
        return 0
    if xi > xs[n - 1]:
        return n - 2
    i = 0
    while i < n - 2 and (xi < xs[i] or xi > xs[i + 1]):
        i += 1
    return i


def _interpol(A, xs, ys, xi):
    """(value, scale) of the linear interpolation of (xs, ys) at xi; a NaN input gives (nan, nan) in either arithmetic."""
    if any(math.isnan(v) for v in list(xs) + list(ys) + [xi]):
        return None, float("nan")
    k = _segment(xs, xi)
    x0, x1, y0, y1, t = A.num(xs[k]), A.num(xs[k + 1]), A.num(ys[k]), A.num(ys[k + 1]), A.num(xi)
    a = (y1 - y0) / (x1 - x0)
    b = y0 - a * x0
    sa = (abs(ys[k + 1]) + abs(ys[k])) / abs(xs[k + 1] - xs[k])      # the terms of a
    scale = sa * abs(xi) + abs(ys[k]) + sa * abs(xs[k])                # |a xi| + |b| with the terms of a and b
    return a * t + b, float(scale)


def _slope_against_index(A, ys):
    """linfit.cpp:17-35 with x = 0 .. n-1: the slope."""
    n = len(ys)
    mx = A.frac(Fraction(n - 1, 2))
    sty = sum(((A.num(i) - mx) * A.num(y) for i, y in enumerate(ys)), A.num(0))
    stt = sum(((A.num(i) - mx) ** 2 for i in range(n)), A.num(0))
    return sty / stt


def _eta0(A, fl0):
    """models.cpp:6065-6084."""
    dnu = _slope_against_index(A, fl0)
    G, dnu_sun, r_sun, m_sun = A.lit("6.667e-8"), A.lit("135.1"), A.lit("6.96342e5"), A.lit("1.98855e30")
    R = r_sun * A.lit("1e5")
    rho_sun = m_sun * A.lit("1e3") / (4 * A.pi * R * R * R / 3)
    rho = (dnu / dnu_sun) ** 2 * rho_sun
    return 3 * A.pi / (rho * G)


def _window(A, grid, l, fc, gamma, g_scale, fs, fs_scale, c):
    """build_lorentzian.cpp:595-676.  gamma, fs, c, fc in the arithmetic A (gamma and fs may be computed quantities: their scales say how
    far a double evaluation of them may sit from the exact one).  Returns (status, i0, i1, edges): edges = [(name, distance, scale)]."""
    x_first, x_last, Nx, step = A.num(grid.x_first), A.num(grid.x_last), grid.Nx, A.num(grid.step)
    lo = hi = None
    one = A.num(1)
    two2 = A.lit("2.2")
    if gamma >= one and fs >= one:
        h = c * (l * fs + gamma) if l != 0 else c * gamma * two2
        lo, hi = fc - h, fc + h
    if gamma <= one and fs >= one:
        h = c * (l * fs + 1) if l != 0 else c * two2
        lo, hi = fc - h, fc + h
    if gamma >= one and fs <= one:
        h = c * (l + gamma) if l != 0 else c * two2 * gamma
        lo, hi = fc - h, fc + h
    if gamma <= one and fs <= one:
        h = c * (l + 1) if l != 0 else c * two2
        lo, hi = fc - h, fc + h
    if lo is None:
        return ERR_NAN_WINDOW, 0, 0, []
    fcf, cf, stepf = abs(float(fc)), abs(float(c)), abs(float(step))
    # what the half width's rounding error is proportional to (the regimes meet continuously at 1: no decision to miss there)
    hs = cf * (l * max(abs(float(fs)), 1.0) + l * fs_scale + max(abs(float(gamma)), 1.0) + g_scale) * (1.0 if l != 0 else 2.2)
    qs = (fcf + hs + abs(float(x_first)) + stepf) / stepf
    edges = []
    t1 = (hi - step) - x_first
    edges.append(("clip_hi", abs(float(t1)), fcf + hs + stepf + abs(float(x_first))))
    if t1 < 0:
        hi = x_first + c
    t2 = (lo + step) - x_last
    edges.append(("clip_lo", abs(float(t2)), fcf + hs + stepf + abs(float(x_last))))
    if t2 >= 0:
        lo = x_last - c
    q0, q1 = (lo - x_first) / step, (hi - x_first) / step
    a = min(max(A.floor(q0), INT_MIN), INT_MAX)
    b = min(max(A.ceil(q1), INT_MIN), INT_MAX)
    for name, q in (("i0", q0), ("i1", q1)):
        r = q - (A.floor(q + A.frac(Fraction(1, 2))))
        # (beyond the clamp to [0, Nx] an edge decides nothing: floor near 0 and ceil near Nx are clamped to the same index)
        inside = (0.5 < float(q) < Nx + 0.5) if name == "i0" else (-0.5 < float(q) < Nx - 0.5)
        edges.append((name, abs(float(r)) if inside else float("inf"), qs))
    a, b = max(a, 0), min(b, Nx)
    if b - a <= 0:
        return ERR_EMPTY_WINDOW, a, b, edges
    return OK, a, b, edges


class Grid:
    """The frequency axis as the builders see it: first and last abscissa, bin count, step = x[1] - x[0] in double."""

    def __init__(self, x):
        x = np.asarray(x, dtype=np.float64)
        self.x, self.Nx = x, int(x.size)
        self.x_first, self.x_last, self.step = float(x[0]), float(x[-1]), float(x[1] - x[0])


# ---------------------------------------------------------------------------------------------------------------- the table

def build(model_id, params, plength, grid, twin=False):
    """Reference table of one parameter vector.  Returns a dict: status, rows (empty unless status is OK), noise (|p|, the doubles
    themselves), nharvey, nnoise.  A row: l, fc, asym (the input doubles), gamma, gamma_scale (0.0: gamma is an input's magnitude),
    nu[7], nu_scale[7], hv[7], hv_scale[7], i0, i1, edges.  Magnitudes are Decimal (float for the twin); unused entries are 0."""
    if not isinstance(grid, Grid):
        grid = Grid(grid)
    if twin:
        with np.errstate(all="ignore"):
            return _build(Twin, model_id, params, plength, grid)
    with localcontext(Context(prec=PREC)):
        return _build(Exact, model_id, params, plength, grid)


def _build(A, model_id, params, plength, grid):
    p = [float(v) for v in params]
    L = Layout(plength)
    per = count_rows(model_id, plength)
    classic = model_id in (CLASSIC, V2, V3)
    sp = L.o_split
    trunc_c, do_amp = p[L.o_cfg], p[L.o_cfg + 1] != 0
    fl0, Wl0 = p[L.o_f[0]:L.o_f[0] + L.Nfl[0]], p[L.o_width:L.o_width + L.Nfl[0]]
    out = {"status": OK, "rows": [], "noise": [abs(v) for v in p[L.o_noise:L.o_noise + L.Nnoise]], "nnoise": L.Nnoise,
           "nharvey": 0 if model_id in (LOCAL, HNLM) else int((L.Nnoise - 1) / 3)}
    # ---- shared scalars
    inc = None
    if model_id in (AJ, CLASSIC):
        inc = A.num(p[L.o_inc])
    elif model_id == LOCAL:
        inc = A.atan_deg(p[sp + 4], p[sp + 3])
    ratios, rscale = {0: [A.num(1)]}, {0: [1.0]}
    for l in range(1, 4):
        if inc is not None and (L.lmax >= l if model_id != LOCAL else L.Nfl[l] >= 1):
            ratios[l], rscale[l] = A.visibilities(l, inc), visibility_scale(l, inc)
        elif model_id == V2:
            b = (0, 2, 5)[l - 1]
            ratios[l] = [A.num(abs(p[L.o_inc + b + abs(k - l)])) for k in range(2 * l + 1)]
            rscale[l] = [float(v) for v in ratios[l]]
    if model_id in (LOCAL, HNLM):
        Vl = [1.0] * 4                                                   # (no degree visibilities in the local models)
    else:
        Vl = [1.0] + [abs(p[L.o_vis + l - 1]) if L.lmax >= l else 0.0 for l in range(1, 4)]
    if model_id == AJ:
        asym = p[sp + 13]
        eta0 = _eta0(A, fl0) if p[sp + 12] == 1 else A.num(0)
        a1 = a3 = None
    elif classic:
        a1, a3, asym, eta0 = A.num(abs(p[sp])), A.num(p[sp + 2]), p[sp + 5], _eta0(A, fl0)
    elif model_id == LOCAL:
        a1 = A.num(p[sp + 3]) ** 2 + A.num(p[sp + 4]) ** 2
        eta0, a3, asym = A.num(p[sp + 1]), A.num(p[sp + 2]), p[sp + 5]
    else:
        a1, eta0, a3, asym = A.num(abs(p[sp])), A.num(p[sp + 1]), A.num(p[sp + 2]), p[sp + 5]
    micro, milli = A.lit("1e-6"), A.lit("1e-3")
    # ---- rows
    for index in range(per):
        if classic:
            per_n = 1 + min(max(L.lmax, 0), 3)
            n, l = divmod(index, per_n)
        else:
            l, n = 0, index
            while l < 3 and n >= L.Nfl[l]:
                n -= L.Nfl[l]
                l += 1
        off = sum(L.Nfl[:l])
        g_scale = 0.0
        a = [A.num(0)] * 7
        if model_id == AJ or classic:
            fc = p[L.o_f[l] + n]
            if l == 0:
                Wd, W = abs(Wl0[n]), A.num(abs(Wl0[n]))
                Hraw, h_scale = A.num(p[n]), abs(p[n])
            else:
                W, g_scale = _interpol(A, fl0, Wl0, fc)
                Wd = float("nan") if W is None else abs(float(W))
                W = None if W is None else abs(W)
                if model_id == AJ:
                    Hraw, h_scale = _interpol(A, fl0, p[0:L.Nfl[0]], fc)
                    a = [A.num(0)] + [A.num(p[sp + 2 * (j - 1)]) + A.num(p[sp + 2 * (j - 1) + 1]) * (A.num(fc) * milli) if j <= 2 * l
                                      else A.num(0) for j in range(1, 7)]
                else:
                    Hraw, h_scale = A.num(p[n]), abs(p[n])
            fs = a[1] if model_id == AJ else a1
            fs_scale = (abs(p[sp]) + abs(p[sp + 1] * fc * 1e-3)) if (model_id == AJ and l > 0) else 0.0
        else:
            fc, Wd = p[L.o_f[0] + off + n], abs(p[L.o_width + off + n])
            W = A.num(Wd)
            Hraw, h_scale = A.num(p[off + n]), abs(p[off + n])
            fs, fs_scale = a1, (float(a1) if model_id == LOCAL else 0.0)
        if W is None or math.isnan(Wd) or math.isnan(float(fs)) or math.isnan(fc):
            out["status"], out["rows"] = ERR_NAN_WINDOW, []
            return out
        st, i0, i1, edges = _window(A, grid, l, A.num(fc), W, g_scale, fs, fs_scale, A.num(trunc_c))
        if st != OK:
            out["status"], out["rows"], out["failed_edges"] = st, [], edges
            return out
        # heights
        if do_amp:
            H = abs(Hraw / (A.pi * W)) * A.num(Vl[l])
            Hs = (h_scale / (math.pi * Wd) * (1.0 + g_scale / Wd) * Vl[l]) if Wd > 0 else float("inf")
        else:
            H, Hs = abs(Hraw * A.num(Vl[l])), h_scale * Vl[l]
        row = {"l": l, "fc": fc, "asym": asym, "gamma": W, "gamma_scale": g_scale, "i0": i0, "i1": i1, "edges": edges, "flags": 0,
               "nu": [A.num(0)] * 7, "hv": [A.num(0)] * 7, "nu_scale": [0.0] * 7, "hv_scale": [0.0] * 7}
        for k in range(2 * l + 1):
            m = k - l
            f = A.num(fc)
            if l == 0:
                nu, ns = f, 0.0
            elif model_id == AJ:
                terms = [a[j] * A.frac(pslm(j, l, m)) for j in range(1, 7)]
                eta = f * eta0 * A.frac(qlm(l, m)) * (a[1] * micro) ** 2 if eta0 > 0 else A.num(0)
                nu = f + sum(terms, A.num(0)) + eta
                ns = abs(fc) + abs(float(eta)) + sum(
                    (abs(p[sp + 2 * (j - 1)]) + abs(p[sp + 2 * (j - 1) + 1] * fc * 1e-3)) * abs(float(pslm(j, l, m))) for j in range(1, 2 * l + 1))
            else:
                eta = f * eta0 * (fs * micro) ** 2 * A.frac(qlm(l, m))
                t3 = A.frac(pslm(3, l, m)) * a3
                nu = f + eta + m * fs + t3
                ns = abs(fc) + abs(float(eta)) + abs(m) * (float(fs) + fs_scale) + abs(float(t3))
            row["nu"][k], row["nu_scale"][k] = nu, ns
            if model_id in (V3, HNLM) and l >= 1:
                hb = (L.o_inc + (l + 1) * n) if model_id == V3 else (off + (l + 1) * n)
                v = abs(p[hb + abs(m)])
                hv = abs(A.num(v) / (A.pi * W)) if do_amp else A.num(v)
                hs = (v / (math.pi * Wd) * (1.0 + g_scale / Wd) if Wd > 0 else float("inf")) if do_amp else 0.0
            else:
                hv, hs = H * ratios[l][k], Hs * rscale[l][k]
            row["hv"][k], row["hv_scale"][k] = hv, hs
        out["rows"].append(row)
    return out


# ---------------------------------------------------------------------------------------------------------------- comparisons

def ratio(got, ref, scale):
    """|got - ref| in units of 2^-52 scale; 0 when both are exactly equal (a zero scale included), inf when they differ at scale 0."""
    with localcontext(Context(prec=PREC)):
        d = abs(Decimal(float(got)) - Decimal(ref if isinstance(ref, Decimal) else float(ref)))
        if d == 0:
            return 0.0
        if not scale > 0 or math.isinf(scale):
            return float("inf") if not scale > 0 else 0.0
        return float(d / (Decimal(scale) * Decimal(EPS)))


def knife_edges(ref, K):
    """The (row index, edge name) pairs of a reference table whose deciding quantity lies within K 2^-52 scale of its decision point --
    computed from the reference alone.  A failed vector reports the edges of the row that failed as row -1."""
    hits = []
    for i, row in enumerate(ref["rows"]):
        hits += [(i, name) for name, dist, scale in row["edges"] if dist <= K * EPS * scale]
    hits += [(-1, name) for name, dist, scale in ref.get("failed_edges", []) if dist <= K * EPS * scale]
    return hits

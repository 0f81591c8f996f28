"""50-digit restatement of the red-giant pre-step (model ids 25 and 27): parameter vector -> mixed modes -> table.

Written from the reference project's sources, for MEANING, with `decimal` at 50 significant digits; no line of csrc/ or oracle/ is used.

    model_RGB_asympt_aj_AppWidth_HarveyLike_v4, _CteWidth_      models.cpp:4684-5079, :4334-4682
    solve_mm_asymptotic_O2p, _O2from_l0, solver_mm, sign_change external/ARMM/solver_mm.cpp:82-121, :340-449, :470-604, :624-755
    lin_interpol (solver: x = p - g, y = nu, at 0)              external/ARMM/interpol.cpp:21-50
    ksi_fct1, ksi_fct2_precise, gamma_l_fct2, h_l_rgb           external/ARMM/bump_DP.cpp:46-64, :125-180, :203-253
    Frstder_adaptive_reggrid (index grid)                       external/ARMM/derivatives_handler.cpp:425-444
    tk::spline, natural ends, cspline / cspline_hermite         external/spline/src/spline.h:219-240, :242-415, :467-499
    linfit                                                      linfit.cpp:17-35

Two layers, as in tile_reference / table_reference.  `Ex` (Decimal, 50 digits) is the definition.  `Tw` (numpy.longdouble) is its twin:
the same statements in extended precision.  The twin also does the definition's BULK passes -- the walk of the `resol` grid, the local
grids, the 4-year zeta grid -- because they only LOCATE things: every point that decides or enters a result (both ends of a sign-change
cell, f_first, f_last, the bracketing pair, the top points of the zeta grid) is then evaluated in Decimal, and every decision the bulk
pass took comes with its margin (below), so a bulk pass that could have decided differently at 50 digits is visible.

Identity used (exact, shown at 50 digits by tests/test_rgb_reference.py): 1e6 / (nu_g DPl) = n_g + alpha, so
tan(pi 1e6 (1/nu - 1/nu_g) / DPl) and cos^2 of the same argument do not depend on WHICH g mode of the ladder is taken.  The reference's
pair loop therefore returns, for a p mode with at least one g mode inside its zone, the same roots once per such g mode (std::unique
drops the copies), and the inner sum of zeta over the g modes is L_g times one term.  `zeta_sum(..., literal=True)` is the double loop
of bump_DP.cpp:138-150 as written; build() uses the identity.

ROUNDING-DECIDED BY CONSTRUCTION.  The local grid has long((range_max - range_min) / (resol factor)) points and range_max - range_min is
4 resol: the exact quotient is the integer 4 / factor (100, 400, 800).  In double the count is that integer or one less depending on the
rounding of nu[idx] +- 2 resol: no arithmetic can be "right" about it.  The reference therefore refines every cell on BOTH grids and a
root carries both results (`alts`); a comparison takes, per root, the alternative nearer to what it got, and everything downstream
(zeta, heights, widths, rows) is rebuilt at that choice (`finish(sol, choice)`).

ERROR SCALES.  Every value comes with the quantity a double evaluation's rounding error is proportional to: the sum of
|df/dt| |t| over the rounded intermediates t (partial sums included).  A comparison is |got - ref| <= K 2^-52 scale.

    p - g at nu   2 nu (1 + G c/nu^2) + G c (1/nu + 4/nu_g) + 4 G |X| + 2 (Dl/pi) q |T| / (1 + u^2) + 3 |g| + S(nu_p) + |p| + |f|
                  + S(Dl) |atan u| / pi, with X the argument of tan, T = tan X, u = q T, c = pi 1e6 / DPl,
                  G = (Dl / pi) q (1 + T^2) / (1 + u^2): the cancelling difference 1/nu - 1/nu_g and the factor 1 + tan^2 X are in it
    root          (|f_b| S(f_a) + |f_a| S(f_b)) / ((f_b - f_a) slope) + 3 |nu|, (a, b) the bracketing pair, slope = (f_b - f_a)/(x_b - x_a)
    zeta term     through d/d(up), d/d(down), d/d(front) of cd^2 / (cd^2 + front cu^2), the root's own scale carried through d/dnu

KNIFE EDGES.  Every decision returns (name, distance of the exact deciding quantity from its decision point, that quantity's scale);
`knife_edges(sol, K_EDGE)` lists those inside K_EDGE 2^-52 scale.
"""
import math
from decimal import ROUND_CEILING, ROUND_DOWN, ROUND_FLOOR, Context, Decimal, localcontext

import numpy as np

import table_reference as tr
from sampler_reference import PI, WORK, _sincos_small

LD = np.longdouble
PREC = tr.PREC
EPS = 2.0 ** -52
OK, ERR_BAD_ARG = 0, -5
ID_APP, ID_CTE = 25, 27
MAXP, CAP1, MAXNODE, MAXL = 32, 400, 16, 32        # the product's stated limits (include/tamcmc_hip.h): part of its contract, not of the model
PI_LD = LD("3.14159265358979323846264338327950288")
INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------- two arithmetics

class Ex(tr.Exact):
    """Decimal at 50 digits (the caller holds the context); series at WORK digits."""

    @staticmethod
    def trunc(q):
        return int(q.to_integral_value(rounding=ROUND_DOWN))

    @staticmethod
    def sincos(x):
        with localcontext() as c:
            c.prec = WORK
            n = int((x / (PI / 2) + Decimal("0.5")).to_integral_value(rounding=ROUND_FLOOR))
            s, co = _sincos_small(x - n * PI / 2)
            s, co = ((s, co), (co, -s), (-s, -co), (-co, s))[n % 4]
        return +s, +co

    @classmethod
    def tan(cls, x):
        s, c = cls.sincos(x)
        return s / c

    @classmethod
    def cos(cls, x):
        return cls.sincos(x)[1]

    @staticmethod
    def atan(t):
        with localcontext() as c:
            c.prec = WORK
            sign, t = (-1 if t < 0 else 1), abs(t)
            inv = t > 1
            if inv:
                t = 1 / t
            k = 0
            while t > Decimal("0.05"):              # atan t = 2 atan(t / (1 + sqrt(1 + t^2)))
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
            a = sign * a
        return +a

    sqrt = staticmethod(lambda x: x.sqrt())
    ln = staticmethod(lambda x: x.ln())
    exp = staticmethod(lambda x: x.exp())


class Tw:
    """numpy.longdouble, the statements in the straightforward order."""
    twin = True
    pi = PI_LD
    num = staticmethod(lambda x: LD(float(x)))
    lit = staticmethod(lambda t: LD(t))
    frac = staticmethod(lambda q: LD(q.numerator) / LD(q.denominator))
    floor = staticmethod(lambda q: int(np.floor(q)))
    ceil = staticmethod(lambda q: int(np.ceil(q)))
    trunc = staticmethod(lambda q: int(np.trunc(q)))
    tan, atan, cos, sqrt, ln, exp = (staticmethod(f) for f in (np.tan, np.arctan, np.cos, np.sqrt, np.log, np.exp))

    @staticmethod
    def sincos_deg(deg):
        a = PI_LD * deg / 180
        return np.sin(a), np.cos(a)

    visibilities = classmethod(tr.Exact.visibilities.__func__)


def _f(v):
    return float(v)


def _sum(A, terms):
    """(sum in the stated order, scale): the scale counts every term and every partial sum."""
    s, sc = A.num(0), 0.0
    for k, t in enumerate(terms):
        s = s + t
        sc += abs(_f(t)) + (abs(_f(s)) if k else 0.0)
    return s, sc


class RGrid(tr.Grid):
    """The frequency axis as the red-giant models see it: step = x[2] - x[1] (models.cpp:4714), used by the solver and the windows."""

    def __init__(self, x):
        super().__init__(x)
        self.step = float(self.x[2] - self.x[1])


# ---------------------------------------------------------------------------------------------------------------- (a) the scalar unpack

class Layout:
    def __init__(self, pl):
        pl = [int(v) for v in pl]
        (self.Nmax, self.lmax, self.Nfl0, self.Nfl1, self.Nfl2, self.Nfl3, self.Nsplit, self.Nwidth, self.Nnoise, self.Ninc) = pl[:10]
        self.Nf = self.Nfl0 + self.Nfl1 + self.Nfl2 + self.Nfl3
        self.o0 = self.Nmax + self.lmax
        self.o1 = self.o0 + self.Nfl0
        self.o2 = self.o1 + self.Nfl1
        self.o3 = self.o2 + self.Nfl2
        self.os = self.o0 + self.Nf
        self.ow = self.os + self.Nsplit
        self.on = self.ow + self.Nwidth
        self.oi = self.on + self.Nnoise
        self.oc = self.oi + self.Ninc


def width_law(A, g, f):
    """models.cpp:4788-4794: (W, scale).  g: six doubles (magnitudes), f a double."""
    g0, g1, g2, g3, g4, g5 = (A.num(v) for v in g)
    t1 = g2 * A.ln(A.num(f) / g0)
    den = A.ln(g4 / g0)
    e = 2 * A.ln(A.num(f) / g1) / den
    L5 = A.ln(g5) / (1 + e * e)
    lnW = t1 + A.ln(g3) - L5
    W = A.exp(lnW)
    ef, df = abs(_f(e)), abs(_f(den))
    s_e = 3 * ef + 2 / df + ef / df
    s_ln = 3 * abs(_f(t1)) + abs(g[2]) + abs(math.log(g[3])) + abs(_f(L5)) * (3 + 2 * ef / (1 + ef * ef) * s_e) + 2 * abs(_f(lnW))
    return W, _f(W) * (s_ln + 1.0)


def _edge(edges, name, dist, scale):
    edges.append((name, abs(float(dist)), float(scale)))


def _int_dist(A, q):
    return abs(_f(q - A.floor(q + A.frac(tr.Fraction(1, 2)))))


def unpack(A, model_id, params, plength, step):
    """Stage (a).  Returns a dict; 'status' != OK: a refusal (the other entries may be missing)."""
    p = [float(v) for v in params]
    L = Layout(plength)
    cte = model_id == ID_CTE
    U = {"status": OK, "edges": [], "L": L, "p": p, "cte": cte, "no_modes": False, "resol": float(step)}
    E = U["edges"]

    def refuse():
        U["status"] = ERR_BAD_ARG
        return U
    do_amp = p[L.oc + 1] != 0
    model_type, bias_type, Nferr = p[L.oc + 3], p[L.oc + 4], int(p[L.oc + 5])
    U.update(do_amp=do_amp, model_type=model_type, bias_type=bias_type, Nferr=Nferr, trunc_c=p[L.oc])
    if (L.Nmax < 2 or L.Nmax != L.Nfl0 or Nferr < 0 or L.Nfl1 != 8 + 2 * Nferr or L.Nwidth < (1 if cte else 6) or L.Nsplit < 10 or L.lmax > 3
            or L.Nfl0 > MAXL or L.Nfl2 > MAXL or L.Nfl3 > MAXL):
        return refuse()
    g = [abs(p[L.ow + k]) if k < (1 if cte else 6) else 0.0 for k in range(6)]
    fl0 = p[L.o0:L.o0 + L.Nfl0]
    fmin, fmax = min(fl0), max(fl0)
    U.update(g=g, fl0=fl0, fmin=fmin, fmax=fmax)
    # widths and heights of the radial modes
    W0, W0s, H0, H0s = [], [], [], []
    for n in range(L.Nmax):
        W, Ws = (A.num(g[0]), 0.0) if cte else width_law(A, g, fl0[n])
        W0.append(W)
        W0s.append(Ws)
        if do_amp:
            h = abs(A.num(p[n]) * (1 / W / A.pi))
            H0.append(h)
            H0s.append(_f(h) * (Ws / _f(W) + 3.0))
        else:
            H0.append(A.num(abs(p[n])))
            H0s.append(0.0)
    U.update(W0=W0, W0s=W0s, H0=H0, H0s=H0s)
    # the l=1 block and the fit of the radial ladder against the index (linfit.cpp:17-35)
    d0l, DPl, alpha, q = p[L.o1], abs(p[L.o1 + 1]), abs(p[L.o1 + 2]), abs(p[L.o1 + 3])
    U.update(d0l=d0l, DPl=DPl, alpha=alpha, q=q, Wfactor=abs(p[L.o1 + 6]), Hfactor=abs(p[L.o1 + 7]))
    n = L.Nfl0
    mx = A.frac(tr.Fraction(n - 1, 2))
    sty, s_sty = _sum(A, [(A.num(i) - mx) * A.num(y) for i, y in enumerate(fl0)])
    stt = sum(((A.num(i) - mx) ** 2 for i in range(n)), A.num(0))
    Dnu = sty / stt
    s_Dnu = s_sty / _f(stt) + abs(_f(Dnu))
    sy, s_sy = _sum(A, [A.num(y) for y in fl0])
    sx = n * (n - 1) // 2
    c = (sy - sx * Dnu) / n
    s_c = (s_sy + sx * s_Dnu + abs(sx * _f(Dnu)) + abs(_f(sy - sx * Dnu))) / n + abs(_f(c))
    U.update(Dnu=Dnu, s_Dnu=s_Dnu, c=c, s_c=s_c)
    _edge(E, "Dnu>0", Dnu, s_Dnu)
    if not Dnu > 0:
        return refuse()
    fmin_s, fmax_s = A.num(fmin) - Dnu, A.num(fmax) + Dnu
    s_fmin_s, s_fmax_s = s_Dnu + abs(_f(fmin_s)), s_Dnu + abs(_f(fmax_s))
    _edge(E, "fmin-Dnu<0", fmin_s, s_fmin_s)
    if fmin_s < 0:
        return refuse()         # models.cpp:4852-4858 exits.  Id 27 tests it for model_type 0 only and would otherwise run 1e6/(0 DPl): undefined, refused too
    fDnu = _f(Dnu)

    def g_count(f, s_f, up):
        v = A.lit("1e6") / (f * A.num(DPl)) - A.num(alpha)
        big = abs(1e6 / (_f(f) * DPl))
        s = big * (2 + s_f / abs(_f(f))) + alpha + abs(_f(v))
        _edge(E, "ng_max" if up else "ng_min", _int_dist(A, v), s)
        return A.ceil(v) if up else A.floor(v)
    if fmin_s == 0:
        return refuse()
    ng_min, ng_max = g_count(fmax_s, s_fmax_s, False), g_count(fmin_s, s_fmin_s, True)
    nu_p, s_nu_p = [], []
    if ng_min <= 0 and ng_max < 1:
        U["no_modes"] = True        # "impossible star": the solver returns an empty structure and the model carries on (solver_mm.cpp:503-507)
    else:
        if ng_min <= 0:
            ng_min = 1
        few = ng_max - ng_min < 6
        U["few_g"] = few
        if model_type == 0:
            e0 = c / Dnu
            s_e0 = s_c / fDnu + abs(_f(e0)) * (s_Dnu / fDnu + 1)
            _edge(E, "n0", _int_dist(A, e0), s_e0)
            n0 = A.floor(e0)
            eps = e0 - n0
            s_eps = s_e0 + abs(_f(eps))
            U.update(n0=n0, eps=eps, s_eps=s_eps)
            lim = []
            for f, s_f, up in ((fmin_s, s_fmin_s, False), (fmax_s, s_fmax_s, True)):
                v = f / Dnu - eps - 0 - A.num(d0l)                       # el/2 with el = 1: INTEGER division in the source, 0
                r = abs(_f(f / Dnu))
                s = r * (1 + s_f / max(abs(_f(f)), 1e-300) + s_Dnu / fDnu) + s_eps + abs(d0l) + 3 * abs(_f(v))
                _edge(E, "np_max" if up else "np_min", _int_dist(A, v), s)
                lim.append(A.ceil(v) if up else A.floor(v))
            np_min, np_max = lim                                           # (alpha_p = 0: the second pass over np_min / np_max changes nothing)
            zone = A.num(np_max) if few else A.lit("1.75")
            if np_min <= 0:
                np_min = 1
            Lp, Lg = np_max - np_min, ng_max - ng_min
            if Lg < 1:
                U["no_modes"] = True
            else:
                if Lp < 1 or Lp > MAXP:
                    return refuse()
                for k in range(np_min, np_max):
                    t = k + eps + A.frac(tr.Fraction(1, 2)) + A.num(d0l)
                    v = t * Dnu
                    nu_p.append(v)
                    s_nu_p.append((abs(k) + abs(_f(eps)) + s_eps + 0.5 + abs(d0l) + 3 * abs(_f(t))) * fDnu + abs(_f(t)) * s_Dnu + abs(_f(v)))
                U.update(keep_lo=fmin_s, keep_hi=fmax_s, s_keep_lo=s_fmin_s, s_keep_hi=s_fmax_s)
        else:
            zone = A.num(20) if few else A.lit("1.75")
            shift = Dnu / 2 + A.num(d0l)
            s_shift = s_Dnu + abs(d0l) + abs(_f(shift))
            ext = [(A.num(fmin) - (3 - k) * Dnu, (3 - k) * s_Dnu) for k in range(3)] + [(A.num(v), 0.0) for v in fl0] + \
                  [(A.num(fmax) + k * Dnu, k * s_Dnu) for k in (1, 2, 3)]
            for k, (e, s_e) in enumerate(ext):
                v = e + shift
                s_v = s_e + abs(_f(e)) * (s_e > 0) + s_shift + abs(_f(v))
                _edge(E, f"ladder[{k}]>=fmin_s", v - fmin_s, s_v + s_fmin_s)
                _edge(E, f"ladder[{k}]<=fmax_s", v - fmax_s, s_v + s_fmax_s)
                if fmin_s <= v <= fmax_s:
                    nu_p.append(v)
                    s_nu_p.append(s_v)
            if len(nu_p) > MAXP:
                return refuse()
            if ng_max - ng_min < 1:
                U["no_modes"] = True
            elif len(nu_p) < 2:
                return refuse()     # Frstder_adaptive_reggrid needs two points
            U.update(keep_lo=A.num(fmin), keep_hi=A.num(fmax), s_keep_lo=0.0, s_keep_hi=0.0)
        U.update(zone=zone, ng_min=ng_min, Lg=ng_max - ng_min)
    fact = "0.04"
    for thr, val in ((150, "0.01"), (50, "0.005")):
        _edge(E, f"fmin_s<={thr}", fmin_s - thr, s_fmin_s)
        if fmin_s <= thr:
            fact = val
    U["fact"] = fact
    if U["no_modes"]:
        nu_p, s_nu_p = [], []
    Lp = len(nu_p)
    dnup, s_dnup = [], []
    for i in range(Lp):
        if Lp == 1:
            d, s = A.num(0), 0.0
        elif i == 0:
            d, s = nu_p[1] - nu_p[0], s_nu_p[1] + s_nu_p[0]
        elif i == Lp - 1:
            d, s = nu_p[i] - nu_p[i - 1], s_nu_p[i] + s_nu_p[i - 1]
        else:
            d, s = (nu_p[i + 1] - nu_p[i - 1]) / 2, (s_nu_p[i + 1] + s_nu_p[i - 1]) / 2
        dnup.append(d)
        s_dnup.append(s + abs(_f(d)))
    if model_type == 0:
        dnu_loc, s_dnu_loc = [Dnu] * Lp, [s_Dnu] * Lp
    else:
        dnu_loc, s_dnu_loc = dnup, s_dnup
    U.update(nu_p=nu_p, s_nu_p=s_nu_p, dnup=dnup, s_dnup=s_dnup, dnu_loc=dnu_loc, s_dnu_loc=s_dnu_loc, Lp=Lp)
    # first g mode inside the zone of each p mode (solver_mm.cpp:348: a pair is solved when numin <= nu_g <= numax)
    ig0 = []
    for i in range(Lp):
        lo, hi = nu_p[i] - zone * Dnu, nu_p[i] + zone * Dnu
        s_z = s_nu_p[i] + _f(zone) * (s_Dnu + fDnu)
        ig0.append(_first_g(A, U, lo, hi, s_z + abs(_f(lo)), s_z + abs(_f(hi)), i))
    U["ig0"] = ig0
    # the bias spline
    U["spline"] = None
    if bias_type != 0:
        xs, ys = p[L.o1 + 8:L.o1 + 8 + Nferr], p[L.o1 + 8 + Nferr:L.o1 + 8 + 2 * Nferr]
        if Nferr < 3 or Nferr > MAXNODE or any(not xs[i] < xs[i + 1] for i in range(Nferr - 1)):
            return refuse()
        U["spline"] = spline_set(A, xs, ys, 1 if bias_type == 1 else 2)
    # what the rows need
    inc = abs(p[L.oi])
    U["Vl"] = [1.0] + [abs(p[L.Nmax + l - 1]) if l <= L.lmax else 0.0 for l in (1, 2, 3)]
    U["V"] = {0: [A.num(1)]}
    U["Vs"] = {0: [1.0]}
    for l in range(1, L.lmax + 1):
        U["V"][l], U["Vs"][l] = A.visibilities(l, A.num(inc)), tr.visibility_scale(l, inc)
    U["eta0"] = tr._eta0(A, fl0) if p[L.os + 8] == 1 else A.num(0)
    U.update(rot_env=abs(p[L.os]), rot_core=abs(p[L.os + 1]), a=[0.0, 0.0, p[L.os + 2], p[L.os + 4], p[L.os + 5], p[L.os + 6], p[L.os + 7]],
             asym=p[L.os + 9], noise=[abs(v) for v in p[L.on:L.on + L.Nnoise]], nharvey=int((L.Nnoise - 1) / 3), nnoise=L.Nnoise,
             fl2=[abs(v) for v in p[L.o2:L.o2 + L.Nfl2]], fl3=[abs(v) for v in p[L.o3:L.o3 + L.Nfl3]])
    return U


def nu_g_of(A, U, ig):
    """asympt_nu_g (solver_mm.cpp:313-317) of the ladder's mode ig."""
    return A.lit("1e6") / ((U["ng_min"] + ig + A.num(U["alpha"])) * A.num(U["DPl"]))


def _first_g(A, U, lo, hi, s_lo, s_hi, i):
    Lg, E = U["Lg"], U["edges"]
    est = A.lit("1e6") / (hi * A.num(U["DPl"])) - A.num(U["alpha"]) - U["ng_min"]      # nu_g(k) <= hi  <=>  k >= est
    k = min(max(A.ceil(est), 0), Lg)
    for kk in (k - 1, k):
        if 0 <= kk < Lg:
            v = nu_g_of(A, U, kk)
            _edge(E, f"first_g[{i}]<=hi", v - hi, s_hi + 4 * abs(_f(v)))
    while k > 0 and nu_g_of(A, U, k - 1) <= hi:
        k -= 1
    while k < Lg and not nu_g_of(A, U, k) <= hi:
        k += 1
    if k >= Lg:
        return -1
    v = nu_g_of(A, U, k)
    _edge(E, f"first_g[{i}]>=lo", v - lo, s_lo + 4 * abs(_f(v)))
    return k if v >= lo else -1


# ---------------------------------------------------------------------------------------------------------------- (c) the bias spline

def spline_set(A, xs, ys, kind):
    """tk::spline::set_points with second derivatives 0 at both ends; kind 1: cspline (the tridiagonal system solved exactly in order),
    kind 2: cspline_hermite.  Returns the coefficient lists (A's numbers) and the figures the scale needs."""
    n = len(xs)
    x, y = [A.num(v) for v in xs], [A.num(v) for v in ys]
    b, c, d = [A.num(0)] * n, [A.num(0)] * n, [A.num(0)] * n
    three = A.num(3)
    if kind == 1:
        sub = [A.num(0)] + [(x[i] - x[i - 1]) / three for i in range(1, n - 1)] + [A.num(0)]
        dia = [A.num(2)] + [2 * (x[i + 1] - x[i - 1]) / three for i in range(1, n - 1)] + [A.num(2)]
        sup = [A.num(0)] + [(x[i + 1] - x[i]) / three for i in range(1, n - 1)] + [A.num(0)]
        rhs = [A.num(0)] + [(y[i + 1] - y[i]) / (x[i + 1] - x[i]) - (y[i] - y[i - 1]) / (x[i] - x[i - 1]) for i in range(1, n - 1)] + [A.num(0)]
        for i in range(1, n):
            w = sub[i] / dia[i - 1]
            dia[i] = dia[i] - w * sup[i - 1]
            rhs[i] = rhs[i] - w * rhs[i - 1]
        c[n - 1] = rhs[n - 1] / dia[n - 1]
        for i in range(n - 2, -1, -1):
            c[i] = (rhs[i] - sup[i] * c[i + 1]) / dia[i]
        for i in range(n - 1):
            h = x[i + 1] - x[i]
            d[i] = (c[i + 1] - c[i]) / (three * h)
            b[i] = (y[i + 1] - y[i]) / h - (2 * c[i] + c[i + 1]) * h / three
        h = x[n - 1] - x[n - 2]
        b[n - 1] = 3 * d[n - 2] * h * h + 2 * c[n - 2] * h + b[n - 2]
    else:
        for i in range(1, n - 1):
            h, hl = x[i + 1] - x[i], x[i] - x[i - 1]
            b[i] = -h / (hl * (hl + h)) * y[i - 1] + (h - hl) / (hl * h) * y[i] + hl / (h * (hl + h)) * y[i + 1]
        b[0] = (-b[1] + 3 * (y[1] - y[0]) / (x[1] - x[0])) / 2
        b[n - 1] = (-b[n - 2] + 3 * (y[n - 1] - y[n - 2]) / (x[n - 1] - x[n - 2])) / 2
        for i in range(n - 1):
            h = x[i + 1] - x[i]
            c[i] = (3 * (y[i + 1] - y[i]) / h - (2 * b[i] + b[i + 1])) / h
            d[i] = ((b[i + 1] - b[i]) / (three * h) - 2 * c[i] / three) / h
    hmin = min(xs[i + 1] - xs[i] for i in range(n - 1))
    return {"x": x, "xs": list(xs), "y": y, "b": b, "c": c, "d": d, "c0": c[0], "n": n, "ymax": max(abs(v) for v in ys), "hmin": hmin}


def spline_eval(A, S, v, s_v, edges=None, tag=""):
    """spline.h:467-499 at v (A's number, scale s_v): (value, scale, branch) with branch in {'left', 'right', 'in'}.
    Scale: the coefficients are bounded by 8 ymax / hmin^k (differences of divided differences of values <= ymax), each enters with
    |h|^k, plus the slope of the spline times the scale of v."""
    n, x = S["n"], S["x"]
    idx = 0
    while idx + 1 < n and x[idx + 1] <= v:
        idx += 1
    if edges is not None:
        for k in range(n):
            _edge(edges, f"spline node {k} {tag}", v - x[k], s_v)
    h = v - x[idx]
    if v < x[0]:
        val, slope, br = (S["c0"] * h + S["b"][0]) * h + S["y"][0], 2 * S["c0"] * h + S["b"][0], "left"
    elif v > x[n - 1]:
        val, slope, br = (S["c"][n - 1] * h + S["b"][n - 1]) * h + S["y"][n - 1], 2 * S["c"][n - 1] * h + S["b"][n - 1], "right"
    else:
        val = ((S["d"][idx] * h + S["c"][idx]) * h + S["b"][idx]) * h + S["y"][idx]
        slope, br = (3 * S["d"][idx] * h + 2 * S["c"][idx]) * h + S["b"][idx], "in"
    r = abs(_f(h)) / S["hmin"]
    return val, 8 * S["ymax"] * (1 + r + r * r + r ** 3) + abs(_f(slope)) * (s_v + abs(_f(v))), br


# ---------------------------------------------------------------------------------------------------------------- (b) the solver

class Pair:
    """One p mode against the g ladder: p(nu) - g(nu) (solver_mm.cpp:143-148, :179-186)."""

    def __init__(self, A, U, ip):
        self.A, self.ip = A, ip
        self.nu_p, self.Dl, self.DPl, self.q = U["nu_p"][ip], U["dnu_loc"][ip], U["DPl"], U["q"]
        self.s_nu_p, self.s_Dl = U["s_nu_p"][ip], U["s_dnu_loc"][ip]
        self.n_alpha = U["ng_min"] + U["ig0"][ip] + U["alpha"]           # n_g + alpha of the g mode used (a double sum of a small integer: exact enough for the scale)
        self.nu_g = nu_g_of(A, U, U["ig0"][ip])
        self.ld = (_to_ld(A, self.nu_p), _to_ld(A, self.Dl))              # the bulk pass sees the definition's nu_p and Dl to extended precision
        self.nu_g_ld = _to_ld(A, self.nu_g)

    def f(self, nu):
        """The definition at one point, as written: X = pi (1/nu - 1/nu_g) 1e6 / DPl."""
        A = self.A
        X = A.pi * (1 / nu - 1 / self.nu_g) * A.lit("1e6") / A.num(self.DPl)
        return (nu - self.nu_p) - self.Dl * A.atan(A.num(self.q) * A.tan(X)) / A.pi

    def f_bulk(self, nu):
        """Extended precision, vectorised (nu: longdouble array)."""
        nu_p, Dl = self.ld
        X = PI_LD * (1 / nu - 1 / self.nu_g_ld) * LD("1e6") / LD(self.DPl)
        return (nu - nu_p) - Dl * np.arctan(LD(self.q) * np.tan(X)) / PI_LD

    def parts(self, nu):
        """float64, vectorised: (g, scale of p - g, derivative of p - g) at nu."""
        nu = np.asarray(nu, dtype=np.float64)
        nu_p, Dl, nu_g = _f(self.nu_p), _f(self.Dl), _f(self.nu_g)
        c = math.pi * 1e6 / self.DPl
        X = c * (1 / nu - 1 / nu_g)
        with np.errstate(all="ignore"):
            T = np.tan(X)
            u = self.q * T
            G = (Dl / math.pi) * self.q * (1 + T * T) / (1 + u * u)
            g = Dl * np.arctan(u) / math.pi
            f = (nu - nu_p) - g
            S = (2 * nu * (1 + G * c / nu ** 2) + G * c * (1 / nu + 4 / nu_g) + 4 * G * np.abs(X) + 2 * (Dl / math.pi) * self.q * np.abs(T) / (1 + u * u)
                 + 3 * np.abs(g) + self.s_nu_p + np.abs(nu - nu_p) + np.abs(f) + self.s_Dl * np.abs(np.arctan(u)) / math.pi)
        return g, S, 1 + G * c / nu ** 2

    def scale(self, nu):
        return self.parts(nu)[1]


def _linspace(A, n, lo, hi):
    step = (hi - lo) / (n - 1)
    return lambda i: hi if i == n - 1 else lo + i * step


def _bulk_grid(n, lo, hi):
    g = lo + np.arange(n, dtype=LD) * ((hi - lo) / LD(n - 1))
    g[-1] = hi
    return g


def _to_ld(A, v):
    return LD(str(v)) if A is Ex else LD(v)


def _changes(a, b):
    return ((b >= 0) & (a < 0)) | ((b > 0) & (a <= 0)) | ((b <= 0) & (a >= 0))


def solve_pair(A, U, ip, edges):
    """solver_mm for p mode ip.  Returns the list of candidates: dicts with cell, alts = [{nl, kind, prop, scale, ratio, accepted, ...}]."""
    if U["ig0"][ip] < 0:
        return []
    P = Pair(A, U, ip)
    resol, fact = A.num(U["resol"]), A.lit(U["fact"])
    Dnu, zone = U["Dnu"], U["zone"]
    numin, numax = P.nu_p - zone * Dnu, P.nu_p + zone * Dnu
    s_lim = P.s_nu_p + _f(zone) * (U["s_Dnu"] + _f(Dnu))
    _edge(edges, f"numin>=0[{ip}]", numin, s_lim + abs(_f(numin)))
    lo = numin if numin >= 0 else A.num(0)
    qn = (numax - lo) / resol
    _edge(edges, f"n[{ip}]", _int_dist(A, qn), (2 * s_lim + 2 * abs(_f(numax)) + 2 * abs(_f(lo))) / U["resol"] + abs(_f(qn)))
    n = A.trunc(qn)
    if n < 2:
        return []
    grid = _linspace(A, n, lo, numax)
    gl = _bulk_grid(n, _to_ld(A, lo), _to_ld(A, numax))
    start = 1 if lo == 0 else 0                                            # nu = 0: 1/nu is infinite, tan(inf) is NaN and a NaN never "changes sign"
    fb = np.full(n, np.nan, dtype=LD)
    with np.errstate(all="ignore"):
        fb[start:] = P.f_bulk(gl[start:])
        sb = np.full(n, np.inf)
        sb[start:] = P.scale(gl[start:].astype(np.float64))
    m = np.abs(fb[start:].astype(np.float64)) / sb[start:]
    k = int(np.argmin(m))
    _edge(edges, f"grid sign[{ip}]@{k + start}", float(fb[k + start]), float(sb[k + start]))
    cells = np.nonzero(_changes(fb[:-1], fb[1:]))[0]
    out = []
    for cell in (int(v) for v in cells):
        x0 = grid(cell)
        if A is Ex:        # both ends of the cell at 50 digits
            fa, fz = P.f(x0), P.f(grid(cell + 1))
            assert bool(_changes(np.float64(_f(fa)), np.float64(_f(fz)))) or abs(_f(fa)) < 1e-25 or abs(_f(fz)) < 1e-25, (ip, cell)
        rmin, rmax = x0 - 2 * resol, x0 + 2 * resol
        nl_exact = (rmax - rmin) / (resol * fact)
        nl_hi = int(round(_f(nl_exact)))                                   # 4 / factor: an integer; a double evaluation gives it or one less
        cand = {"ip": ip, "cell": cell, "x0": x0, "alts": []}
        for nl in (nl_hi, nl_hi - 1):
            cand["alts"].append(_refine(A, U, P, rmin, rmax, nl, edges))
        out.append(cand)
    return out


def _refine(A, U, P, rmin, rmax, nl, edges):
    """The local grid of nl points over [rmin, rmax], lin_interpol(p - g, nu, 0) and the ratio test (solver_mm.cpp:377-431)."""
    ip = P.ip
    lg = _linspace(A, nl, rmin, rmax)
    gl = _bulk_grid(nl, _to_ld(A, rmin), _to_ld(A, rmax))
    with np.errstate(all="ignore"):
        fb = P.f_bulk(gl)
        sb = P.scale(gl.astype(np.float64))
    ff = fb.astype(np.float64)

    def val(j):
        return P.f(lg(j)) if A is Ex else fb[j]
    f_first, f_last = val(0), val(nl - 1)
    tag = f"[{ip}]@{_f(rmin):.4f}/{nl}"
    _edge(edges, "f_first" + tag, f_first, sb[0])
    _edge(edges, "f_last" + tag, f_last, sb[-1])
    alt = {"nl": nl, "rmin": rmin, "rmax": rmax}
    if f_first <= 0 <= f_last:
        hit = np.nonzero(~((0.0 < ff[:-1]) | (0.0 > ff[1:])))[0]           # the loop condition of lin_interpol, negated: the FIRST such pair
        j = int(hit[0])
        # every local point up to the pair decides whether the scan stops earlier
        mm = np.abs(ff[:j + 2]) / sb[:j + 2]
        kk = int(np.argmin(mm))
        _edge(edges, "local sign" + tag + f"#{kk}", ff[kk], sb[kk])
        kind = "interp"
    elif 0 > f_last:
        j, kind = nl - 2, "above"     # interpol.cpp:38-48: three `if`s in a row, not else-if -- with a pole inside (f_first > 0 > f_last) both
    else:                             # extrapolations apply and the LAST one, towards the upper edge, is the one returned
        j, kind = 0, "below"
    xa, xb, fa, fz = lg(j), lg(j + 1), val(j), val(j + 1)
    a = (xb - xa) / (fz - fa)
    prop = xa - a * fa                                                     # a*0 + b with b = y[i] - a x[i]
    slope = abs(_f((fz - fa) / (xb - xa)))
    df = abs(_f(fz - fa))
    s_prop = (abs(_f(fz)) * sb[j] + abs(_f(fa)) * sb[j + 1]) / (df * slope) + 3 * abs(_f(prop))
    # the ratio test: g(prop) / p(prop) = 1 - f(prop) / p(prop)
    pp = prop - P.nu_p
    X = A.pi * (1 / prop - 1 / P.nu_g) * A.lit("1e6") / A.num(P.DPl)
    gp = P.Dl * A.atan(A.num(P.q) * A.tan(X)) / A.pi
    ratio = gp / pp
    with np.errstate(all="ignore"):
        _, s_f, fprime = P.parts(_f(prop))
    s_ratio = (float(s_f) + float(fprime) * s_prop) / abs(_f(pp)) + 3 * abs(_f(ratio))
    _edge(edges, "ratio>=0.999" + tag, ratio - A.lit("0.999"), s_ratio)
    _edge(edges, "ratio<=1.001" + tag, ratio - A.lit("1.001"), s_ratio)
    accepted = A.lit("0.999") <= ratio <= A.lit("1.001")
    alt.update(kind=kind, j=j, prop=prop, scale=float(s_prop), ratio=ratio, ratio_scale=s_ratio, accepted=bool(accepted), xa=xa, xb=xb, fa=fa, fb=fz,
               slope=slope)
    if accepted:
        for nm, lim, s_lim in (("keep_lo", U["keep_lo"], U["s_keep_lo"]), ("keep_hi", U["keep_hi"], U["s_keep_hi"])):
            _edge(edges, nm + tag, prop - lim, s_prop + s_lim)
        alt["kept"] = bool(U["keep_lo"] <= prop <= U["keep_hi"])
    else:
        alt["kept"] = False
    return alt


def solve(A, model_id, params, plength, x):
    """Stages (a) and (b): the unpack and every p mode's candidates, then sort and tolerance-unique on the first alternative (the margins
    of the unique say whether the second could change it)."""
    grid = x if isinstance(x, RGrid) else RGrid(x)
    U = unpack(A, model_id, params, plength, grid.step)
    sol = {"U": U, "status": U["status"], "grid": grid, "edges": U["edges"], "cands": [], "roots": [], "A": A, "model_id": model_id}
    if U["status"] != OK or U["no_modes"]:
        return sol
    E = sol["edges"]
    for ip in range(U["Lp"]):
        sol["cands"] += solve_pair(A, U, ip, E)
    kept = [c for c in sol["cands"] if c["alts"][0]["kept"]]
    for c in sol["cands"]:
        k0, k1 = c["alts"][0], c["alts"][1]
        c["same_fate"] = (k0["kept"] == k1["kept"])
        if not c["same_fate"]:
            _edge(E, f"fate of the two local grids differs@{_f(c['x0']):.4f}", 0.0, 1.0)
    kept.sort(key=lambda c: c["alts"][0]["prop"])
    tol = 2 * A.num(U["resol"])
    roots, runs, run = [], [], []
    for c in kept:
        v, s = c["alts"][0]["prop"], c["alts"][0]["scale"]
        spread = abs(_f(c["alts"][0]["prop"] - c["alts"][1]["prop"])) if c["alts"][1]["kept"] else 0.0
        if roots:
            last = roots[-1]
            d = abs(last["alts"][0]["prop"] - v)
            _edge(E, f"unique@{_f(v):.4f}", _f(d - tol) if d != 0 else INF, s + last["alts"][0]["scale"] + (spread + last["spread"]) / EPS)
            if d <= tol:
                last["dropped"].append(c)
                continue
        c["dropped"], c["spread"] = [], spread
        roots.append(c)
    sol["roots"], sol["sorted"] = roots, kept
    sol["n_raw"] = len(kept)
    return sol


def unique_runs(sol):
    """Runs of the sorted raw roots chained within tol (each within tol of its left neighbour), duplicates of one root (distance below 1e-9)
    merged first.  Returns a list of runs, each a list of (value, kept?)."""
    U, A = sol["U"], sol["A"]
    tol = 2 * U["resol"]
    vals, keptset = [], {id(c) for c in sol["roots"]}
    for c in sol["sorted"]:
        v = _f(c["alts"][0]["prop"])
        if vals and abs(vals[-1][0] - v) < 1e-9:
            continue
        vals.append((v, id(c) in keptset))
    runs, cur = [], []
    for v in vals:
        if cur and abs(cur[-1][0] - v[0]) <= tol:
            cur.append(v)
        else:
            if cur:
                runs.append(cur)
            cur = [v]
    if cur:
        runs.append(cur)
    return runs


# ---------------------------------------------------------------------------------------------------------------- (d) zeta

def _zeta_term(A, U, nu, ip, n_alpha=None):
    """ksi_fct1 for p mode ip and the g mode of index sum n_alpha (None: as an angle reduced by the identity)."""
    DPl, q = A.num(U["DPl"]), A.num(U["q"])
    if n_alpha is None:
        up = A.pi * (A.lit("1e6") / (nu * DPl) - (U["ng_min"] + A.num(U["alpha"])))
    else:
        up = A.pi * A.lit("1e6") * (1 / nu - 1 / (A.lit("1e6") / (n_alpha * DPl))) / DPl
    down = A.pi * (nu - U["nu_p"][ip]) / U["dnup"][ip]
    front = A.lit("1e-6") * nu * nu * DPl / (q * U["dnup"][ip])
    cu, cd = A.cos(up), A.cos(down)
    return 1 / (1 + front * (cu * cu) / (cd * cd))


def zeta_sum(A, U, nu, literal=False):
    """The un-normalised sum over all (p, g) pairs at nu (bump_DP.cpp:138-150)."""
    s = A.num(0)
    for ip in range(U["Lp"]):
        if literal:
            loc = A.num(0)
            for ig in range(U["Lg"]):
                loc = loc + _zeta_term(A, U, nu, ip, U["ng_min"] + ig + A.num(U["alpha"]))
            s = s + loc
        else:
            s = s + U["Lg"] * _zeta_term(A, U, nu, ip)
    return s


def _zeta_bulk(U, nu, with_scale=False, s_nu=0.0):
    """Extended precision, vectorised over nu; with_scale: also the float64 scale of the sum at nu (s_nu: the scale of nu itself)."""
    A = U["_A"]
    nu = np.asarray(nu, dtype=LD)
    DPl, q, Lg = LD(U["DPl"]), LD(U["q"]), U["Lg"]
    na = LD(U["ng_min"]) + LD(U["alpha"])
    up = PI_LD * (LD("1e6") / (nu * DPl) - na)
    cu2 = np.cos(up) ** 2
    tot = np.zeros(nu.shape, dtype=LD)
    sc = np.zeros(nu.shape, dtype=np.float64)
    nuf = nu.astype(np.float64)
    c1 = math.pi * 1e6 / U["DPl"]
    nu_g_mid = 1e6 / ((U["ng_min"] + U["Lg"] / 2 + U["alpha"]) * U["DPl"])
    for ip in range(U["Lp"]):
        nu_p, dn = _to_ld(A, U["nu_p"][ip]), _to_ld(A, U["dnup"][ip])
        down = PI_LD * (nu - nu_p) / dn
        cd2 = np.cos(down) ** 2
        F = LD("1e-6") * nu * nu * DPl / (q * dn)
        D = cd2 + F * cu2
        T = cd2 / D
        tot = tot + Lg * T
        if with_scale:
            Tf, Ff = T.astype(np.float64), F.astype(np.float64)
            cu2f, cd2f, Df = cu2.astype(np.float64), cd2.astype(np.float64), D.astype(np.float64)
            su_cu = np.abs(np.sin(2 * up.astype(np.float64))) / 2            # |cos sin|
            sd_cd = np.abs(np.sin(2 * down.astype(np.float64))) / 2
            dT_dup = 2 * cd2f * Ff * su_cu / Df ** 2
            dT_ddown = 2 * sd_cd * Ff * cu2f / Df ** 2
            dnf, s_dn = float(dn), U["s_dnup"][ip]
            upf, downf = np.abs(up.astype(np.float64)), np.abs(down.astype(np.float64))
            s_up = c1 * (2 / nuf + 4 / nu_g_mid) + 4 * (upf + math.pi * U["Lg"]) + c1 / nuf ** 2 * s_nu
            s_down = math.pi * (s_nu + nuf + U["s_nu_p"][ip] + np.abs(nuf - float(nu_p))) / dnf + downf * (3 + s_dn / dnf)
            s_F = Ff * (5 + s_dn / dnf + 2 * s_nu / nuf)
            one_T = Tf * (1 - Tf)
            sc = sc + Lg * (dT_dup * s_up + dT_ddown * s_down + one_T / np.maximum(Ff, 1e-300) * s_F + 4 * one_T + 4 * Tf) + np.abs(tot.astype(np.float64))
    return (tot, sc) if with_scale else tot


def zeta_norm(A, U):
    """The maximum of the sum over the 4-year grid between the lowest and the highest of the p and g ladders (bump_DP.cpp:130-168):
    (norm, scale).  The bulk pass ranks the grid; the top points are evaluated in the definition's arithmetic."""
    U["_A"] = A
    if "_norm" in U:
        return U["_norm"]
    g_hi, g_lo = nu_g_of(A, U, 0), nu_g_of(A, U, U["Lg"] - 1)
    p_lo, p_hi = min(U["nu_p"]), max(U["nu_p"])
    lo = g_lo if p_lo >= g_lo else p_lo
    hi = p_hi if p_hi >= g_hi else g_hi
    resol = A.lit("1e6") / (4 * A.num(365) * A.num(86400))
    qn = (hi - lo) / resol
    n = A.trunc(qn)
    _edge(U["edges"], "zeta grid n", _int_dist(A, qn), 8 * (abs(_f(hi)) + abs(_f(lo))) / _f(resol))
    if n < 2:
        return A.num(0), 0.0
    gl = _bulk_grid(n, _to_ld(A, lo), _to_ld(A, hi))
    tot = _zeta_bulk(U, gl)
    top = np.argsort(tot)[-4:]
    grid = _linspace(A, n, lo, hi)
    best, at = None, None
    for i in (int(v) for v in top):
        v = zeta_sum(A, U, grid(i)) if A is Ex else tot[i]
        if best is None or v > best:
            best, at = v, i
    _, sc = _zeta_bulk(U, gl[at:at + 1], with_scale=True, s_nu=3 * float(gl[at]))
    U["_norm"] = (best, float(sc[0]))
    return U["_norm"]


# ---------------------------------------------------------------------------------------------------------------- (c)-(e) modes and rows

def _interp(A, xs, ys, s_ys, xi, s_xi, edges=None, tag=""):
    """interpol.cpp:13-43 (tamcmc/sources) with computed ordinates: xs, ys in A's numbers, s_ys their scales, xi with scale s_xi."""
    n = len(xs)
    if xi < xs[0]:
        k = 0
    elif xi > xs[n - 1]:
        k = n - 2
    else:
        k = 0
        while k < n - 2 and (xi < xs[k] or xi > xs[k + 1]):
            k += 1
    if edges is not None:
        for j in range(n):
            _edge(edges, f"segment {tag} node {j}", xi - xs[j], s_xi + 2 * abs(_f(xs[j])))
    x0, x1, y0, y1 = xs[k], xs[k + 1], ys[k], ys[k + 1]
    a = (y1 - y0) / (x1 - x0)
    b = y0 - a * x0
    dx = abs(_f(x1 - x0))
    sa = (abs(_f(y1)) + abs(_f(y0)) + s_ys[k] + s_ys[k + 1]) / dx + abs(_f(a))
    val = a * xi + b
    scale = sa * abs(_f(xi)) + abs(_f(y0)) + s_ys[k] + sa * abs(_f(x0)) + abs(_f(a)) * s_xi + abs(_f(val))
    return val, scale


def finish(sol, choice=None):
    """Stages (c), (d), (e) at the chosen alternatives (choice[i] in {0, 1} per root; None: all 0).  Returns a dict: status, modes, rows,
    noise, nharvey, nnoise, edges (the decisions taken here)."""
    A, U, grid = sol["A"], sol["U"], sol["grid"]
    with localcontext(Context(prec=PREC)):
        return _finish(A, U, grid, sol, choice)


def _finish(A, U, grid, sol, choice):
    out = {"status": sol["status"], "modes": [], "rows": [], "edges": [], "noise": [], "nharvey": 0, "nnoise": 1}
    if sol["status"] != OK:
        return out
    E = out["edges"]
    L = U["L"]
    out.update(noise=U["noise"], nharvey=U["nharvey"], nnoise=U["nnoise"])
    roots = sol["roots"]
    if len(roots) > CAP1:
        out["status"] = ERR_BAD_ARG
        return out
    choice = choice if choice is not None else [0] * len(roots)
    modes = []
    if roots:
        norm, s_norm = zeta_norm(A, U)
        out["zeta_norm"], out["zeta_norm_scale"] = norm, s_norm
    Hf, Wf = A.num(U["Hfactor"]), A.num(U["Wfactor"])
    fmin, fmax = A.num(U["fmin"]), A.num(U["fmax"])
    six, eight, twelve, fourteen = (A.lit(t) for t in ("0.6", "0.8", "1.2", "1.4"))
    fi = [fmin * six, fmin * eight] + [A.num(v) for v in U["fl0"]] + [fmax * twelve, fmax * fourteen]
    hi = [A.num(0), U["H0"][0] / 4] + list(U["H0"]) + [U["H0"][-1] / 4, A.num(0)]
    s_hi = [0.0, U["H0s"][0] / 4] + list(U["H0s"]) + [U["H0s"][-1] / 4, 0.0]
    fl0A = [A.num(v) for v in U["fl0"]]
    for i, c in enumerate(roots):
        alt = c["alts"][choice[i]]
        v, s_v = alt["prop"], alt["scale"]
        m = {"root": v, "root_scale": s_v, "ip": c["ip"], "alt": choice[i], "branch": None}
        if U["spline"] is not None:
            bias, s_b, br = spline_eval(A, U["spline"], v, s_v, E, f"mode {i}")
            f1, s_f1 = v + bias, s_v + s_b + abs(_f(v + bias))
            m["branch"] = br
        else:
            f1, s_f1 = v, s_v
        m.update(nu=f1, nu_scale=s_f1)
        # zeta
        raw = zeta_sum(A, U, f1) if A is Ex else _zeta_bulk(U, np.array([f1], dtype=LD))[0]
        _, s_raw = _zeta_bulk(U, np.array([_to_ld(A, f1)], dtype=LD), with_scale=True, s_nu=s_f1)
        z = raw / norm
        s_z = float(s_raw[0]) / _f(norm) + abs(_f(z)) * (s_norm / _f(norm) + 1)
        _edge(E, f"z>1 mode {i}", z - 1, s_z)
        m["clipped"] = bool(z > 1)
        if z > 1:
            z, s_z = A.num(1), 0.0
        m.update(zeta=z, zeta_scale=s_z)
        arg = 1 - Hf * z
        s_arg = U["Hfactor"] * (s_z + abs(_f(z))) + abs(_f(arg))
        hr = A.sqrt(arg)
        hrf = _f(hr)
        _edge(E, f"|hr|<1e-5 mode {i}", arg - A.lit("1e-10"), s_arg)       # hr < 1e-5  <=>  1 - Hf z < 1e-10
        m["lifted"] = bool(hr < A.lit("1e-5"))
        if m["lifted"]:
            hr, s_hr = A.lit("1e-10"), 1e-10        # (the constant itself: a double holds 1e-10 to half an ulp)
        else:
            s_hr = s_arg / (2 * hrf) + hrf
        m.update(hr=hr, hr_scale=s_hr)
        t, s_t = _interp(A, fi, hi, s_hi, f1, s_f1, E, f"H mode {i}")
        _edge(E, f"t<0 mode {i}", t if U["do_amp"] or any(_f(h) != 0 for h in U["H0"]) else INF, s_t)
        Hp, s_Hp = (A.num(0), 0.0) if t < 0 else (abs(t), s_t)
        Vl1 = U["Vl"][1]
        H = abs(hr * (Hp * A.num(Vl1)))
        s_H = (_f(hr) * (s_Hp + 2 * _f(Hp)) + s_hr * _f(Hp)) * Vl1
        w0, s_w0 = _interp(A, fl0A, U["W0"], U["W0s"], f1, s_f1, E, f"W mode {i}")
        wz = 1 - Wf * z
        W = w0 * wz / A.sqrt(hr)
        s_W = abs(_f(W)) * (s_w0 / abs(_f(w0)) + (U["Wfactor"] * (s_z + abs(_f(z))) + abs(_f(wz))) / max(abs(_f(wz)), 1e-300)
                            + (s_hr / _f(hr)) / 2 + 3) if _f(w0) != 0 else s_w0
        rc, re = A.num(U["rot_core"]), A.num(U["rot_env"])
        a1 = abs(z * (rc / 2 - re) + re)
        s_a1 = (s_z + 2 * abs(_f(z))) * abs(_f(rc / 2 - re)) + U["rot_env"] + _f(a1)
        m.update(H=H, H_scale=s_H, W=W, W_scale=s_W, a1=a1, a1_scale=s_a1)
        modes.append(m)
    out["modes"] = modes
    # rows in the model's accumulation order: l=0, the mixed modes, l=2, l=3 (models.cpp:4931-5006)
    tc = A.num(U["trunc_c"])
    eta0 = U["eta0"]
    micro = A.lit("1e-6")

    def row(l, fc, s_fc, Wd, s_W, H, s_H, a, s_a1, e0):
        fs = a[1]
        st, i0, i1, edges = tr._window(A, grid, l, fc, Wd, s_W, fs, s_a1, tc)
        # (a computed centre: its scale enters the clip tests as it is and the edge quotients divided by the step)
        edges = [(nm, d, sc + (s_fc / abs(grid.step) if nm in ("i0", "i1") else s_fc)) for nm, d, sc in edges]
        r = {"l": l, "fc": fc, "fc_scale": s_fc, "gamma": Wd, "gamma_scale": s_W, "asym": U["asym"], "i0": i0, "i1": i1, "edges": edges, "flags": 0,
             "status": st, "nu": [A.num(0)] * 7, "hv": [A.num(0)] * 7, "nu_scale": [0.0] * 7, "hv_scale": [0.0] * 7}
        for k in range(2 * l + 1):
            mm = k - l
            if l == 0:
                r["nu"][k], r["nu_scale"][k] = fc, s_fc
            else:
                terms = [a[j] * A.frac(tr.pslm(j, l, mm)) for j in range(1, 7)]
                eta = fc * e0 * A.frac(tr.qlm(l, mm)) * (a[1] * micro) ** 2 if e0 > 0 else A.num(0)
                r["nu"][k] = fc + sum(terms, A.num(0)) + eta
                r["nu_scale"][k] = s_fc + abs(_f(fc)) + 4 * abs(_f(eta)) + sum(abs(_f(t)) for t in terms) * 2 + abs(mm) * s_a1 + abs(_f(r["nu"][k]))
            r["hv"][k] = H * U["V"][l][k]
            r["hv_scale"][k] = (s_H + _f(H)) * U["Vs"][l][k] + _f(r["hv"][k])
        return r
    zero_a = [A.num(0)] * 7
    rows = []
    for n in range(L.Nfl0):
        rows.append(row(0, A.num(U["fl0"][n]), 0.0, U["W0"][n], U["W0s"][n], U["H0"][n], U["H0s"][n], zero_a, 0.0, A.num(0)))
    for m in modes:
        a = [A.num(0), m["a1"]] + [A.num(0)] * 5
        rows.append(row(1, m["nu"], m["nu_scale"], m["W"], m["W_scale"], m["H"], m["H_scale"], a, m["a1_scale"], eta0))
    for l, lst in ((2, U["fl2"]), (3, U["fl3"])):
        for f in lst:
            W, s_W = (A.num(U["g"][0]), 0.0) if U["cte"] else width_law(A, U["g"], f)
            h, s_h = tr._interpol(A, U["fl0"], [_f(v) for v in U["H0"]], f) if not U["do_amp"] else _interp(A, fl0A, U["H0"], U["H0s"], A.num(f), 0.0)
            Vl = A.num(U["Vl"][l])
            if U["do_amp"]:
                H = abs(h / (A.pi * W) * Vl)
                s_H = _f(H) * (s_h / max(abs(_f(h)), 1e-300) + s_W / _f(W) + 4)
            else:
                H, s_H = abs(h * Vl), s_h * U["Vl"][l] + _f(abs(h * Vl))
            a = [A.num(0), A.num(U["rot_env"])] + [A.num(v) for v in U["a"][2:5]] + ([A.num(v) for v in U["a"][5:7]] if l == 3 else [A.num(0)] * 2)
            rows.append(row(l, A.num(f), 0.0, W, s_W, H, s_H, a, 0.0, eta0))
    bad = [r["status"] for r in rows if r["status"] != OK]
    if bad:
        out["status"] = bad[-1]
    out["rows"] = rows
    return out


def build(model_id, params, plength, x, twin=False):
    """solve() in the definition's arithmetic (twin: the longdouble twin)."""
    if twin:
        with np.errstate(all="ignore"):
            return solve(Tw, model_id, params, plength, x)
    with localcontext(Context(prec=PREC)):
        return solve(Ex, model_id, params, plength, x)


def finish_twin(sol, choice=None):
    with np.errstate(all="ignore"):
        return _finish(Tw, sol["U"], sol["grid"], sol, choice)


def knife_edges(edges, K):
    return [(name, dist, scale) for name, dist, scale in edges if dist <= K * EPS * scale]


# ---------------------------------------------------------------------------------------------------------------- definition-level layer

def true_roots(sol, ip):
    """The zeros of p - g for p mode ip inside its zone, each found between two consecutive poles of tan X (where p - g is continuous and
    increasing: at most one zero), located in extended precision by bisection and polished at 50 digits by Newton steps.  Returns
    (roots [Decimal], poles [float])."""
    U = sol["U"]
    with localcontext(Context(prec=PREC)):
        P = Pair(Ex, U, ip)
        zone, Dnu = U["zone"], U["Dnu"]
        lo, hi = _f(P.nu_p - zone * Dnu), _f(P.nu_p + zone * Dnu)
        lo, hi = max(lo, _f(U["keep_lo"]) - 1.0, 1e-3), min(hi, _f(U["keep_hi"]) + 1.0)     # (zeros outside the keep range are of no interest)
        na = U["ng_min"] + U["ig0"][ip] + U["alpha"]
        ks = 1e6 / U["DPl"]
        k_hi, k_lo = math.floor(ks / lo - na - 0.5) + 1, math.ceil(ks / hi - na - 0.5) - 1
        poles = sorted(ks / (k + na + 0.5) for k in range(k_lo, k_hi + 1) if k + na + 0.5 > 0)
        bounds = [lo] + [v for v in poles if lo < v < hi] + [hi]
        roots = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            w = b - a
            xa, xb = LD(a) + LD(w) * LD(1e-9), LD(b) - LD(w) * LD(1e-9)
            fa, fb = P.f_bulk(np.array([xa, xb], dtype=LD))
            if not (fa < 0 < fb):
                continue
            for _ in range(80):
                xm = (xa + xb) / 2
                if P.f_bulk(np.array([xm], dtype=LD))[0] < 0:
                    xa = xm
                else:
                    xb = xm
            r = Decimal(str(xa))
            c = PI * Decimal("1e6") / Decimal(U["DPl"])
            for _ in range(3):
                X = PI * (1 / r - 1 / P.nu_g) * Decimal("1e6") / Decimal(P.DPl)
                T = Ex.tan(X)
                u = Decimal(P.q) * T
                fp = 1 + (P.Dl / PI) * Decimal(P.q) * (1 + T * T) / (1 + u * u) * c / (r * r)
                r = r - P.f(r) / fp
            roots.append(r)
        return roots, poles

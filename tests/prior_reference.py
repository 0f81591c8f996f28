"""Exact restatement of the reference's log-priors, for the parity tests of the host (long double) and device (double) code.

Written from the reference's own text -- the primitives of tamcmc/sources/stats_dictionary.cpp:38-250, apply_generic_priors and the five
prior functions of tamcmc/sources/priors_calc.cpp (classes 0 Kallinger2014_Gaussian, 1 Harvey_Gaussian, 2 MS_Global, 3 local,
4 asymptotic), the replicated-edge second difference of derivatives_handler.cpp:400-426 and linfit.cpp -- and from nothing else: it
shares no line with csrc/priors_impl.h or oracle/tamcmc_oracle.c, which is its worth.  Standard library only.

Arithmetic.  Every long-double expression of the reference is evaluated with `decimal` at 50 significant digits (Decimal.ln(), .sqrt(),
**; pi as a 50-digit literal), every input converted exactly with Decimal(float).  What the reference itself holds in a `double` is formed
in double here too, in the reference's order of operations: the a_j / a1 of the aj family and their ratio, the ratio sums of
impose_normHnlm = 1, a3 / a1 of the local and asymptotic classes, `params[i] < 0`, the slope Dnu of the l = 0 frequencies (linfit, sums
taken left to right), d02 = f(l=0) - f(l=2), Dnu / 3, 0.015 Dnu and the second differences.  Only the Stello width bound of classes 0
and 1 is a long-double comparison in the reference (priors_calc.cpp:636-639, :654-658, :683) and is taken in Decimal.

The same formulas run a second time in plain float64 (math.log / math.sqrt, sums left to right): `log_prior(..., exact=False)`.  The
distance between the two measures what double arithmetic costs on a given vector, independently of the code under test.

log_prior() returns a Result:
    value    Decimal (float with exact=False), or float('-inf')
    failed   None, or the name of the first constraint / term that gave -inf, in the reference's order of evaluation
    terms    the additive terms in the reference's order of summation (those evaluated before a hard constraint ended the function)
    scale    sum over the terms of max(1, |term|) (finite terms only)
    margins  [(name, quantity, threshold)] of every hard constraint decided by a COMPUTED quantity (a ratio, a ratio sum, the width
             bound), whether it passed or not: near_threshold() gives the smallest relative distance
Prior ids and options at which the reference itself stops (ids 3, 9, 11, 12; impose_normHnlm = 2; the families flagged "needs checks")
raise Unsupported.
"""
import math
from decimal import Decimal, localcontext

PREC = 50
PI50 = Decimal("3.1415926535897932384626433832795028841971693993751")
NEG_INF = float("-inf")


class Unsupported(Exception):
    """The reference exits here (or this restatement does not cover the branch)."""


class _Exact:
    pi = PI50
    half = Decimal("0.5")
    ninf = Decimal("-Infinity")

    @staticmethod
    def num(x):
        return Decimal(float(x))

    @staticmethod
    def fabs(v):  # (abs() would round its result to the context's 50 digits: a double can carry more, and a comparison must see them all)
        return v.copy_abs()

    @staticmethod
    def ln(v):
        return v.ln()

    @staticmethod
    def sqrt(v):
        return v.sqrt()


class _Double:
    pi = math.pi
    half = 0.5
    ninf = NEG_INF

    @staticmethod
    def num(x):
        return float(x)

    @staticmethod
    def fabs(v):
        return abs(v)

    @staticmethod
    def ln(v):
        return math.log(v)

    @staticmethod
    def sqrt(v):
        return math.sqrt(v)


# ---- primitives: stats_dictionary.cpp:38-250 (A = arithmetic; every argument already A.num()) ----
def logP_uniform(A, b_min, b_max, x):
    if x <= b_max and x >= b_min:
        return -A.ln(abs(b_max - b_min))
    return A.ninf


def logP_uniform_abs(A, b_min, b_max, x):
    if A.fabs(x) <= b_max and A.fabs(x) >= b_min:
        return -A.ln(abs(b_max - b_min))
    return A.ninf


def logP_gaussian(A, mean, sigma, x):
    return -A.ln(A.sqrt(2 * A.pi) * sigma) - A.half * ((x - mean) / sigma) ** 2


def logP_jeffrey(A, hmin, hmax, h):
    if h < hmax and h > 0:
        prior = 1 / (h + hmin)
        norm = A.ln((hmax + hmin) / hmin)
        return A.ln(prior / norm)
    return A.ninf


def logP_jeffrey_abs(A, hmin, hmax, h):
    if A.fabs(h) < hmax:
        prior = 1 / (A.fabs(h) + hmin)
        norm = A.ln((hmax + hmin) / hmin)
        return A.ln(prior / norm)
    return A.ninf


def logP_uniform_gaussian(A, b_min, b_max, sigma, x):
    logP = 0
    if x < b_min:
        logP = A.ninf
    if x <= b_max and x >= b_min:
        logP = 0
    if x > b_max:
        logP = -A.half * ((x - b_max) / sigma) ** 2
    C = A.ln(abs(b_max - b_min) + A.half * A.sqrt(2 * A.pi) * sigma)
    return logP - C


def logP_gaussian_uniform(A, b_min, b_max, sigma, x):
    logP = 0
    if x > b_max:
        logP = A.ninf
    if x <= b_max and x >= b_min:
        logP = 0
    if x < b_min:
        logP = -A.half * ((x - b_min) / sigma) ** 2
    C = A.ln(abs(b_max - b_min) + A.half * A.sqrt(2 * A.pi) * sigma)
    return logP - C


def logP_gaussian_uniform_gaussian(A, b_min, b_max, sigma1, sigma2, x):
    logP = 0
    if x < b_min:
        logP = -A.half * ((x - b_min) / sigma1) ** 2
    if x <= b_max and x >= b_min:
        logP = 0
    if x > b_max:
        logP = -A.half * ((x - b_max) / sigma2) ** 2
    C = A.ln(abs(b_max - b_min) + A.half * A.sqrt(2 * A.pi) * (sigma1 + sigma2))
    return logP - C


class Result:
    def __init__(self, A):
        self.A = A
        self.terms = []
        self.names = []
        self.failed = None
        self.margins = []

    def add(self, name, t):
        self.terms.append(t)
        self.names.append(name)
        if self.failed is None and t == self.A.ninf:
            self.failed = name

    def reject(self, name):
        if self.failed is None:
            self.failed = name
        self.rejected = True
        return self

    rejected = False

    def _value(self):
        if self.failed is not None:
            return NEG_INF
        f = 0
        for t in self.terms:  # left to right, as f = f + ... / pena = pena + ... in the reference
            f = f + t
        return f

    def _scale(self):
        s = 0
        for t in self.terms:
            if t != self.A.ninf:
                s = s + max(1, abs(t))
        return s

    def near_threshold(self):
        """Smallest relative distance of a computed deciding quantity from its threshold (1.0 when there is none).  A threshold of 0 is
        measured against 1, the width of the interval it bounds; a quantity that is exactly 0 there came from stored zeros."""
        d = 1.0
        for _, q, thr in self.margins:
            q, thr = Decimal(q) if not isinstance(q, Decimal) else q, Decimal(thr) if not isinstance(thr, Decimal) else thr
            if thr == 0:
                if q == 0:
                    continue
                d = min(d, float(abs(q)))
            else:
                d = min(d, float(abs(q / thr - 1)))
        return d


# ---- apply_generic_priors: priors_calc.cpp:725-870 ----
def _generic(A, R, params, priors, sw):
    n = len(params)
    for i in range(n):
        k = int(sw[i])
        if k == 0 or k == 13:
            continue
        x = A.num(params[i])
        p = [A.num(priors[r][i]) for r in range(4)]
        nm = "id %d on parameter %d" % (k, i)
        if k == 1:
            R.add(nm, logP_uniform(A, p[0], p[1], x))
        elif k == 2:
            R.add(nm, logP_gaussian(A, p[0], p[1], x))
        elif k == 4:
            R.add(nm, logP_jeffrey(A, p[0], p[1], x))
        elif k == 5:
            R.add(nm, logP_uniform_gaussian(A, p[0], p[1], p[2], x))
        elif k == 6:
            R.add(nm, logP_gaussian_uniform(A, p[0], p[1], p[2], x))
        elif k == 7:
            R.add(nm, logP_gaussian_uniform_gaussian(A, p[0], p[1], p[2], p[3], x))
        elif k == 8:
            R.add(nm, logP_uniform_abs(A, p[0], p[1], x))
        elif k == 10:
            R.add(nm, logP_jeffrey_abs(A, p[0], p[1], x))
        else:
            raise Unsupported("prior id %d" % k)


def second_differences(y):
    """Scndder_adaptive_reggrid(y), in double: forward at the first point, backward at the last, centred in between -- all three are
    y[i+2] - 2 y[i+1] + y[i] on their three points."""
    n = len(y)
    if n < 3:
        raise Unsupported("second difference of fewer than three points")
    mid = [float(y[i + 2]) - 2. * float(y[i + 1]) + float(y[i]) for i in range(n - 2)]
    return [mid[0]] + mid + [mid[-1]]


def linfit_slope(y):
    """linfit(0 .. n-1, y)[0] in double (linfit.cpp), sums left to right."""
    n = len(y)
    sx = 0.0
    for i in range(n):
        sx = sx + float(i)
    mean_x = sx / float(n)
    t = [float(i) - mean_x for i in range(n)]
    sty, stt = 0.0, 0.0
    for i in range(n):
        sty = sty + t[i] * float(y[i])
    for i in range(n):
        stt = stt + t[i] * t[i]
    return sty / stt


def _noise_checks(R, params, sw, on, i_sw3):
    """The three positivity checks both MS_Global (:251-274) and asymptotic (:377-396) make on the noise block."""
    if sw[on + 3] != 0 and (params[on + 3] < 0 or params[on + 4] < 0 or params[on + 5] < 0):
        return "noise check 1 (second Harvey profile)"
    if sw[on + 6] != 0 and (params[on + 6] < 0 or params[on + 7] < 0 or params[on + 8] < 0):
        return "noise check 2 (third Harvey profile)"
    if sw[i_sw3] != 0 and params[on + 9] < 0:
        return "noise check 3 (white noise)"
    return None


def _ms_global(A, R, params, pl, priors, sw, extra):
    smooth_switch, scoef = int(extra[0]), float(extra[1])
    limit = [float(extra[2 + j]) for j in range(6)]
    impose_normHnlm, model_index = int(extra[8]), int(extra[9])
    Nmax, lmax = int(pl[0]), int(pl[1])
    Nfl = [int(pl[2]), int(pl[3]), int(pl[4]), int(pl[5])]
    Nsplit, Nwidth, Nnoise = int(pl[6]), int(pl[7]), int(pl[8])
    Nf = sum(Nfl)
    for i in range(Nmax, Nmax + lmax + 1):
        if params[i] < 0:
            return R.reject("negative visibility (parameter %d)" % i)
    o = Nmax + lmax + Nf
    if model_index == 9:
        i0 = Nfl[0]
        for el in range(1, lmax + 1):
            for j in range(1, 6):
                for n in range(Nfl[el]):
                    fl = float(params[Nmax + lmax + i0 + n])
                    a1 = float(params[o]) + float(params[o + 1]) * (fl * 1e-3)
                    aj = float(params[o + 2 * j]) + float(params[o + 2 * j + 1]) * (fl * 1e-3)
                    ratio = abs(aj / a1) if a1 != 0 else math.inf
                    R.margins.append(("a%d/a1 l=%d n=%d" % (j + 1, el, n), ratio, limit[j]))
                    if ratio >= limit[j]:
                        return R.reject("|a%d/a1| over its limit at l=%d n=%d" % (j + 1, el, n))
                    if a1 < 0:
                        return R.reject("a1 < 0 at l=%d n=%d" % (el, n))
            i0 = i0 + Nfl[el]
    elif 0 <= model_index <= 8:
        raise Unsupported("model_index %d" % model_index)
    else:
        if impose_normHnlm == 1:
            q = o + Nsplit + Nwidth + Nnoise
            p = [float(v) for v in params[q:q + 9]]
            sums = [p[0] + 2 * p[1], p[2] + 2 * p[3] + 2 * p[4], p[5] + 2 * p[6] + 2 * p[7] + 2 * p[8]]
            for l, s in enumerate(sums, 1):
                R.margins.append(("ratio sum l=%d (upper)" % l, s, 1. + 1e-10))
                R.margins.append(("ratio sum l=%d (lower)" % l, s, 0.0))
                R.add("ratio sum l=%d" % l, logP_uniform(A, A.num(0), A.num(1. + 1e-10), A.num(s)))
        elif impose_normHnlm != 0:
            raise Unsupported("impose_normHnlm %d" % impose_normHnlm)
    on = o + Nsplit + Nwidth
    bad = _noise_checks(R, params, sw, on, o + 9)
    if bad:
        return R.reject(bad)
    _generic(A, R, params, priors, sw)
    fl0 = params[Nmax + lmax:Nmax + lmax + Nfl[0]]
    Dnu = linfit_slope(fl0)
    if Nfl[0] == Nfl[2]:
        for i in range(Nfl[0]):
            d02 = float(params[Nmax + lmax + i]) - float(params[Nmax + lmax + Nfl[0] + Nfl[1] + i])
            R.add("d02 %d" % i, logP_gaussian_uniform(A, A.num(0), A.num(Dnu / 3.), A.num(0.015 * Dnu), A.num(d02)))
    if smooth_switch == 1:
        i0 = 0
        for el in range(lmax + 1):
            if Nfl[el] != 0:
                d = second_differences(params[Nmax + lmax + i0:Nmax + lmax + i0 + Nfl[el]])
                for i in range(Nfl[el]):
                    R.add("smoothness l=%d %d" % (el, i), logP_gaussian(A, A.num(0), A.num(scoef), A.num(d[i])))
            i0 = i0 + Nfl[el]
    return R


def _asymptotic(A, R, params, pl, priors, sw, extra):
    scoef, a3ova1_limit, model_switch = float(extra[1]), float(extra[2]), int(extra[4])
    Nmax, lmax, Nfl0, Nfl1, Nfl2, Nfl3 = (int(pl[k]) for k in range(6))
    Nsplit, Nwidth = int(pl[6]), int(pl[7])
    Nf = Nfl0 + Nfl1 + Nfl2 + Nfl3
    i0 = Nmax + lmax + Nf + Nsplit
    a3 = float(params[Nmax + lmax + Nf + 4])
    rot_env = abs(float(params[Nmax + lmax + Nf]))
    for i in range(Nmax, Nmax + lmax + 1):
        if params[i] < 0:
            return R.reject("negative visibility (parameter %d)" % i)
    ratio = abs(a3 / rot_env) if rot_env != 0 else math.inf
    R.margins.append(("a3/rot_env", ratio, a3ova1_limit))
    if ratio >= a3ova1_limit:
        return R.reject("|a3/rot_env| over its limit")
    bad = _noise_checks(R, params, sw, i0 + Nwidth, Nmax + lmax + Nf + 9)
    if bad:
        return R.reject(bad)
    i = i0
    while i < i0 + Nwidth:
        if sw[i] == 2 and params[i] < 0:
            return R.reject("negative width-law parameter %d" % i)
        i += 1
    _generic(A, R, params, priors, sw)
    if model_switch == 1:
        raise Unsupported("model_switch 1")
    if model_switch == 3:
        if params[Nmax + lmax + Nfl0 + 6] < 0:
            return R.reject("negative Wfactor")
        if params[Nmax + lmax + Nfl0 + 7] < 0:
            return R.reject("negative Hfactor")
    if sw[i] == 1:  # (:466: the loop variable of the width check, left at i0 + Nwidth)
        if Nfl0 != 0:
            d = second_differences(params[Nmax + lmax:Nmax + lmax + Nfl0])
            for k in range(Nfl0):
                R.add("smoothness l=0 %d" % k, logP_gaussian(A, A.num(0), A.num(scoef), A.num(d[k])))
        if Nfl3 != 0:
            s = Nmax + lmax + Nfl0 + Nfl1 + Nfl2
            d = second_differences(params[s:s + Nfl3])
            for k in range(Nfl3):
                R.add("smoothness l=3 %d" % k, logP_gaussian(A, A.num(0), A.num(scoef), A.num(d[k])))
    return R


def _local(A, R, params, pl, priors, sw, extra):
    a3ova1_limit = float(extra[2])
    o = int(pl[0]) + int(pl[1]) + int(pl[2]) + int(pl[3]) + int(pl[4]) + int(pl[5])
    Nsplit, Nwidth, Nnoise = int(pl[6]), int(pl[7]), int(pl[8])
    if params[o] != 0:
        ratio = abs(float(params[o + 2]) / float(params[o]))
        R.margins.append(("a3/a1 (a1 fitted)", ratio, a3ova1_limit))
        if ratio >= a3ova1_limit:
            return R.reject("|a3/a1| over its limit (a1 fitted)")
    elif params[o + 3] != 0 and params[o + 4] != 0:
        ratio = abs(float(params[o + 2]) / (float(params[o + 3]) ** 2 + float(params[o + 4]) ** 2))
        R.margins.append(("a3/a1 (sqrt(a1) cos i, sin i)", ratio, a3ova1_limit))
        if ratio >= a3ova1_limit:
            return R.reject("|a3/a1| over its limit (sqrt(a1) cos i, sin i)")
    oi = o + Nsplit + Nwidth + Nnoise
    if sw[oi] != 0 and params[oi] < 0:
        return R.reject("negative inclination")
    _generic(A, R, params, priors, sw)
    return R


def _width_bound(A, R, numax, sigma):
    """sigma < beta0 numax^beta1 / 2 with beta0, beta1 double literals held in long doubles and the power taken in long double."""
    if A is _Exact:
        Dnu_expected = Decimal(0.263) * Decimal(float(numax)) ** Decimal(0.77)
        s = Decimal(float(sigma))
    else:
        Dnu_expected = 0.263 * float(numax) ** 0.77
        s = float(sigma)
    R.margins.append(("Stello width bound", s, Dnu_expected / 2))
    return s < Dnu_expected / 2


def _harvey_gaussian(A, R, params, priors, sw):
    if _width_bound(A, R, params[8], params[9]):
        return R.reject("Gaussian width under the Stello bound")
    _generic(A, R, params, priors, sw)
    return R


def _kallinger_gaussian(A, R, params, priors, sw):
    if params[5] < 0 or params[6] < 0:
        return R.reject("negative a1 or a2")
    if _width_bound(A, R, params[15], params[16]):
        return R.reject("Gaussian width under the Stello bound")
    if A.num(params[15]) + A.num(params[17]) < 0:
        return R.reject("numax + mu_numax < 0")
    R.add("mu_numax", logP_gaussian(A, A.num(0), A.fabs(A.num(params[18])), A.num(params[17])))
    _generic(A, R, params, priors, sw)
    return R


def log_prior(prior_class, params, plength, priors, priors_switch, extra_priors, exact=True):
    A = _Exact if exact else _Double
    R = Result(A)
    params = [float(v) for v in params]
    priors = [[float(v) for v in row] for row in priors]
    sw = [int(v) for v in priors_switch]
    pl = [int(v) for v in plength]
    extra = [float(v) for v in extra_priors]
    with localcontext() as ctx:
        ctx.prec = PREC
        if prior_class == 0:
            _kallinger_gaussian(A, R, params, priors, sw)
        elif prior_class == 1:
            _harvey_gaussian(A, R, params, priors, sw)
        elif prior_class == 2:
            _ms_global(A, R, params, pl, priors, sw, extra)
        elif prior_class == 3:
            _local(A, R, params, pl, priors, sw, extra)
        elif prior_class == 4:
            _asymptotic(A, R, params, pl, priors, sw, extra)
        else:
            raise Unsupported("prior class %d" % prior_class)
        R.value, R.scale = R._value(), R._scale()  # (formed inside the 50-digit context)
    return R


def star_log_prior(star, params=None, exact=True):
    return log_prior(int(star.prior_class), star.params if params is None else params, star.plength, star.priors, star.priors_switch,
                     star.extra_priors, exact=exact)

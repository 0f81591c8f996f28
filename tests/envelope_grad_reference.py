"""50-digit derivative of S(theta) = sum_i (y_i / M_i + ln M_i) for the Gaussian-envelope fits (ids 0, 1), and of the row quantities.

S is written from the model statements of tests/envelope_numpy.py (which restates the reference) in mpmath at 50 digits and
differentiated as it stands, by a central difference with a step of 1e-20 (truncation ~1e-40 |S'''|, rounding ~1e-30 |S|): no derivative
formula is shared with the kernels or with tests/envelope_grad_numpy.py.  Two exact rewritings keep it quick: sum_i ln M_i = ln prod_i M_i
(mpmath's exponent range is unbounded), and a component of M that a perturbation does not touch is taken from a cache keyed by the
component's own parameters.

The convention of include/tamcmc_hip.h for |p|: d|p|/dp = copysign(1, p) -- here |p| is s p with s = copysign(1, p) of the base point,
so the difference is two-sided also at p = 0.  A Harvey term with tc = 0 is switched off (the model's own `if`): S is not continuous in tc
there and the component of that tc is not defined (`None`)."""
import math

import mpmath as mp

mp.mp.dps = 50
H = mp.mpf(10) ** -20
HALF_PI = mp.mpf(0.5 * math.pi)   # 0.5*M_PI: the double constant
MILLI = mp.mpf(1e-3)              # the double constant


def _signs(p):
    return [mp.mpf(math.copysign(1.0, float(v))) for v in p]


class EnvelopeS:
    """S of one spectrum (x, y: float64 arrays) as a function of the parameter vector."""

    def __init__(self, model_id, x, y):
        self.id = int(model_id)
        self.x = [mp.mpf(float(v)) for v in x]
        self.y = [mp.mpf(float(v)) for v in y]
        self.lnx = [mp.log(v) if v != 0 else None for v in self.x]
        self.n = len(self.x)
        self._cache = {}
        if self.id == 0:
            xn = max(self.x)
            self.eta2 = []
            for i, v in enumerate(self.x):
                if i == 0 and v == 0:
                    self.eta2.append(mp.mpf(1))
                else:
                    a = HALF_PI * v / xn
                    self.eta2.append((mp.sin(a) / a) ** 2)

    # ---- components (cached by their own parameters) ----
    def _power(self, lnscale, expo):
        """(scale x)^expo per bin, scale = exp(lnscale) > 0; at x = 0: 0 for expo > 0, 1 for expo = 0."""
        out = []
        for lx in self.lnx:
            if lx is None:
                out.append(mp.mpf(1) if expo == 0 else (mp.mpf(0) if expo > 0 else mp.inf))
            else:
                out.append(mp.exp(expo * (lnscale + lx)))
        return out

    def _lorentz(self, lnscale, expo):
        key = ("L", lnscale, expo)
        if key not in self._cache:
            self._cache[key] = [1 / (1 + t) if t != mp.inf else mp.mpf(0) for t in self._power(lnscale, expo)]
        return self._cache[key]

    def _gauss(self, numax, sig2):
        key = ("G", numax, sig2)
        if key not in self._cache:
            g = [mp.exp((mp.mpf(-0.5) * (v - numax) ** 2) / sig2) for v in self.x]
            if self.id == 0:
                g = [a * b for a, b in zip(self.eta2, g)]
            self._cache[key] = g
        return self._cache[key]

    def model(self, p, s):
        """M per bin; p: mpf list, s: the frozen signs of the base point."""
        A = lambda j: s[j] * p[j]   # |p_j|
        if self.id == 1:
            g = self._gauss(p[8], A(9) ** 2)
            m = [A(7) * v for v in g]
            for k in range(2):
                tc = A(3 * k + 1)
                if tc != 0:
                    L = self._lorentz(mp.log(MILLI * tc), A(3 * k + 2))
                    Hk = A(3 * k)
                    m = [a + Hk * b for a, b in zip(m, L)]
            return [a + A(6) for a in m]
        Amax, numax, sig, mu = A(14), A(15), A(16), p[17]
        g = self._gauss(numax, sig ** 2)
        N0 = A(13)
        m = [Amax * v + N0 for v in g]
        nm = numax + mu
        snm = 1 if nm >= 0 else -1
        a0 = p[0] * numax ** p[1]
        h = self.x[1] - self.x[0]
        for a, i, j, ic in ((a0, 2, 3, 4), (p[5], 7, 8, 9), (p[6], 10, 11, 12)):
            b = s[i] * p[i] * (snm * nm) ** p[j]        # |p_i |numax + mu|^p_j|
            c = A(ic)
            L = self._lorentz(-mp.log(b), c)            # 1 / (1 + (x / b)^c)
            key = ("I", -mp.log(b), c)
            if key not in self._cache:
                self._cache[key] = mp.fsum(L) - (L[0] + L[-1]) / 2
            ksi = b / (self._cache[key] * h)
            coef = ksi * a ** 2 / b
            m = [u + coef * v for u, v in zip(m, L)]
        return m

    def S(self, p, s):
        m = self.model(p, s)
        prod = mp.mpf(1)
        acc = mp.mpf(0)
        for yi, mi in zip(self.y, m):
            acc += yi / mi
            prod *= mi
        return acc + mp.log(prod)

    def gradient(self, params):
        """dS/dtheta_j, j < 10 (id 1) / 19 (id 0), as mpf; None for the tc of a switched-off Harvey term."""
        base = [mp.mpf(float(v)) for v in params]
        s = _signs(params)
        n = 10 if self.id == 1 else 19
        out = []
        for j in range(n):
            if self.id == 1 and j in (1, 4) and base[j] == 0:
                out.append(None)
                continue
            if self.id == 0 and j == 18:
                out.append(mp.mpf(0))   # omega_numax: read by the prior only
                continue
            up, dn = list(base), list(base)
            up[j] += H
            dn[j] -= H
            out.append((self.S(up, s) - self.S(dn, s)) / (2 * H))
        self._cache.clear()
        return out


# ---- the row quantities (the scalars formed once per vector), in the order of tamcmc_hip_envelope_gradient_sums ----
def row_quantities(model_id, p, s):
    A = lambda j: s[j] * p[j]
    if model_id == 1:
        r = [A(7), p[8], A(9) ** 2, A(6), A(0), A(3)]
        r += [mp.log(MILLI * A(3 * k + 1)) if A(3 * k + 1) != 0 else mp.mpf(0) for k in range(2)]
        return r + [A(2), A(5), mp.mpf(0), mp.mpf(0), mp.mpf(0)]
    numax, mu = A(15), p[17]
    nm = numax + mu
    snm = 1 if nm >= 0 else -1
    r = [A(14), numax, A(16) ** 2, A(13), (p[0] * numax ** p[1]) ** 2, p[5] ** 2, p[6] ** 2]
    r += [mp.log(s[i] * p[i] * (snm * nm) ** p[j]) for i, j in ((2, 3), (7, 8), (10, 11))]
    return r + [A(4), A(9), A(12)]


def row_jacobian(model_id, params):
    """J[q][j] = d(row quantity q)/d(parameter j) at 50 digits (None: not defined, the tc of a switched-off term)."""
    base = [mp.mpf(float(v)) for v in params]
    s = _signs(params)
    n = 10 if model_id == 1 else 19
    J = [[mp.mpf(0)] * n for _ in range(13)]
    for j in range(n):
        if model_id == 1 and j in (1, 4) and base[j] == 0:
            J[6 + j // 3][j] = None
            continue
        up, dn = list(base), list(base)
        up[j] += H
        dn[j] -= H
        a, b = row_quantities(model_id, up, s), row_quantities(model_id, dn, s)
        for q in range(13):
            J[q][j] = (a[q] - b[q]) / (2 * H)
    return J

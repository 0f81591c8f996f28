"""Long-double numpy restatement of the Gaussian-envelope background fits -- the checker of tests/test_gpu_envelope.py and
tests/test_envelope_inputs.py, written from the reference's statements and independent of the product code:
  model_Harvey_Gaussian (id 1)           tamcmc/sources/models.cpp + harvey_like, noise_models.cpp:15-39
  model_Kallinger2014_Gaussian (id 0)    tamcmc/sources/models.cpp + Kallinger2014, get_ksinorm, eta_squared_Kallinger2014
                                         (noise_models.cpp:70-153), as executed: eta^2 multiplies the Gaussian only
  priors_Harvey_Gaussian / priors_Kallinger2014_Gaussian   tamcmc/sources/priors_calc.cpp:631-703
  apply_generic_priors primitives        tamcmc/sources/stats_dictionary.cpp
Every array is np.longdouble (80-bit on x86-64), in the reference's order of operations."""
import numpy as np

LD = np.longdouble
PIl = LD("3.141592653589793238462643383279502884")


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def harvey_like(noise, x, y, nharvey):
    out = y.copy()
    for k in range(nharvey):
        tc = noise[3 * k + 1]
        if tc != 0:
            t = (LD(1e-3) * tc * x) ** noise[3 * k + 2]
            out = out + noise[3 * k] * (LD(1) / (t + LD(1)))
    return out + noise[-1]


def model_harvey_gaussian(params, x):
    p, x = _ld(params), _ld(x)
    m = (LD(-0.5) * (x - p[8]) ** 2) / np.abs(p[9]) ** 2
    m = np.abs(p[7]) * np.exp(m)
    return harvey_like(np.abs(p[0:7]), x, m, 2)


def eta_squared(x):
    xn = x.max()
    a = LD(0.5) * LD(np.pi) * x / xn  # 0.5*M_PI: the double constant
    with np.errstate(invalid="ignore", divide="ignore"):
        eta = np.sin(a) / a
    if x[0] == 0:
        eta[0] = 1
    return eta ** 2


def ksinorm(b, c, x):
    h = x[1] - x[0]
    with np.errstate(divide="ignore", over="ignore"):
        term = LD(1) / (LD(1) + (x / b) ** c)
    w = np.ones_like(x)
    w[0] = w[-1] = LD(0.5)
    integral = np.sum(w * term) * h
    return b / integral


def model_kallinger_gaussian(params, x):
    p, x = _ld(params), _ld(x)
    Amax, numax, sig, mu = np.abs(p[14]), np.abs(p[15]), np.abs(p[16]), p[17]
    g = (LD(-0.5) * (x - numax) ** 2) / np.abs(sig) ** 2
    m = np.abs(Amax) * eta_squared(x) * np.exp(g)
    n = p[0:14]
    a0 = np.abs(n[0] * np.abs(numax) ** n[1])
    b0 = np.abs(n[2] * np.abs(numax + mu) ** n[3])
    c0 = np.abs(n[4])
    a1, a2 = n[5], n[6]
    b1 = np.abs(n[7] * np.abs(numax + mu) ** n[8])
    b2 = np.abs(n[10] * np.abs(numax + mu) ** n[11])
    c1, c2, N0 = np.abs(n[9]), np.abs(n[12]), np.abs(n[13])
    power = m + N0
    for a, b, c in ((a0, b0, c0), (a1, b1, c1), (a2, b2, c2)):
        ksi = ksinorm(b, c, x)
        with np.errstate(divide="ignore", over="ignore"):
            power = power + (ksi * a ** 2 / b) * (LD(1) / ((x / b) ** c + LD(1)))
    return power  # (the leakage filter's product with the whole spectrum is discarded by the reference)


def model(model_id, params, x):
    return model_kallinger_gaussian(params, x) if model_id == 0 else model_harvey_gaussian(params, x)


def loglike(model_id, params, x, y, p=1.0, T=1.0):
    """likelihood_chi22p + call_likelihood: -p * (sum y/M + sum ln M) / T (long double)."""
    m = model(model_id, params, x)
    S = np.sum(_ld(y) / m) + np.sum(np.log(m))
    return float((-LD(int(p)) * S) / LD(T)), m


# ---- priors ----
def logP_uniform(bmin, bmax, x):
    return -np.log(np.abs(bmax - bmin)) if (x <= bmax) and (x >= bmin) else LD(-np.inf)


def logP_gaussian(mean, sigma, x):
    return -np.log(np.sqrt(2 * PIl) * sigma) - LD(0.5) * ((x - mean) / sigma) ** 2


def logP_jeffrey(hmin, hmax, h):
    if h < hmax and h > 0:
        prior, norm = LD(1) / (h + hmin), np.log((hmax + hmin) / hmin)
        return np.log(prior / norm)
    return LD(-np.inf)


def logP_gug(bmin, bmax, s1, s2, x):
    lp = LD(0)
    if x < bmin:
        lp = LD(-0.5) * ((x - bmin) / s1) ** 2
    if bmax >= x >= bmin:
        lp = LD(0)
    if x > bmax:
        lp = LD(-0.5) * ((x - bmax) / s2) ** 2
    return lp - np.log(np.abs(bmax - bmin) + LD(0.5) * np.sqrt(2 * PIl) * (s1 + s2))


def generic_priors(params, priors, sw):
    p, pp = _ld(params), _ld(priors)
    pena = LD(0)
    for i, s in enumerate(sw):
        if s == 0:
            t = LD(0)
        elif s == 1:
            t = logP_uniform(pp[0, i], pp[1, i], p[i])
        elif s == 2:
            t = logP_gaussian(pp[0, i], pp[1, i], p[i])
        elif s == 4:
            t = logP_jeffrey(pp[0, i], pp[1, i], p[i])
        elif s == 7:
            t = logP_gug(pp[0, i], pp[1, i], pp[2, i], pp[3, i], p[i])
        else:
            raise ValueError("prior id %d not restated" % s)
        pena = pena + t
    return pena


def _width_rejects(numax, sigma):
    beta0, beta1 = LD(0.263), LD(0.77)  # double literals held in long doubles
    with np.errstate(invalid="ignore"):
        dnu = beta0 * LD(numax) ** beta1
    return LD(sigma) < dnu / 2


def log_prior(prior_class, params, priors, sw):
    p = np.asarray(params, dtype=np.float64)
    if prior_class == 1:
        if _width_rejects(p[8], p[9]):
            return -np.inf
        return float(LD(0) + generic_priors(p, priors, sw))
    if prior_class == 0:
        if p[5] < 0 or p[6] < 0:
            return -np.inf
        if _width_rejects(p[15], p[16]):
            return -np.inf
        numax, mu, omega = LD(p[15]), LD(p[17]), LD(p[18])
        if numax + mu < 0:
            return -np.inf
        f = LD(0) + logP_gaussian(LD(0), np.abs(omega), mu)
        return float(f + generic_priors(p, priors, sw))
    raise ValueError(prior_class)

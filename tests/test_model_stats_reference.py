"""The accumulator law of the posterior model spectrum (tests/model_stats_numpy.py: the sequential replay of include/tamcmc_hip.h's
statements) against a two-pass evaluation in 50-digit arithmetic: the weighted mean, then the weighted mean of the squared deviations
from it, both over the exact values of the doubles in the rows.  No GPU.

Bounds (u = 2^-53, n accepted vectors, first order in u; the second-order terms are below 1e-13 of these for n = 200).

Mean.  mean = R + A1 / W.  With |d| <= max|M| and a mean that lies among the rows, the issue's bound is (n + 2) u max|M| per bin.

Variance.  var = (A2 - (A1 A1) / W) / W.  Write mu = mean - R (the mean of d), s1 = A1 / W = mu, s2 = A2 / W = sigma^2 + mu^2.
  * d = fl(M - R) carries a relative error u: the variance of the rounded d differs from that of d by at most
    2 u sum w |d| |d - mu| / W <= 2 u max|d| sigma (Cauchy-Schwarz);
  * a term w (d d) of A2 passes the square, the product and at most n - 1 additions:   (n + 1) u s2;
  * a term w d of A1 passes the product and n - 1 additions, A1 enters twice, then the product A1 A1, the division by W and W's own
    n - 1 additions:   (2 n + 2 + n - 1) u s1^2 = (3 n + 1) u mu^2;
  * the subtraction, the last division and W's error in it act on the result:   (n + 1) u sigma^2.
  Sum:  u [2 (n + 1) sigma^2 + (4 n + 2) mu^2 + 2 sigma max|d|].  The reference row is one of the rows, so |mu| <= max|d|, and where it
  lies within two standard deviations of the mean, |mu| <= 2 sigma, mu^2 <= 2 sigma max|d|:
      <= u [2 (n + 1) sigma^2 + (8 n + 6) sigma max|d|] <= 8 (n + 2) u (sigma^2 + sigma max|d|).
  That is where the constant 8 comes from; the rows below are built so that |mu| <= 2 sigma at every bin (asserted on the inputs).
  Without the shift mu is the mean model itself and the same sum reads ~ 4 n u mean^2: at a relative spread of 1e-12 that is 1e24 times
  sigma^2, which the last test pins."""
from decimal import Decimal, localcontext

import numpy as np
import pytest

import model_stats_numpy as msn

U = 2.0 ** -53
NX = 48
REF = 1e-45  # the 50-digit reference's own rounding, relative to max|M| (mean) and max|M|^2 (variance): added to each bound


def make_rows(spread, n, seed):
    """n accepted rows M0 (1 + spread g_b p_i) with g = 0 for the first accepted one, zero-weight rows in between (first position
    included).  Every bin has the same mu / sigma = mean_w(g) / std_w(g)."""
    rng = np.random.default_rng(seed)
    i = np.arange(NX)
    M0 = 1.0 + 10.0 * np.exp(-((i - 20.0) ** 2) / 30.0)
    p = 1.0 + 0.5 * np.sin(0.7 * i)
    g = rng.uniform(-0.5, 0.5, n)
    g[0] = 0.0
    w = rng.uniform(0.5, 2.0, n)
    rows_acc = M0[None, :] * (1.0 + spread * g[:, None] * p[None, :])
    # zero-weight rows (far off, so that a law which took them would miss every bound): before the first and after every third
    rows, weights = [M0 * 3.0], [0.0]
    for b in range(n):
        rows.append(rows_acc[b]); weights.append(w[b])
        if b % 3 == 1:
            rows.append(M0 * 0.25); weights.append(0.0)
    if n >= 2:
        gm = np.sum(w * g) / np.sum(w)
        gs = np.sqrt(np.sum(w * (g - gm) ** 2) / np.sum(w))
        assert abs(gm) <= 2.0 * gs, "test data: the reference row must lie within 2 sigma of the mean"
    return np.array(rows), np.array(weights)


def exact_two_pass(rows, weights):
    """(mean, var, sigma, max|d|, max|M|) per bin over the accepted rows, 50 digits, as floats of the exact values' nearest doubles
    except var and sigma, which stay Decimal-accurate to ~1e-50 before the final float()."""
    ok = msn.accepted(weights)
    R_, W_ = rows[ok], weights[ok]
    with localcontext() as ctx:
        ctx.prec = 50
        Wd = [Decimal(float(w)) for w in W_]
        Wsum = sum(Wd)
        mean, var = [], []
        for i in range(rows.shape[1]):
            col = [Decimal(float(v)) for v in R_[:, i]]
            m = sum(w * v for w, v in zip(Wd, col)) / Wsum
            s2 = sum(w * (v - m) * (v - m) for w, v in zip(Wd, col)) / Wsum
            mean.append(m); var.append(s2)
        sig = [v.sqrt() for v in var]
    maxd = np.max(np.abs(R_ - R_[0][None, :]), axis=0)  # (differences of nearby doubles: exact or within u of it, far inside the bound's slack)
    return mean, var, sig, maxd, np.max(np.abs(R_), axis=0)


def errors(out, mean, var):
    with localcontext() as ctx:
        ctx.prec = 50
        em = np.array([float(abs(Decimal(float(a)) - b)) for a, b in zip(out["mean"], mean)])
        ev = np.array([float(abs(Decimal(float(a)) - b)) for a, b in zip(out["var"], var)])
    return em, ev


@pytest.mark.parametrize("n", [1, 2, 200])
@pytest.mark.parametrize("spread", [1.0, 1e-6, 1e-12])
def test_replay_against_two_pass(spread, n):
    rows, weights = make_rows(spread, n, seed=int(-np.log10(spread)) * 1000 + n)
    out = msn.replay(rows, weights=weights)
    assert out["counts"] == (n, 0, len(weights) - n)
    assert out["W"] == pytest.approx(float(np.sum(weights)), rel=1e-13)
    mean, var, sig, maxd, maxM = exact_two_pass(rows, weights)
    em, ev = errors(out, mean, var)
    bound_m = (n + 2) * U * maxM + REF * maxM
    bound_v = 8 * (n + 2) * U * (np.array([float(v) for v in var]) + np.array([float(s) for s in sig]) * maxd) + REF * maxM ** 2
    print("spread %g n %d: mean error / bound %.3g, variance error / bound %.3g" %
          (spread, n, np.max(em / bound_m), np.max(ev / np.where(bound_v > 0, bound_v, 1.0))))
    assert np.all(em <= bound_m)
    assert np.all(ev <= bound_v)
    ok = msn.accepted(weights)
    assert np.array_equal(out["min"], rows[ok].min(axis=0)) and np.array_equal(out["max"], rows[ok].max(axis=0))
    if n == 1:
        assert np.array_equal(out["mean"], rows[ok][0]) and not out["var"].any()


def test_unshifted_law_fails_the_variance_bound():
    """The shift by the reference plane is part of the law: the textbook sums of w M and w M^2 miss the bound at a spread of 1e-12."""
    n = 200
    rows, weights = make_rows(1e-12, n, seed=12000 + n)
    mean, var, sig, maxd, maxM = exact_two_pass(rows, weights)
    bound_v = 8 * (n + 2) * U * (np.array([float(v) for v in var]) + np.array([float(s) for s in sig]) * maxd) + REF * maxM ** 2
    _, ev_shift = errors(msn.replay(rows, weights=weights), mean, var)
    _, ev_plain = errors(msn.replay(rows, weights=weights, shift=False), mean, var)
    assert np.all(ev_shift <= bound_v)
    assert np.all(ev_plain > bound_v)


def test_nan_contract_and_counts():
    """A non-finite M reaches mean, var and ratio of its bin and no other; failed tables and zero weights are counted apart."""
    rows, weights = make_rows(1e-6, 5, seed=5)
    rows = rows.copy()
    ok = np.flatnonzero(msn.accepted(weights))
    rows[ok[2], 7] = np.nan
    status = np.zeros(len(weights), dtype=int)
    status[ok[4]] = -3
    y = np.ones(NX)
    out = msn.replay(rows, y=y, weights=weights, status=status)
    assert out["counts"] == (4, 1, len(weights) - 5)
    for k in ("mean", "var", "ratio"):
        assert np.isnan(out[k][7]) and np.isfinite(np.delete(out[k], 7)).all(), k
    assert np.isfinite(out["min"]).all() and np.isfinite(out["max"]).all()

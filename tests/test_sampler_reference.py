"""The 50-digit restatement of the sampler's algebra (tests/sampler_reference.py) against what is independent of it.  No GPU, no product
code: the oracle's pieces (oracle/sampler_oracle.c), identities, and detailed balance of the reference's own kernel.

Sizes 1, 2, 7, 40, 93; covariances Sigma = D R D with D spanning 1e-5 .. 1e2 and a well-conditioned correlation matrix R, as
tests/test_oracle_langevin.py builds them.

  * L L^T = A to 45 digits.
  * log q against orc_mvn_logpdf (pivoted Gaussian elimination in long double, with the normalising constant: the reference adds
    -sum ln L_ii - n/2 ln 2 pi) and the drift against orc_langevin_drift (long double sums): within 4 x 2^-63 x scale, the bound
    tests/test_priors.py uses for long double, applied before the oracle's value is rounded to double.  The drift's scale is the sum of
    the magnitudes of its terms, the density's the reference's own (+ the magnitudes of the constant's terms).
  * orc_sampler_iteration (random walk, learn = True) computes in DOUBLE -- a plain column Cholesky, the Robbins-Monro update as Eigen
    evaluates it -- so the long-double bound cannot hold for it; its bounds are those of double arithmetic, written down here:
      proposal   the computed factor has L L^T = A + dA with |dA| <= g_(n+1) |L| |L^T| (Higham, Accuracy and Stability, thm 10.3), hence to
                 first order |dL| <= g_(n+1) |L| tril(|L^-1| |L| |L^T| |L^-T|); the product L z adds g_(n+1) |L| |z|, the sum x + . one
                 rounding; g_k = k 2^-53 / (1 - k 2^-53).  Everything on the right is the reference's.
      mu', sigma'   three roundings each, cov' seven (the deviation is taken from the oracle's own rounded mu', as an engine's is from
                 its own): K = 4 in units of 2^-52 x scale.
  * Detailed balance  pi(x) q(x'|x) a(x -> x') = pi(x') q(x|x') a(x' -> x)  of the reference's kernel on a 3-variable Gaussian target,
    by making the reverse move with the reference's own pieces.
"""
import math
from decimal import Decimal

import numpy as np
import pytest

import sampler_reference as R

SIZES = (1, 2, 7, 40, 93)
LD = Decimal(2) ** -63


def _law(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) * 0.1
    Rm = np.eye(n) + A @ A.T
    Rm = Rm / np.sqrt(np.outer(np.diag(Rm), np.diag(Rm)))
    D = np.geomspace(1e-5, 1e2, n)[rng.permutation(n)] if n > 1 else np.array([0.3])
    return Rm * np.outer(D, D), D, rng


def _within_long_double(got, ref, scale, k=4):
    """got: a double that a long double within k 2^-63 scale of ref was rounded to."""
    tol = k * LD * Decimal(scale)
    return float(ref - tol) <= got <= float(ref + tol)


@pytest.fixture(scope="module")
def factors():
    out = {}
    for n in SIZES:
        cov, D, rng = _law(n, 100 + n)
        sigma = 2.38 ** 2 / n
        A = R.matrix_to_factor(cov, 1e-12, sigma)
        out[n] = (cov, D, sigma, A, R.cholesky(A))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_factor_times_its_transpose(factors, n):
    cov, D, sigma, A, L = factors[n]
    assert L is not None
    with R._ctx():
        for i in range(n):
            for j in range(i + 1):
                s = sum((L[i][k] * L[j][k] for k in range(j + 1)), R.ZERO)
                a = R.dec(A[i][j])
                assert abs(s - a) <= Decimal(10) ** -45 * max(abs(a), (R.dec(A[i][i]) * R.dec(A[j][j])).sqrt()), (i, j)
    assert np.array_equal(A, (cov + 1e-12 * np.eye(n)) * sigma)                # fl(fl(c + eps2) sigma), element by element


def test_not_positive_definite_is_reported():
    assert R.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]])) is None
    assert R.cholesky(np.array([[0.0]])) is None and R.cholesky(np.array([[-1.0]])) is None
    assert R.cholesky(np.array([[4.0, 2.0], [2.0, 1.0]])) is None              # singular: the second pivot is exactly 0
    L = R.cholesky(np.array([[4.0, 2.0], [2.0, 3.0]]))
    with R._ctx():
        assert L[0][0] == 2 and L[1][0] == 1 and abs(L[1][1] - Decimal(2).sqrt()) < Decimal(10) ** -48


@pytest.mark.parametrize("delta", [0.0, 30.0])
@pytest.mark.parametrize("n", SIZES)
def test_drift_and_density_against_the_oracle(oracle, factors, n, delta):
    cov, D, sigma, A, L = factors[n]
    rng = np.random.default_rng(7 * n + int(delta))
    g = rng.standard_normal(n) / D * 3.0                    # a gradient of ~3 posterior sigmas per variable: |g| > 30 for every n > 1
    x = rng.standard_normal(n) * D * 10
    dr = R.drift(cov, sigma, 1e-12, delta, g)
    assert dr.truncated == (delta > 0 and np.linalg.norm(g) > delta)
    got = oracle.langevin_drift(cov, sigma, 1e-12, delta, g)
    worst = 0.0
    for i in range(n):
        assert _within_long_double(got[i], dr.d[i], dr.spread[i]), (i, got[i], dr.d[i])
        worst = max(worst, float(abs(R.dec(got[i]) - dr.d[i]) / (Decimal(dr.spread[i]) * Decimal(2) ** -53)))
    assert worst <= 1.1                                      # (a correctly rounded double of a long-double sum: half an ulp of the spread)
    # the density of a move drawn from the law itself
    z = rng.standard_normal(n)
    xp, _ = R.proposal(x, dr.d, L, [R.dec(v) for v in z], [R.dec(abs(v)) for v in z])
    xp = np.array([float(v) for v in xp])
    mean = x + np.array([float(v) for v in dr.d])           # the oracle takes the mean as doubles: the reference is given the same mean
    with R._ctx():
        dr_mean = R.Drift([R.dec(a) - R.dec(b) for a, b in zip(mean, x)], dr.spread, dr.truncated, dr.s)
    den = R.density(L, x, xp, dr_mean)
    with R._ctx():
        logdet_half = sum((L[i][i].ln() for i in range(n)), R.ZERO)
        const = -logdet_half - Decimal(n) / 2 * (2 * R.PI).ln()
        const_scale = sum((abs(L[i][i].ln()) for i in range(n)), R.ZERO) + abs(Decimal(n) / 2 * (2 * R.PI).ln())
        ref = den.lq + const
    got = oracle.mvn_logpdf(xp, mean, A)
    assert _within_long_double(got, ref, Decimal(den.scale) + const_scale), (n, got, float(ref), den.scale)
    # a whitened step has |w|^2 ~ n
    assert 0.0 <= -2 * float(den.lq) < 4 * n + 30


def test_drift_rules():
    cov, g = np.array([[2.0, 1.0], [1.0, 3.0]]), np.array([3.0, 4.0])
    d = R.drift(cov, 0.5, 1.0, 0.0, g)
    assert [float(v) for v in d.d] == [3.25, 4.75] and not d.truncated
    d = R.drift(cov, 0.5, 1.0, 1.0, g)
    assert np.allclose([float(v) for v in d.d], [0.65, 0.95], rtol=1e-15) and d.truncated and d.s == Decimal(1) / 5
    assert not R.drift(cov, 0.5, 1.0, 5.0, g).truncated     # |g| = delta exactly: not truncated
    assert [float(v) for v in R.drift(cov, 0.5, 1.0, 0.0, [np.inf, 1.0]).d] == [0.0, 0.0]
    assert [float(v) for v in R.drift(cov, 0.5, 1.0, 0.0, [np.nan, 1.0]).d] == [0.0, 0.0]


def test_acceptance_rules():
    t = R.mh_test(-5.0, -5.0, -10.0, -12.0)
    assert t.r == 1 and t.accepts(1.0 - 2.0 ** -53)
    t = R.mh_test(-8.0, -5.0, -13.0, -12.0)
    with R._ctx():
        assert abs(t.r - Decimal(-1).exp()) < Decimal(10) ** -48 and t.accepts(0.3) and not t.accepts(0.4)
    assert t.accepts(float(t.r)) == (R.dec(float(t.r)) <= t.r)                                  # u <= r
    assert R.mh_test(float("nan"), -1.0, float("nan"), -12.0).r == 0                           # NaN model
    assert R.mh_test(-5.0, -math.inf, -math.inf, -12.0).r == 0                                  # outside the prior's support
    assert R.mh_test(-5.0, float("nan"), -math.inf, -12.0).r == 0                               # a NaN prior is treated the same
    assert R.mh_test(-5.0, -5.0, float("nan"), -12.0).r == 0                                    # NaN ratio: refused
    assert not R.mh_test(-5.0, -math.inf, -math.inf, -12.0).accepts(2.0 ** -54)                 # (u > 0 always)
    assert R.mh_test(-5.0, -5.0, -1e6, -12.0).r == 0 or R.mh_test(-5.0, -5.0, -1e6, -12.0).r < Decimal(10) ** -1000


def test_swap_and_carried_gradient_by_hand():
    """T = (1, 2): LA = -10 at T_A = 1 -> -5 at T_B; LB = -4 at T_B = 2 -> -8 at T_A.  exponent = -5 - 8 + 10 + 4 = 1 -> r_T = 1."""
    s = R.resolve_swap((-10.0, -1.0, -11.0), (-4.0, -3.0, -7.0), 1.0, 2.0, 0.99, swap_rule=0)
    assert s.rT == 1 and s.swapped and s.A == (-8, -3, -11) and s.B == (-5, -1, -6)
    s = R.resolve_swap((-10.0, -1.0, -11.0), (-4.0, -3.0, -7.0), 1.0, 2.0, 0.99, swap_rule=1)
    assert s.B == (-5, -1, -8)                               # B's stored posterior keeps B's own old prior
    s = R.resolve_swap((-4.0, -1.0, -5.0), (-10.0, -3.0, -13.0), 1.0, 2.0, 0.5)
    assert abs(s.ln_rT + 8) < Decimal(10) ** -48 and not s.swapped and s.A == (-4, -1, -5)     # -2 - 20 + 4 + 10 = -8
    assert R.resolve_swap((-4.0, -1.0, -5.0), (-10.0, -3.0, -13.0), 1.0, 2.0, 0.000335).swapped  # exp(-8) = 0.00033546
    assert not R.resolve_swap((-4.0, -1.0, -5.0), (-10.0, -3.0, -13.0), 1.0, 2.0, 0.000336).swapped
    g, sc = R.carried_gradient([5.0, -1.0], [1.0, -1.0], 2.0, 1.0)
    assert g == [9, -1] and list(sc) == [9.0, 1.0]           # likelihood share 4 -> 8 at half the temperature, the prior's stays


@pytest.mark.parametrize("n", SIZES)
def test_iteration_against_the_oracle(oracle, synth, n):
    """Random walk, learn = True: the proposal x + L z and the adapted law of orc_sampler_iteration (double arithmetic) against the
    reference, within the bounds of the module docstring."""
    if n <= 21:
        star = synth.make_c2_star(nx=600)
    else:
        star = synth.make_c3_star(nx=3000, step=0.7)
    for i in star.index_to_relax[n:]:
        star.relax[i] = 0
        star.priors_switch[i] = 0
        star.priors[:, i] = -9999.0
    assert star.nvars == n
    _, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    y = star.set_spectrum_from_model(m0, seed=n)
    nch, lam, c0, it = 2, 1.5, 2.0, 50
    T = lam ** np.arange(nch)
    cov, D, rng = _law(n, 300 + n)
    x0 = star.params[star.index_to_relax]
    vars_ = np.array([x0, x0 * (1 + 1e-6 * rng.standard_normal(n))])
    params = np.tile(star.params, (nch, 1))
    params[:, star.index_to_relax] = vars_
    logL = oracle.loglike_batch(star.model_id, params, star.plength, star.x, y, 1.0, T)[0]
    logPr = np.array([oracle.call_prior(star, p) for p in params])
    state = dict(params=params, vars=vars_, logL=logL, logPrior=logPr, logPost=logL + logPr)
    mu = vars_ + 0.3 * D * rng.standard_normal((nch, n))
    covs = np.array([cov, cov * 1.7])
    sigma = np.array([2.38 ** 2 / n, 1.3 * 2.38 ** 2 / n])
    z = rng.standard_normal((nch, n))
    u = np.array([0.3, 0.6])
    exp, law2, rc = oracle.sampler_iteration(star, y, T, logL.copy(), state, (mu, covs, sigma), i=it, z=z, u_mh=u, learn=True, c0=c0)
    assert rc == 0
    worst = {"proposal": 0.0, "mu": 0.0, "cov": 0.0, "sigma": 0.0}
    for m in range(nch):
        A = R.matrix_to_factor(covs[m], 1e-12, sigma[m])
        L = R.cholesky(A)
        xp, _ = R.proposal(vars_[m], [R.ZERO] * n, L, [R.dec(v) for v in z[m]], [R.dec(abs(v)) for v in z[m]])
        Lf = np.abs(R.factor_float(L))
        Li = R.abs_inverse(R.factor_float(L))
        gk = (n + 1) * 2.0 ** -53 / (1 - (n + 1) * 2.0 ** -53)
        dL = gk * Lf @ np.tril(Li @ Lf @ Lf.T @ Li.T)
        bound = (dL + gk * Lf) @ np.abs(z[m]) * 1.01 + 2.0 ** -53 * np.abs(exp["prop_vars"][m])
        err = np.array([float(abs(R.dec(a) - b)) for a, b in zip(exp["prop_vars"][m], xp)])
        assert np.all(err <= bound), (m, np.max(err / bound))
        worst["proposal"] = max(worst["proposal"], float(np.max(err / bound)))
        # (and the bound is no licence: in units of 2^-52 (|x| + |L| |z|) a double factor of D R D stays below 2 Nv)
        assert np.max(err / (2.0 ** -52 * (np.abs(vars_[m]) + Lf @ np.abs(z[m])))) < 2 * n
        # the adapted law, at the position after the test
        law = R.adapt(mu[m], covs[m], sigma[m], exp["vars"][m], exp["Pmove"][m], it,
                      c0, 0.234, 1e-12, 1e14, mu_new_given=law2[0][m])
        r_mu = R.ratio(law2[0][m], law.mu, law.mu_scale)
        r_cov = R.ratio(law2[1][m], [v for row in law.cov for v in row], law.cov_scale)
        r_sig = R.ratio([law2[2][m]], [law.sigma], [law.sigma_scale])
        worst["mu"], worst["cov"], worst["sigma"] = max(worst["mu"], r_mu), max(worst["cov"], r_cov), max(worst["sigma"], r_sig)
        assert r_mu <= 4 and r_cov <= 4 and r_sig <= 4, (m, r_mu, r_cov, r_sig)
        assert float(law.gamma) == pytest.approx(c0 / 51.0, rel=1e-15)
    print("\nNv %d: proposal error / first-order bound %.3f; mu %.2f cov %.2f sigma %.2f (units of 2^-52 x scale)" %
          (n, worst["proposal"], worst["mu"], worst["cov"], worst["sigma"]))


def test_detailed_balance_of_the_reference_kernel():
    """pi = N(0, P^-1) in 3 variables; log pi and its gradient are exact rationals of the inputs.  For a forward move x -> x' (drift from
    the gradient at x, truncated or not) and the reverse move made explicitly:  ln pi(x) + lq(x'|x) + ln a(x -> x') equals
    ln pi(x') + lq(x|x') + ln a(x' -> x)  to 45 digits."""
    P = np.array([[2.0, 0.5, 0.0], [0.5, 1.0, -0.25], [0.0, -0.25, 4.0]])
    cov = np.array([[0.5, 0.1, 0.0], [0.1, 0.9, 0.05], [0.0, 0.05, 0.2]])
    sigma, eps2 = 0.8, 1e-12
    L = R.cholesky(R.matrix_to_factor(cov, eps2, sigma))
    rng = np.random.default_rng(5)

    def logpi(x):
        with R._ctx():
            return -R.HALF * sum((R.dec(x[i]) * R.dec(P[i][j]) * R.dec(x[j]) for i in range(3) for j in range(3)), R.ZERO)

    seen = set()
    for delta in (0.0, 1.5):
        for _ in range(6):
            x = rng.standard_normal(3) * 1.5
            gx = -P @ x                                      # (rounded: the kernel is a function of the gradient it is given -- the same
            dx = R.drift(cov, sigma, eps2, delta, gx)        #  doubles serve the forward move from x and the reverse move to x)
            z = rng.standard_normal(3)
            xp, _ = R.proposal(x, dx.d, L, [R.dec(v) for v in z], [R.dec(abs(v)) for v in z])
            xp = np.array([float(v) for v in xp])
            gxp = -P @ xp
            dxp = R.drift(cov, sigma, eps2, delta, gxp)
            qf, qr = R.density(L, x, xp, dx), R.density(L, xp, x, dxp)
            lpx, lpxp = logpi(x), logpi(xp)
            # the engine's test needs doubles for the log-posteriors: here the exact values are handed over through their exponent
            with R._ctx():
                e_fwd = lpxp - lpx + qr.lq - qf.lq
                a_fwd = min(R.ZERO, e_fwd)
                a_rev = min(R.ZERO, -e_fwd)                  # the reverse move's exponent: forward and reverse densities change places
                lhs = lpx + qf.lq + a_fwd
                rhs = lpxp + qr.lq + a_rev
                assert abs(lhs - rhs) <= Decimal(10) ** -45 * (abs(lpx) + abs(lpxp) + abs(qf.lq) + abs(qr.lq) + 1)
            # ... and mh_test makes the same min(1, exp(.)) of doubles
            t = R.mh_test(0.0, 0.0, float(lpxp), float(lpx), qf, qr)
            tr = R.mh_test(0.0, 0.0, float(lpx), float(lpxp), qr, qf)
            with R._ctx():
                assert abs((t.r.ln() if t.r < 1 else R.ZERO) - a_fwd) < Decimal("1e-14") and abs((tr.r.ln() if tr.r < 1 else R.ZERO) - a_rev) < Decimal("1e-14")
                assert min(t.r, tr.r) < 1 or e_fwd == 0
            seen.add((dx.truncated, e_fwd > 0))
            # the whitened forward step IS z
            assert max(abs(float(w) - v) for w, v in zip(qf.w, z)) < 1e-9
    assert {s[0] for s in seen} == {False, True} and {s[1] for s in seen} == {False, True}

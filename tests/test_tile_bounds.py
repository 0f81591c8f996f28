"""The truncation bounds of the FAST tile's two series, pinned on the CPU: the Python-double restatement of the device's recurrences
(tile_series.py) against the 50-digit definition (tile_reference.py).  TAU_FAR, TAU_ASYM and HARVEY_BUDGET, the only tolerances the
GPU test imports, are what these tests hold the series to."""
import math
from decimal import Decimal, localcontext

import pytest

import tile_reference as tr
import tile_series as ts

S_GRID = [-1.0 + i / 20.0 for i in range(41)]
A_GRID = (0.0, 0.5, 1.0, 3.0, 10.0, 100.0, 1e4)
# what the restatement's own double arithmetic adds to a truncation bound: NC coefficients by a three-term recurrence and NC Horner
# steps, a rounding each, on terms of one magnitude (rho < 1: no growth)
ROUNDING = 4 * ts.NC * 2.0 ** -53


def _D(v):
    return Decimal(float(v))


def _far_exact(hv, A, beta, s):
    with localcontext() as c:
        c.prec = tr.PREC
        return _D(hv) / (1 + (_D(beta) * _D(s) - _D(A)) ** 2)


def _far_worst(A, q2, early_stop=True):
    """Worst |series - definition| / definition over the tile of one component with rho^2 = q2 (as the device's far_seed computes it)."""
    beta = math.sqrt(q2 * (A * A + 1.0))
    seed = ts.far_seed(1.0, A, beta)
    fc = ts.far_coefs(seed, early_stop)
    worst = 0.0
    for s in S_GRID:
        e = _far_exact(1.0, A, beta, s)
        worst = max(worst, float(abs(_D(ts.horner(fc, s)) - e) / e))
    return worst, seed[2]


def test_tau_is_not_the_simple_pole_figure():
    """The figure the headers quoted, rho^n / (1 - rho), is 16 times too small at the gate; tau(1/6, 16) is what the issue derived."""
    assert ts.TAU_FAR == pytest.approx(6.96e-12, rel=2e-3)
    assert (1.0 / 6.0) ** 16 / (1.0 - 1.0 / 6.0) < ts.TAU_FAR / 16


@pytest.mark.parametrize("A", A_GRID)
def test_far_series_at_the_gate(A):
    worst, q2 = _far_worst(A, ts.RHO_MAX2 * (1.0 - 1e-9))
    assert q2 <= ts.RHO_MAX2 and ts.n_terms(q2) == ts.NC
    print("A = %g: worst %.4e, tau %.4e" % (A, worst, ts.TAU_FAR))
    assert worst <= ts.TAU_FAR + ROUNDING


def test_the_gate_bound_is_reached_in_the_wing():
    """tau is sharp: deep in the wing the series errs by more than 0.99 tau -- and by 16 times the simple-pole figure, so this test
    and the previous one cannot both pass with rho^n / (1 - rho) in tau's place."""
    worst, _ = _far_worst(1e4, ts.RHO_MAX2 * (1.0 - 1e-9))
    assert 0.99 * ts.TAU_FAR <= worst <= ts.TAU_FAR + ROUNDING
    assert worst > 10 * (1.0 / 6.0) ** 16 / (1.0 - 1.0 / 6.0)


@pytest.mark.parametrize("thr,n", ts.EARLY_STOP)
@pytest.mark.parametrize("A", A_GRID)
def test_far_series_below_each_early_stop_threshold(A, thr, n):
    worst, q2 = _far_worst(A, thr * (1.0 - 1e-9))
    assert q2 <= thr and ts.n_terms(q2) == n
    bound = ts.tau(math.sqrt(thr), n)
    print("A = %g, q2 < %g (n = %d): worst %.4e, tau %.4e" % (A, thr, n, worst, bound))
    assert worst <= bound + ROUNDING
    assert bound <= ts.TAU_FAR   # an early stop never costs more than the gate itself: one tolerance serves the GPU test


@pytest.mark.parametrize("thr,n", ts.EARLY_STOP)
def test_above_a_threshold_the_longer_loop_runs(thr, n):
    worst, q2 = _far_worst(100.0, thr * (1.0 + 1e-9))
    assert ts.n_terms(q2) == n + 2
    assert worst <= ts.tau(math.sqrt(q2), n + 2) + ROUNDING


def _asym_worst(asym, A, side):
    gamma, xc = 2.0, 2000.0
    beta = math.sqrt(ts.RHO_MAX2_ASYM * (1.0 - 1e-9) * (A * A + 1.0))
    h = beta * gamma / 2.0
    nu = xc + side * A * gamma / 2.0
    seed = ts.far_seed(1.0, 2.0 * (nu - xc) / gamma, 2.0 * h / gamma)
    assert seed[2] <= ts.RHO_MAX2_ASYM
    P = ts.asym_poly(asym / nu, asym, (0.5 * gamma * asym / nu) ** 2, xc, h)
    co = ts.far_coefs_asym(seed, P)
    worst = 0.0
    for s in S_GRID:
        x = xc + h * s
        e = tr.component_exact(x, nu, 1.0, gamma, asym, nu)
        worst = max(worst, float(abs(_D(ts.horner(co, (x - xc) / h)) - e) / abs(e)))
    return worst


def test_asymmetric_far_series():
    """No closed form (tile_series.py): the worst error of the restatement over the issue's grid is measured here, TAU_ASYM is four times
    the recorded measurement, and the measurement must not have moved."""
    worst = max(_asym_worst(asym, A, side) for asym in (-100.0, -30.0, 5.0, 30.0, 100.0) for A in A_GRID for side in (1.0, -1.0))
    print("worst asymmetric far-series error: %.4e (recorded %.4e)" % (worst, ts.TAU_ASYM_MEASURED))
    assert worst == pytest.approx(ts.TAU_ASYM_MEASURED, rel=0.01)
    assert ts.TAU_ASYM == 4.0 * ts.TAU_ASYM_MEASURED
    assert _asym_worst(30.0, 0.0, 1.0) < 1e-14   # the headers' figure, 3.6e-15, holds at the tile's centre only


@pytest.mark.parametrize("p", (1.0, 2.0, 2.5, 3.5, 4.0, 6.0, 8.0))
@pytest.mark.parametrize("axc", (0.3, 1.0, 2.0, 5.0, 50.0))
def test_harvey_series_at_the_gate(p, axc):
    eps = ts.eps_at_gate(p)
    xc = 1000.0
    h = eps * xc
    tau_ = axc / (1e-3 * xc)
    assert tr.series_gate([1.0, tau_, p, 0.0], 1, xc, h * (1.0 - 1e-12))
    assert not tr.series_gate([1.0, tau_, p, 0.0], 1, xc, h * 1.001)
    f = ts.harvey_term_series(1.0, tau_, p, xc, h)
    worst = 0.0
    for s in S_GRID:
        x = xc + h * s
        e = tr.harvey_exact(x, 1.0, tau_, p)
        worst = max(worst, float(abs(_D(ts.horner(f, (x - xc) / h)) - e) / e))
    print("p = %g, a x_c = %g, eps = %.5f: worst %.3e, budget %.3e" % (p, axc, eps, worst, ts.HARVEY_BUDGET))
    assert worst <= ts.HARVEY_BUDGET


def test_old_gate_misses_the_budget_for_steep_exponents():
    """What the p-blind gate admitted: eps = 0.02 whatever the exponent.  p = 4 deep in the decline: 4e-12 of the term (the issue's table)."""
    xc, eps, p, axc = 1000.0, 0.02, 4.0, 5.0
    f = ts.harvey_term_series(1.0, axc / (1e-3 * xc), p, xc, eps * xc)
    e = tr.harvey_exact(xc * (1.0 - eps), 1.0, axc / (1e-3 * xc), p)
    err = float(abs(_D(ts.horner(f, -1.0)) - e) / e)
    assert 3e-12 < err < 6e-12
    assert not tr.series_gate([1.0, axc / (1e-3 * xc), p, 0.0], 1, xc, eps * xc)


def test_gate_constants_agree():
    assert (tr.EPS_MAX, tr.SERIES_BUDGET) == (ts.EPS_MAX, ts.SERIES_BUDGET)
    assert (tr.R2_FAR, tr.R2_FAR_ASYM) == (ts.RHO_MAX2, ts.RHO_MAX2_ASYM)
    # every BASELINE shape (p = 2, h / x_c <= 0.003) passes the new gate with five orders of magnitude to spare
    assert ts.binom_rising(2.0) * 0.003 ** 8 < 1e-5 * ts.SERIES_BUDGET

"""The rank-one step of the proposal factor (TAMCMC_OPT_FACTOR_REFRESH) on the host: tests/factor_update_reference.py against itself, the
host-only entry tamcmc_factor_rank_one_update (the arithmetic of both engines, csrc/factor_update.h) against it, the entry's refusals,
and option 14 in the public surface.  No GPU.

Laws `ar1` and `pairs` of tests/sampler_cases.py on errors spread over 0.05 .. 20 (one of them shrunk to 3e-5 by the law; `pairs` has
pivots at 2e-3 of their variance), sigma = 2.38^2 / n, eps2 = 1e-12; L is the exact factor of (Sigma + eps2 I) sigma rounded to double.
Gains 0.9, 0.1, 1e-4 with sigma' = sigma: beta2 = 1 - g, w = sqrt(g sigma) d, d once along the axis of the shrunk variable (two of its
standard deviations) and once dense (every variable between one and two of its own, alternating signs).

The largest |got - exact| / bound seen (bound: factor_update_reference's, K1 = n + 2, K2 = 6 n + 24, no input term) is printed when the
module ends; measured 0.068 (n = 3, pairs, g = 0.1, dense), 0.028 at n = 8 and 0.005 from n = 64 on: the bound is a worst case over the
signs of n terms.
"""
import os
import re
from decimal import Decimal

import numpy as np
import pytest

import factor_update_reference as F
import sampler_cases as C
import sampler_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 8, 9, 64, 65, 93)
GAINS = (0.9, 0.1, 1e-4)
WORST = {}


def _errors(n):
    return np.geomspace(0.05, 20.0, n)[np.random.default_rng(n).permutation(n)] if n > 1 else np.array([0.3])


def _case(n, name):
    """(Sigma, sigma, L double, errors as the law has them) -- the factor is the exact one, rounded."""
    cov = C.law(name, _errors(n))
    sigma = 2.38 ** 2 / n
    Lx = R.cholesky(R.matrix_to_factor(cov, C.EPS2, sigma))
    assert Lx is not None
    return cov, sigma, R.factor_float(Lx), np.sqrt(np.diag(cov))


def _deviations(n, D):
    axis = np.zeros(n)
    axis[C.small_index(n)] = 2.0 * D[C.small_index(n)]
    dense = D * (1.0 + 0.5 * np.cos(np.arange(n))) * np.where(np.arange(n) % 2, -1.0, 1.0)
    return (("axis", axis), ("dense", dense))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        r, what = max(WORST.values())
        print("\nlargest |got - exact| / bound of tamcmc_factor_rank_one_update: %.4f (%s)" % (r, what))
        for n in SIZES:
            print("  n = %3d: %.4f" % (n, max((v[0] for k, v in WORST.items() if k[0] == n), default=0.0)))


@pytest.mark.parametrize("n", (1, 2, 3, 8, 9, 21))
def test_reference_against_itself(n):
    """L' L'^T is the matrix to 45 digits; the closed form L G is the exact Cholesky factor; cholesky_exact is R.cholesky on doubles."""
    tiny = Decimal(10) ** -45
    for name in ("ar1", "pairs"):
        cov, sigma, L, D = _case(n, name)
        A = R.matrix_to_factor(cov, C.EPS2, sigma)
        La, Lb = R.cholesky(A), F.cholesky_exact([[R.dec(v) for v in row] for row in A])
        assert all(La[i][k] == Lb[i][k] for i in range(n) for k in range(i + 1))
        for g in GAINS:
            for wname, d in _deviations(n, D):
                w, beta2 = np.sqrt(g * sigma) * d, 1.0 - g
                M = F.matrix(L, w, beta2)
                upd = F.rank_one(L, w, beta2)
                cf = F.closed_form(L, w, beta2)
                with R._ctx():
                    for i in range(n):
                        for j in range(i + 1):
                            s = sum((upd.L[i][k] * upd.L[j][k] for k in range(j + 1)), R.ZERO)
                            assert abs(s - M[i][j]) <= tiny * max(abs(M[i][j]), (M[i][i] * M[j][j]).sqrt()), (name, g, wname, i, j)
                            assert abs(cf[i][j] - upd.L[i][j]) <= tiny * (M[i][i]).sqrt(), (name, g, wname, i, j)


def test_law_matrix():
    cov = C.law("ar1", _errors(3))
    M, rho = F.law_matrix(cov, 0.5, 1e-12, [0.25, 0.5])
    assert rho == Decimal("0.375")
    with R._ctx():
        assert M[1][1] == Decimal("0.5") * (R.dec(cov[1][1]) + R.dec(1e-12) * Decimal("0.375")) and M[0][2] == Decimal("0.5") * R.dec(cov[0][2])


@pytest.mark.parametrize("name", ("ar1", "pairs"))
@pytest.mark.parametrize("n", SIZES)
def test_host_rule_within_the_bound(pkg, n, name):
    cov, sigma, L, D = _case(n, name)
    for g in GAINS:
        for wname, d in _deviations(n, D):
            w, beta2 = np.sqrt(g * sigma) * d, 1.0 - g
            got = pkg.sampler.factor_rank_one_update(L, w, beta2)
            assert np.all(np.triu(got, 1) == 0.0) and np.all(np.diag(got) > 0)
            upd = F.rank_one(L, w, beta2)
            r = F.ratio(got, upd)
            what = "n %d %s g %g %s" % (n, name, g, wname)
            WORST[(n, name, g, wname)] = (r, what)
            assert r <= 1.0, what + ": ratio %.3g" % r


def test_refusals(pkg):
    OKAY = np.array([[2.0, 0.0], [1.0, 3.0]])
    w = np.array([0.5, -1.0])
    pkg.sampler.factor_rank_one_update(OKAY, w, 0.5)
    bad = [(OKAY, [np.nan, 0.0], 0.5), (OKAY, [np.inf, 0.0], 0.5), (OKAY, w, np.nan), (OKAY, w, np.inf), (OKAY, w, 0.0), (OKAY, w, -0.5),
           ([[2.0, 0.0], [np.nan, 3.0]], w, 0.5), ([[2.0, 0.0], [1.0, 0.0]], w, 0.5), ([[-2.0, 0.0], [1.0, 3.0]], w, 0.5),
           ([[2.0, 0.0], [1.0, np.inf]], w, 0.5), (OKAY, [1e200, 1e200], 0.5)]
    for L, ww, b2 in bad:
        with pytest.raises(pkg.TamcmcError) as e:
            pkg.sampler.factor_rank_one_update(np.array(L), np.array(ww, dtype=np.float64), b2)
        assert e.value.code == pkg.ERR_BAD_ARG, (L, ww, b2)
    # what is above the diagonal is not read
    up = OKAY.copy()
    up[0, 1] = np.nan
    assert np.array_equal(pkg.sampler.factor_rank_one_update(up, w, 0.5), pkg.sampler.factor_rank_one_update(OKAY, w, 0.5))


def test_option_14_in_the_public_surface(pkg):
    hip_h = open(os.path.join(ROOT, "include", "tamcmc_hip.h")).read()
    smp_h = open(os.path.join(ROOT, "include", "tamcmc_sampler.h")).read()
    assert re.search(r"#define\s+TAMCMC_OPT_FACTOR_REFRESH\s+14\b", hip_h)
    assert pkg.OPT_FACTOR_REFRESH == 14
    others = {int(m.group(1)) for m in re.finditer(r"#define\s+TAMCMC_OPT_(?!FACTOR_REFRESH)\w+\s+(\d+)\b", hip_h)}
    assert 14 not in others
    doc = hip_h[hip_h.index("TAMCMC_OPT_FACTOR_REFRESH"):]
    doc = doc[:doc.index("*/")]
    assert "0 (default) or 1" in doc and "2 ... 65536" in doc and "TAMCMC_ERR_BAD_ARG" in doc    # the value range, as the header states it
    for name in ("tamcmc_sampler_get_factor(", "tamcmc_factor_rank_one_update(", "TAMCMC_INFO_FACTOR_UPDATES 15", "TAMCMC_INFO_FACTOR_REFRESHES 16",
                 "TAMCMC_INFO_FACTOR_FORCED 17", "TAMCMC_SAMPLER_INFO_N 18"):
        assert name in smp_h, name
    assert hasattr(pkg.lib(), "tamcmc_sampler_get_factor") and hasattr(pkg.lib(), "tamcmc_factor_rank_one_update")
    assert hasattr(pkg.Sampler, "factor")

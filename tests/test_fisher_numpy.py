"""The yardstick of the Fisher-information tests (tests/fisher_numpy.py) and the chunk rule of tamcmc_hip_fisher, on the CPU.

At y = M0 the Hessian of p S, S = sum_i (y_i / M_i + ln M_i), IS the expected information F: d_j d_k S = sum_i [(2 y / M^3 - 1 / M^2) d_j M d_k M
+ (1 / M - y / M^2) d_j d_k M], whose second bracket vanishes at y = M and whose first is 1 / M^2.  So central second differences of the
long-double S (frozen windows, like F's rows) must reproduce fisher_central to their own Richardson figure."""
import os
import subprocess

import numpy as np
import pytest

import adjoint_numpy as an
import fisher_numpy as fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _hessian(pkg, star, y, base, h):
    """Central second differences of S at the star's parameters, every table with the base table's windows."""
    idx = np.asarray(star.index_to_relax)
    n = idx.size

    def S(shift):
        P = np.array(star.params, dtype=np.float64)
        for k, s in shift:
            P[idx[k]] = P[idx[k]] + s * h[k]
        M, _ = fn.frozen_rows(pkg, star, P, base)
        return np.sum((y / M).astype(LD)) + np.sum(np.log(M).astype(LD))

    S0 = S(())
    Sp = [S(((k, 1.0),)) for k in range(n)]
    Sm = [S(((k, -1.0),)) for k in range(n)]
    H = np.zeros((n, n))
    for j in range(n):
        H[j, j] = float((Sp[j] - 2 * S0 + Sm[j]) / (LD(h[j]) * LD(h[j])))
        for k in range(j + 1, n):
            v = S(((j, 1.0), (k, 1.0))) - S(((j, 1.0), (k, -1.0))) - S(((j, -1.0), (k, 1.0))) + S(((j, -1.0), (k, -1.0)))
            H[j, k] = H[k, j] = float(v / (4 * LD(h[j]) * LD(h[k])))
    return H


def test_fisher_is_the_hessian_at_the_model(built, pkg, synth):
    star = an.stars(synth)["c2"]
    idx = star.index_to_relax
    F, U, happ = fn.fisher_central(pkg, star, an.steps(star.params, idx))
    assert F.shape == (idx.size, idx.size) and np.array_equal(F, F.T) and np.all(np.diag(F) > 0)
    y, base = fn.frozen_rows(pkg, star, star.params)        # y = M0: the expectation of the data
    h = an.steps(star.params, idx, rel=1e-4)
    H1, H2 = _hessian(pkg, star, y, base, h), _hessian(pkg, star, y, base, 0.5 * h)
    sc = fn.scale(F)
    rich, diff = np.max(np.abs(H1 - H2) / sc), np.max(np.abs(H2 - F) / sc)
    print("\nHessian of S at y = M0 against F: |H(h/2) - F| %.2e, Richardson |H(h) - H(h/2)| %.2e of sqrt(F_jj F_kk)" % (diff, rich))
    assert rich < 0.2            # (the Hessian itself has converged: the comparison says something)
    assert diff <= 3 * rich


def test_bound_is_small_against_the_information(built, pkg, synth):
    """The derived device tolerance is far below what a wrong lane map, a missing block or an unfrozen window would cost (percent)."""
    star = an.stars(synth)["c2"]
    F, U, happ = fn.fisher_central(pkg, star, an.steps(star.params, star.index_to_relax))
    rel = fn.bound(U, happ, star.x.size) / fn.scale(F)
    assert np.max(rel) <= 5e-3 and np.median(rel) < 1e-5


# (chains, Nvars, Nx, budget in MiB) -> (chains per pass, passes)
CASES = [
    ((3, 21, 4000, 1), (1, 3)),              # C2 under a 1 MiB budget: 2 x 21 x 4000 x 8 B = 1 344 000 B per chain, one chain per pass
    ((3, 21, 4000, 2048), (3, 1)),
    ((20, 93, 100000, 2048), (14, 2)),       # the headline shape: 148.8 MB per chain, 14 fit 2 GiB
    ((1, 93, 100000, 10), (1, 1)),           # a single chain above the budget still runs alone
    ((5, 93, 100000, 300), (2, 3)),          # ragged last pass
    ((0, 93, 100000, 2048), (1, 0)),
]


def test_chunk_rule_with_the_fisher_budget(tmp_path):
    exe = str(tmp_path / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "fisher_chunk_driver.cpp")], check=True)
    args = [str(v) for case, _ in CASES for v in case]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    for (case, want), line in zip(CASES, out):
        chunk, passes, covered, per_chain = (int(v) for v in line.split())
        assert (chunk, passes) == want, (case, line)
        assert covered == case[0]
        assert per_chain == 2 * case[1] * case[2] * 8
        assert chunk == 1 or chunk * per_chain <= case[3] << 20
    assert out[len(CASES)] == "default_budget_mb 2048"


def test_seed_covariance_rule(built, pkg, synth):
    """E (I + E F E)^-1 E on the host, with the c2 star's F at T = 1 and T = 150, a variable with zero initial error and one without
    information: within 1e-9 e_j e_k of numpy's (the eigenvalues of I + E F E lie in [1, ~150]), symmetric, never wider than e^2."""
    from tamcmc_c_amd.sampler import default_errors, fisher_seed_covariance
    star = an.stars(synth)["c2"]
    F1, _, _ = fn.fisher_central(pkg, star, an.steps(star.params, star.index_to_relax))
    e = default_errors(star)
    e[3] = 0.0
    for T in (1.0, 150.0):
        F = F1 / T
        F[5, :] = 0.0
        F[:, 5] = 0.0
        cov = fisher_seed_covariance(F, e)
        ee = e[:, None] * e[None, :]
        A = np.eye(e.size) + ee * F
        ev = np.linalg.eigvalsh(A)
        print("\nT = %g: eigenvalues of I + E F E in [%.3f, %.1f]" % (T, ev[0], ev[-1]))
        assert ev[0] >= 1 - 1e-12
        assert np.all(np.abs(cov - ee * np.linalg.inv(A)) <= 1e-9 * ee)
        assert np.array_equal(cov, cov.T) and np.all(np.diag(cov) <= e * e)
        assert not cov[3].any() and cov[5, 5] == e[5] * e[5]
        assert np.min(np.diag(cov)[e > 0] / (e * e)[e > 0]) < (0.5 if T == 1.0 else 1.0)
    with pytest.raises(pkg.TamcmcError):
        fisher_seed_covariance(np.full((2, 2), np.nan), np.ones(2))

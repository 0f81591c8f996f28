"""Finite-difference gradient of the red-giant models (ids 25 / 27) through the device-built batch (csrc/fd_batch.hip): the perturbed
vectors' class-4 log-prior and scalar unpack in k_fd_rgb_perturb, their tables from the device pre-step, then the same likelihood
launches as every other model -- brute force (every arithmetic mode) or windowed (FAST modes: k_fd_compare's delta tables).

One small star for the whole file: 4000 bins, 4 radial orders, l = 0..3, period spacing 200 s -> 25 mixed modes (a likelihood tile holds
near and far rows), two Harvey profiles (what the synthetic red-giant builder makes)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_LOGL = {"strict": 1e-11, "fast": 1e-11}   # include/tamcmc_hip.h: red-giant tolerance (STRICT) / the FAST tolerance


def _small_star(synth, cte=False):
    star = synth.make_c5_star(nx=4000, nmax=4, dnu=20.0, nferr=4, cte_width=cte)
    o = np.cumsum([0] + list(star.plength))
    star.params[o[3] + 1] = 200.0                 # period spacing
    star.priors[:2, o[3] + 1] = [199.0, 201.0]
    return star, o


@pytest.fixture(scope="module")
def small(synth, oracle):
    star, o = _small_star(synth)
    st, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    assert st == 0
    star.set_spectrum_from_model(m0, 4)
    rc, modes = oracle.rgb_modes(star.params, star.plength, star.x[2] - star.x[1])
    assert rc == 0 and 10 <= len(modes["fl1"]) <= 40
    return star, o


@pytest.fixture(scope="module")
def ctxs(pkg, small):
    star, _ = small
    c = {"strict": pkg.HipContext(0, precision=pkg.PRECISION_STRICT), "fast": pkg.HipContext(0, precision=pkg.PRECISION_FAST, timing=True)}
    for v in c.values():
        v.set_spectrum(star.x, star.y)
    yield c
    for v in c.values():
        v.close()


def _steps(p, idx):
    return 1e-6 * np.maximum(np.abs(p[idx]), 1e-2)


def _batch(P, idx, h):
    """The (Nvars + 1) vectors per chain of a finite-difference batch and the steps actually applied."""
    P = np.atleast_2d(P)
    V = np.repeat(P[:, None, :], idx.size + 1, axis=1)
    for k, i in enumerate(idx):
        V[:, k + 1, i] = P[:, i] + h[k]
    happ = V[:, 1:, :][:, np.arange(idx.size), idx] - P[:, idx]
    return V, happ


def _every_block(star, o):
    """Indices covering every parameter block: heights, l=0 frequencies, the eight mixed-mode parameters, the bias values at the spline nodes,
    one l=2 and one l=3 frequency, splitting (envelope, core, a2, a3, asymmetry), width law, noise, inclination."""
    nferr = (star.plength[3] - 8) // 2
    return np.concatenate([np.arange(0, o[1]), np.arange(o[2], o[3]), np.arange(o[3], o[3] + 8), np.arange(o[3] + 8 + nferr, o[4]), [o[4], o[5]],
                           [o[6], o[6] + 1, o[6] + 2, o[6] + 4, o[6] + 9], np.arange(o[7], o[8]), np.arange(o[8], o[9]), [o[9]]]).astype(np.int32)


@pytest.fixture(scope="module")
def oracle_quotients(small, oracle):
    """Forward quotients of the oracle's red-giant log-likelihood (CPU, long double), chain at T = 1.3, every parameter block: computed once."""
    star, o = small
    idx = _every_block(star, o)
    h = _steps(star.params, idx)
    V, happ = _batch(star.params, idx, h)
    T = 1.3
    L, _, st = oracle.loglike_batch(star.model_id, V[0], star.plength, star.x, star.y, 1.0, np.full(idx.size + 1, T))
    assert (st == 0).all()
    return idx, h, T, L[0], (L[1:] - L[0]) / happ[0]


def test_gradient_entries_accept_the_red_giant_ids(pkg, synth, small, ctxs):
    """Fails without the feature: ids 25 and 27 used to end in TamcmcError(TAMCMC_ERR_BAD_MODEL)."""
    star, _ = small
    idx = star.index_to_relax
    l0, g = ctxs["fast"].fd_gradient(25, np.tile(star.params, (2, 1)), star.plength, idx, _steps(star.params, idx), [1.0, 2.0])
    assert l0.shape == (2,) and g.shape == (2, idx.size) and np.isfinite(l0).all() and np.isfinite(g).all()
    s27, _ = _small_star(synth, cte=True)
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    c.set_spectrum(s27.x, np.ones_like(s27.x))
    idx = s27.index_to_relax
    l0, g = c.fd_gradient(27, s27.params, s27.plength, idx, _steps(s27.params, idx))
    l0p, pr0, gp = c.fd_gradient_posterior(s27, s27.params, _steps(s27.params, idx))
    c.close()
    assert g.shape == (1, idx.size) and np.isfinite(l0).all() and np.isfinite(g).all()
    assert np.isfinite(pr0).all() and np.isfinite(gp).all() and l0p[0] == l0[0]
    s27.prior_class = 2                                # io_asymptotic (4) is the red giants' prior class, and the only one
    with pytest.raises(pkg.TamcmcError) as e:
        ctxs["fast"].fd_gradient_posterior(s27, s27.params, _steps(s27.params, idx))
    assert e.value.code == pkg.ERR_BAD_MODEL


def test_strict_brute_force_equals_two_evaluations(pkg, small, ctxs):
    """STRICT: grad[c, k] = (logL(theta_c + h e_k) - logL(theta_c)) / h_applied with both terms from loglike_params_batch on the same vectors,
    three chains at three temperatures, all free parameters.  Exact equality: a vector's logL does not depend on its batch."""
    star, _ = small
    idx = star.index_to_relax
    rng = np.random.default_rng(11)
    P = np.tile(star.params, (3, 1))
    P[1:, idx] *= 1 + 0.002 * rng.standard_normal((2, idx.size))
    T = np.array([1.0, 1.5, 2.25])
    h = _steps(star.params, idx)
    c = ctxs["strict"]
    l0, g = c.fd_gradient(star.model_id, P, star.plength, idx, h, T)
    V, happ = _batch(P, idx, h)
    L, _, st = c.loglike_params_batch(star.model_id, V.reshape(-1, P.shape[1]), star.plength, np.repeat(T, idx.size + 1))
    assert (st == 0).all()
    L = L.reshape(3, idx.size + 1)
    want = (L[:, 1:] - L[:, :1]) / happ
    print("\nSTRICT gradient vs two evaluations: max |dlogL0| %.3e, max |dgrad| %.3e (gradient scale %.3e)"
          % (np.max(np.abs(l0 - L[:, 0])), np.max(np.abs(g - want)), np.max(np.abs(want))))
    assert np.array_equal(l0, L[:, 0])
    assert np.array_equal(g, want)


@pytest.mark.parametrize("mode", ["strict", "fast"])
def test_gradient_against_the_oracle(small, ctxs, oracle_quotients, mode):
    """|dgrad| <= 2 tol_logL |logL| / h: each of the two log-likelihoods of a quotient is within the stated red-giant tolerance of the oracle's."""
    star, _ = small
    idx, h, T, L0, want = oracle_quotients
    l0, g = ctxs[mode].fd_gradient(star.model_id, star.params, star.plength, idx, h, [T])
    _, happ = _batch(star.params, idx, h)
    bound = 2 * TOL_LOGL[mode] * abs(L0) / np.abs(happ[0])
    print("\n%s gradient vs oracle: max |dgrad| / bound %.3e" % (mode, np.max(np.abs(g[0] - want) / bound)))
    assert abs(l0[0] - L0) <= TOL_LOGL[mode] * abs(L0)
    assert np.all(np.abs(g[0] - want) <= bound)
    assert np.count_nonzero(g[0]) >= idx.size - 3      # (the two unused slots of the l=1 block move nothing)


def _windowed_and_brute(pkg, c, star, P, idx, h, T):
    c.set_option(pkg.OPT_FD_WINDOWED, 0)
    l0_f, g_f = c.fd_gradient(star.model_id, P, star.plength, idx, h, T)
    c.set_option(pkg.OPT_FD_WINDOWED, 1)
    c.reset_kernel_stats()
    l0_w, g_w = c.fd_gradient(star.model_id, P, star.plength, idx, h, T)
    assert np.allclose(l0_w, l0_f, rtol=1e-12)
    scale = np.max(np.abs(g_f), axis=1, keepdims=True)
    # the brute-force difference of two ~Nx-term sums carries ~1e-15 Nx / h of cancellation noise; the windowed one does not
    tol = 5e-15 * star.x.size / h[None, :] + 1e-6 * scale
    print("\nwindowed vs brute force: max |dgrad| / tol %.3e" % np.max(np.abs(g_w - g_f) / tol))
    assert np.all(np.abs(g_w - g_f) <= tol)
    return g_w, g_f


def test_windowed_equals_brute_force(pkg, small, ctxs):
    star, o = small
    c = ctxs["fast"]
    idx = star.index_to_relax
    rng = np.random.default_rng(12)
    P = np.tile(star.params, (2, 1))
    P[1, idx] *= 1 + 0.002 * rng.standard_normal(idx.size)
    T = np.array([1.0, 1.7])
    h = _steps(star.params, idx)
    _windowed_and_brute(pkg, c, star, P, idx, h, T)
    assert c.fd_stats()[1] > 0
    # which perturbations end as whole tables: the envelope rotation and the period spacing move every mixed mode; the white noise and an
    # l=0 height move no row / one row
    for i, full in ((o[6], True), (o[3] + 1, True), (o[9] - 1, False), (0, False)):
        one = np.array([i], dtype=np.int32)
        c.reset_kernel_stats()
        c.fd_gradient(star.model_id, P, star.plength, one, _steps(star.params, one), T)
        assert c.fd_stats()[1] > 0
        assert (c.fd_full_tables() > 0) == full, (i, c.fd_full_tables())


def test_perturbation_that_changes_the_mode_count(pkg, oracle, small, ctxs):
    """A step on the period spacing across a value where a mixed mode leaves the solver's set (found with the oracle): the two tables differ in
    length, every row after the first difference differs."""
    star, o = small
    k = o[3] + 1
    p = star.params.copy()
    p[k] = 199.95987434979568 - 1e-5
    one, h = np.array([k], dtype=np.int32), np.array([2e-5])
    V, happ = _batch(p, one, h)
    step = star.x[2] - star.x[1]
    n_o = [len(oracle.rgb_modes(v, star.plength, step)[1]["fl1"]) for v in V[0]]
    n_d = [ctxs["fast"].rgb_mixed_modes(star.model_id, v, star.plength)[0].size for v in V[0]]
    assert n_o[0] != n_o[1] and n_d == n_o, (n_o, n_d)
    g_w, g_f = _windowed_and_brute(pkg, ctxs["fast"], star, p, one, h, [1.0])
    L, _, st = oracle.loglike_batch(star.model_id, V[0], star.plength, star.x, star.y, 1.0, None)
    assert (st == 0).all()
    want = (L[1] - L[0]) / happ[0, 0]
    for name, g in (("windowed", g_w), ("brute force", g_f)):
        bound = 2 * TOL_LOGL["fast"] * abs(L[0]) / abs(happ[0, 0])
        print("\n%s vs oracle across a mode-count change: |dgrad| / bound %.3e (gradient %.3e)" % (name, abs(g[0, 0] - want) / bound, want))
        assert abs(g[0, 0] - want) <= bound, name


def test_prior_share_of_class_4(pkg, small, ctxs):
    from tamcmc_c_amd.sampler import log_prior
    star, o = small
    idx = star.index_to_relax
    h = 1e-7 * np.maximum(np.abs(star.params[idx]), 1e-3)
    k_inc = int(np.flatnonzero(idx == o[9])[0])
    P = np.tile(star.params, (3, 1))
    P[1, o[9]] = 90.0 - 0.25 * h[k_inc]                # forward point beyond the upper edge of the inclination's uniform prior
    P[2, o[1]] = -1.5                                  # a negative visibility: the base point violates a constraint
    c = ctxs["fast"]
    l0, pr0, g = c.fd_gradient_posterior(star, P, h, [1.0, 1.4, 2.0])
    gp = c.last_grad_prior
    assert pr0[2] == -np.inf and np.isfinite(l0).all() and np.isfinite(g).all() and np.all(gp[2] == 0)
    V, happ = _batch(P, idx, h)
    for ch in (0, 1):
        lp = np.array([log_prior(star, v)[0] for v in V[ch]])
        assert abs(pr0[ch] - lp[0]) <= 1e-12 * abs(lp[0])
        for k in range(idx.size):
            if np.isfinite(lp[k + 1]):
                want, scale = (lp[k + 1] - lp[0]) / happ[ch, k], max(abs(lp[k + 1]), abs(lp[0]))
            else:                                          # backward difference
                back = P[ch].copy()
                back[idx[k]] -= h[k]
                lb = log_prior(star, back)[0]
                assert ch == 1 and k == k_inc and np.isfinite(lb)
                want, scale = (lp[0] - lb) / happ[ch, k], max(abs(lb), abs(lp[0]))
            # device double against the host's long double: each log-prior within a few Np eps of the other, 1e-12 of the term's scale
            assert np.isfinite(gp[ch, k]) and abs(gp[ch, k] - want) <= 1e-12 * scale / abs(happ[ch, k]), (ch, k, gp[ch, k], want)


def test_failed_prestep_of_one_perturbed_vector(pkg, small, ctxs):
    """The last radial mode pulled below the first: the fit of the l=0 ladder gives a negative large separation and the table builder refuses
    the vector (the condition tests/test_gpu_rgb.py provokes).  That component is NaN, the other one is what it is alone."""
    star, o = small
    c = ctxs["fast"]
    idx = np.array([o[3] - 1, 0], dtype=np.int32)
    h = np.array([-80.0, 1e-5])
    p = np.ascontiguousarray(star.params)
    pl = np.ascontiguousarray(star.plength, dtype=np.int32)
    l0, g = np.zeros(1), np.zeros((1, 2))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = pkg.lib().tamcmc_hip_fd_gradient(c._h, star.model_id, 1, p.ctypes.data_as(dp), p.size, pl.ctypes.data_as(ip), idx.ctypes.data_as(ip), 2,
                                          h.ctypes.data_as(dp), None, 1.0, l0.ctypes.data_as(dp), g.ctypes.data_as(dp))
    assert rc == pkg.ERR_BAD_ARG
    _, g1 = c.fd_gradient(star.model_id, p, pl, idx[1:], h[1:])
    assert np.isfinite(l0[0]) and np.isnan(g[0, 0]) and np.isfinite(g[0, 1]) and g[0, 1] == g1[0, 0]


def test_host_engine_langevin_sampler(pkg, small, ctxs):
    """Host-driven engine with the Langevin drift on id 25.  The gradient the sampler holds for a chain equals the direct call on the
    chain's position: bit for bit while no swap has moved it (a vector's logL and prior do not depend on the batch); a gradient that
    followed its position through a parallel-tempering swap had its likelihood share (held as grad - grad_prior) re-tempered by
    T_old / T_new -- a subtraction, a multiplication, a division and an addition, each within half an ulp of |grad| + |grad_prior|, at
    most once per iteration: 4 * 30 * 2^-53 of that scale bounds it."""
    star, _ = small
    c = ctxs["fast"]
    n, T = 30, np.array([math.pow(1.6, m) for m in range(3)])   # the engine's ladder: C pow(lambda, m), not numpy's x * x for m = 2
    kw = dict(nchains=3, lambda_temp=1.6, use_drift=1, seed=5, engine="host", Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,))

    def held_and_direct(s):
        g, gp, valid = s.gradient()
        held = np.tile(star.params, (3, 1))
        held[:, star.index_to_relax] = s.state()["vars"]
        h = 1e-7 * np.maximum(np.abs(s.get_proposal(0)[0]), 1e-3)     # the engine's steps: fd_step_rel max(|mu_0|, 1e-3)
        _, _, g_direct = c.fd_gradient_posterior(star, held, h, T)
        assert valid.any()
        return g, g_direct, c.last_grad_prior.copy(), np.flatnonzero(valid)

    s = pkg.Sampler(c, star, **kw)
    smp, stat = s.run(n, stats=True)
    assert np.isfinite(stat).all() and np.isfinite(smp).all()
    assert s.state()["accepted0"] > 0                  # at least one accepted move in the coldest chain (a swap does not count)
    g, g_direct, gp_direct, valid = held_and_direct(s)
    for m in valid:
        bound = 4 * n * 2.0 ** -53 * (np.abs(g_direct[m]) + np.abs(gp_direct[m]))
        print("\nchain %d: held vs direct gradient, max |d| / bound %.3e" % (m, np.max(np.abs(g[m] - g_direct[m]) / np.maximum(bound, 1e-300))))
        assert np.all(np.abs(g[m] - g_direct[m]) <= bound), m
    s2 = pkg.Sampler(c, star, **kw)
    smp2, stat2 = s2.run(n, stats=True)
    assert np.array_equal(smp2, smp) and np.array_equal(stat2, stat)
    s.close(); s2.close()
    s3 = pkg.Sampler(c, star, **dict(kw, dN_mixing=10**6))   # no swap within the run: nothing is re-tempered
    s3.run(n)
    assert s3.state()["swap_attempts"] == 0
    g, g_direct, _, valid = held_and_direct(s3)
    for m in valid:
        assert np.array_equal(g[m], g_direct[m]), m
    s3.close()
    with pytest.raises(pkg.TamcmcError) as e:
        pkg.Sampler(c, star, **dict(kw, engine="device"))
    assert e.value.code == pkg.ERR_BAD_MODEL


def test_existing_models_twice_bit_for_bit(pkg, oracle, synth):
    """Id 23 through the comparison kernel, windowed: the same call twice gives the same bits (the delta rows are stored in table order)."""
    star = synth.make_c3_star(nx=20000, step=0.1)
    _, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    y = star.set_spectrum_from_model(m0, 1)
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    c.set_spectrum(star.x, y)
    idx = star.index_to_relax
    P = np.tile(star.params, (2, 1))
    P[1, idx] *= 1 + 0.002 * np.random.default_rng(3).standard_normal(idx.size)
    h = _steps(star.params, idx)
    a = c.fd_gradient(star.model_id, P, star.plength, idx, h, [1.0, 1.3])
    b = c.fd_gradient(star.model_id, P, star.plength, idx, h, [1.0, 1.3])
    c.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

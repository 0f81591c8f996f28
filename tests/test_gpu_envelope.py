"""Gaussian-envelope background fits on the GPU (model ids 0 = model_Kallinger2014_Gaussian, 1 = model_Harvey_Gaussian; csrc/envelope.hip)
against the long-double restatement tests/envelope_numpy.py: model rows and logL within the stated 1e-12 (include/tamcmc_hip.h) on
synthetic stars and on the real 1161491 spectrum, bit-identical logL at any batch position and size, the brute-force gradient of the
log-posterior, the host-driven sampler's bookkeeping, examples/fit_star's `simple` dialect, and posterior recovery (MH and Langevin)."""
import os
import subprocess

import numpy as np
import pytest

import envelope_numpy as en
from mc_stats import compare_chains, mc_error_of_mean

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "envelope")
TOL = 1e-12


@pytest.fixture(scope="module")
def mods(pkg):
    from tamcmc_c_amd import inputs, sampler, synth
    return pkg, inputs, sampler, synth


def _synthetic(synth, model_id, nx=5400, seed=1, x0_zero=False):
    star = synth.make_envelope_star(model_id, nx=nx, seed=seed)
    if x0_zero:
        star.x = star.x - star.x[0]
    m = np.asarray(en.model(model_id, star.params, star.x), dtype=np.float64)
    star.set_spectrum_from_model(m, seed=seed + 100)
    return star


def _real_1161491(inputs):
    star, _ = inputs.load_simple_star(os.path.join(GOLD, "1161491_Gaussfit.model"), os.path.join(GOLD, "1161491_Gaussfit.data"), 1)
    return star


def _perturbed(star, B, seed):
    rng = np.random.default_rng(seed)
    P = np.tile(star.params, (B, 1))
    free = star.relax == 1
    P[1:, free] *= 1.0 + 0.03 * rng.standard_normal((B - 1, int(free.sum())))
    return P


def _check_batch(pkg, star, model_id, P, T=None, p=1.0):
    ctx = pkg.HipContext(0)
    try:
        ctx.set_spectrum(star.x, star.y)
        got, rows, status = ctx.loglike_params_batch(model_id, P, star.plength, Tcoefs=T, p=p, want_model=True)
    finally:
        ctx.close()
    assert (status == 0).all()
    for b in range(P.shape[0]):
        ref, mref = en.loglike(model_id, P[b], star.x, star.y, p=p, T=1.0 if T is None else T[b])
        mref = np.asarray(mref, dtype=np.float64)
        dm = np.max(np.abs(rows[b] - mref) / mref)
        assert dm <= TOL, (b, dm)
        assert abs(got[b] - ref) <= TOL * abs(ref), (b, got[b], ref)
    return got


@pytest.mark.parametrize("model_id", [0, 1])
@pytest.mark.parametrize("B", [1, 7, 64])
def test_synthetic_rows_and_logl(mods, model_id, B):
    pkg, _, _, synth = mods
    star = _synthetic(synth, model_id, seed=11 + model_id)
    T = 1.7 ** np.arange(B)
    _check_batch(pkg, star, model_id, _perturbed(star, B, seed=B), T=T, p=1.0)


@pytest.mark.parametrize("B", [1, 7, 64])
def test_real_1161491_harvey_gaussian(mods, B):
    pkg, inputs, _, _ = mods
    star = _real_1161491(inputs)
    _check_batch(pkg, star, 1, _perturbed(star, B, seed=100 + B))


@pytest.mark.parametrize("B", [1, 7, 64])
def test_real_1161491_kallinger_gaussian(mods, B):
    """The Kallinger model on the real, irregular 1161491 grid (h = x(1) - x(0) differs from the later steps)."""
    pkg, inputs, _, synth = mods
    real = _real_1161491(inputs)
    star = synth.make_envelope_star(0, nx=64, seed=5)
    star.params[15], star.params[16], star.params[14] = 52.0, 16.7, 3000.0
    star.x, star.y = real.x, real.y
    _check_batch(pkg, star, 0, _perturbed(star, B, seed=200 + B))


def test_inactive_harvey_term_and_edge_cases(mods):
    pkg, _, _, synth = mods
    star = _synthetic(synth, 1, nx=3000, seed=21)
    P = np.tile(star.params, (4, 1))
    P[1, 4] = 0.0            # second Harvey term: |tc| = 0 -> skipped
    P[2, 1] = 0.0            # first one skipped
    P[3, [2, 5]] = 0.0       # exponents 0: (a x)^0 = 1
    _check_batch(pkg, star, 1, P)


@pytest.mark.parametrize("model_id", [0, 1])
def test_first_bin_at_zero(mods, model_id):
    """A spectrum whose first bin is x = 0: eta^2[0] = 1 (id 0), (1e-3 tc 0)^p = 0 (id 1)."""
    pkg, _, _, synth = mods
    star = _synthetic(synth, model_id, nx=2048, seed=31, x0_zero=True)
    assert star.x[0] == 0.0
    _check_batch(pkg, star, model_id, _perturbed(star, 7, seed=3))


@pytest.mark.parametrize("model_id", [0, 1])
def test_logl_bit_identical_across_batches(mods, model_id):
    pkg, _, _, synth = mods
    star = _synthetic(synth, model_id, nx=20000, seed=41)
    P = _perturbed(star, 64, seed=9)
    ctx = pkg.HipContext(0)
    try:
        ctx.set_spectrum(star.x, star.y)
        full, _, _ = ctx.loglike_params_batch(model_id, P, star.plength)
        rev, _, _ = ctx.loglike_params_batch(model_id, P[::-1].copy(), star.plength)
        np.testing.assert_array_equal(rev[::-1], full)
        for b in (0, 5, 63):
            one, _, _ = ctx.loglike_params_batch(model_id, P[b], star.plength)
            assert one[0] == full[b]
            mid, _, _ = ctx.loglike_params_batch(model_id, np.vstack([P[(b + 1) % 64], P[b], P[(b + 2) % 64]] * 2 + [P[b]]), star.plength)
            assert mid[1] == full[b] and mid[6] == full[b]
    finally:
        ctx.close()


def test_no_mode_table(mods):
    pkg, _, _, synth = mods
    star = synth.make_envelope_star(1, nx=64)
    for mid in (0, 1):
        st = pkg.build_mode_table(mid, star.params, np.zeros(11, dtype=np.int32), star.x)[0]
        assert st == pkg.ERR_BAD_MODEL


# ---------------------------------------------------------------- gradient
@pytest.mark.parametrize("model_id", [0, 1])
def test_fd_gradient_posterior(mods, model_id):
    pkg, _, sampler, synth = mods
    star = _synthetic(synth, model_id, nx=5400, seed=51)
    P = _perturbed(star, 3, seed=52)
    idx = star.index_to_relax
    h = 1e-4 * np.maximum(np.abs(star.params[idx]), 1e-3)
    T = np.array([1.0, 2.5, 7.0])
    ctx = pkg.HipContext(0)
    try:
        ctx.set_spectrum(star.x, star.y)
        l0, pr0, g = ctx.fd_gradient_posterior(star, P, h, Tcoefs=T)
        l0b, gl = ctx.fd_gradient(model_id, P, star.plength, idx, h, Tcoefs=T)
    finally:
        ctx.close()
    np.testing.assert_array_equal(l0b, l0)
    for c in range(P.shape[0]):
        L0, _ = en.loglike(model_id, P[c], star.x, star.y, T=T[c])
        assert abs(l0[c] - L0) <= TOL * abs(L0)
        Pr0 = en.log_prior(star.prior_class, P[c], star.priors, star.priors_switch)
        assert abs(pr0[c] - Pr0) <= 1e-12 * max(1.0, abs(Pr0))
        for k, i in enumerate(idx):
            q = P[c].copy()
            q[i] = P[c, i] + h[k]
            happ = q[i] - P[c, i]
            Lk, _ = en.loglike(model_id, q, star.x, star.y, T=T[c])
            gref_l = (Lk - L0) / happ
            Prk = en.log_prior(star.prior_class, q, star.priors, star.priors_switch)
            gref = gref_l + ((Prk - Pr0) / happ if np.isfinite(Prk) else 0.0)
            # noise of the difference of two evaluations, each within the stated tolerance, plus the prior's double arithmetic
            tol = 2 * TOL * abs(L0) / happ + 1e-9 * abs(gref) + 1e-9
            assert abs(gl[c, k] - gref_l) <= tol, (c, k, gl[c, k], gref_l, tol)
            assert abs(g[c, k] - gref) <= tol, (c, k, g[c, k], gref, tol)


# ---------------------------------------------------------------- sampler
def test_sampler_bookkeeping_1161491(mods):
    pkg, inputs, sampler, _ = mods
    star = _real_1161491(inputs)
    ctx = pkg.HipContext(0)
    try:
        ctx.set_spectrum(star.x, star.y)
        s = sampler.Sampler(ctx, star, nchains=4, lambda_temp=1.5, seed=7, Nt_learn=(50, 100, 300), periods_learn=(1, 5))
        s.run(400, record=False)
        st = s.state()
        assert st["iteration"] == 400 and st["accepted0"] > 0
        T = 1.5 ** np.arange(4)
        for m in range(4):
            p = star.params.copy()
            p[star.index_to_relax] = st["vars"][m]
            L, _ = en.loglike(1, p, star.x, star.y, T=T[m])
            assert abs(st["logL"][m] - L) <= TOL * abs(L), (m, st["logL"][m], L)
            Pr = en.log_prior(1, p, star.priors, star.priors_switch)
            assert abs(st["logPrior"][m] - Pr) <= 1e-15 * max(1.0, abs(Pr)), (m, st["logPrior"][m], Pr)
        s.close()
        with pytest.raises(pkg.TamcmcError) as e:
            sampler.Sampler(ctx, star, nchains=4, engine="device")
        assert e.value.code == pkg.ERR_BAD_MODEL
    finally:
        ctx.close()


def test_fit_star_simple(pkg, tmp_path):
    exe = os.path.join(ROOT, "examples", "fit_star")
    cfg = tmp_path / "gauss.cfg"
    src = open(os.path.join(HERE, "golden", "sampler_test.cfg")).read()
    src = src.replace("prior_fct_name=io_local;", "prior_fct_name=priors_Harvey_Gaussian;")
    src = src.replace("model_fct_name=io_local;", "model_fct_name=model_Harvey_Gaussian;")
    src = src.replace("Nt_learn=200, 600, 4000;", "Nt_learn=50, 100, 300;")
    cfg.write_text(src)
    root = str(tmp_path / "1161491_Gaussfit_")
    r = subprocess.run([exe, "simple", os.path.join(GOLD, "1161491_Gaussfit.model"), os.path.join(GOLD, "1161491_Gaussfit.data"), str(cfg),
                        os.path.join(HERE, "golden", "errors_test.cfg"), root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "model_Harvey_Gaussian (id 1)" in r.stdout
    for f in ("params.hdr", "params_chain-0.bin", "stat_criteria.hdr", "stat_criteria.bin", "restore_1.dat", "restore_2.dat",
              "restore_3.dat", "evidence.txt"):
        assert os.path.exists(root + f), f
    hdr = open(root + "params.hdr").read()
    assert "H1" in hdr and "Gauss_sigma" in hdr
    nv = 9
    raw = np.fromfile(root + "params_chain-0.bin", dtype=np.float64)
    assert raw.size == 150 * nv and np.isfinite(raw).all()


# ---------------------------------------------------------------- posterior
def _posterior(pkg, sampler, star, use_drift, n, seed):
    ctx = pkg.HipContext(0)
    try:
        ctx.set_spectrum(star.x, star.y)
        s = sampler.Sampler(ctx, star, nchains=4, lambda_temp=1.5, seed=seed, use_drift=use_drift, Nt_learn=(200, 1000, 3000),
                            periods_learn=(1, 5))
        s.run(3000, record=False)
        smp, _ = s.run(n, record=True)
        s.close()
    finally:
        ctx.close()
    return smp[:, 0, :]


@pytest.mark.parametrize("model_id", [0, 1])
def test_posterior_recovers_injection_mh_vs_langevin(mods, model_id):
    pkg, _, sampler, synth = mods
    star = _synthetic(synth, model_id, nx=5400, seed=61 + model_id)
    truth = star.params[star.index_to_relax].copy()
    mh = _posterior(pkg, sampler, star, 0, 12000, seed=3)
    names = [star.names[i] for i in star.index_to_relax]
    for nm in ("numax", "Amax", "Gauss_sigma"):
        k = names.index(nm)
        mean, sd = mh[:, k].mean(), mh[:, k].std()
        err = mc_error_of_mean(mh[:, k])
        # the posterior of one noise realisation sits within a few posterior widths of the injection
        assert abs(mean - truth[k]) <= 4.0 * sd + 4.0 * err, (nm, mean, sd, err, truth[k])
    lg = _posterior(pkg, sampler, star, 1, 6000, seed=4)
    zm, zv, ea, eb = compare_chains(mh, lg)
    assert np.all(np.abs(zm) < 5.0), (zm, ea, eb)
    assert np.all(np.abs(zv) < 5.0), (zv, ea, eb)

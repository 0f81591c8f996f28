"""The sampler's own algebra on both engines against the 50-digit reference (tests/sampler_reference.py), -m gpu.

Every test replays single-iteration run(1) calls of a three-chain sampler (lambda = 1.5, FAST arithmetic) at the sizes and under the
directed proposal laws of tests/sampler_cases.py.  The reference is fed the PRODUCT's own inputs of the iteration -- positions, held
gradients, proposal law, log-posteriors -- so no finite-difference noise enters: what is compared is the linear algebra, and every
comparison is |got - ref| <= K 2^-52 scale with the scale the reference computes from the same inputs (sampler_reference.py lists them).

    test_proposal_settled       x' = x + d + L z with z from the reference's own Philox / Box-Muller; draws() against that z
    test_langevin_test          Pmove and the accept flag (host engine: the pair of proposal log-densities too), delta = 0 and 30
    test_adaptation             mu, cov, sigma element by element after a Robbins-Monro step at gain c0 / 51, then the NEXT proposal against
                                the exact factor of the product's own new matrix: the engine's Cholesky and its L z, isolated
    test_indefinite_update_keeps_the_factor     gain 10 / 3: the updated matrix is not positive definite, the old factor proposes
    test_swap_carries_the_gradient              accepted and refused swaps, both rules: exchanged statistics, re-tempered gradient

K = max(4, 4 r), r the worst ratio seen on the MI355X over all sizes and laws (the convention of tests/test_gpu_priors.py); the module
prints the r of its run when it ends.  Measured r (host | device) and the K in force are in the table K below (the device engine keeps
its log-densities on the device: no K).  Caps hold whatever K says: a ratio above 2 Nv for a proposal or an update is a bug, not a
tolerance.

Conditions of test_langevin_test, asserted on the host engine for every size and delta: at least half of the checked chain-iterations
have 1e-6 < r_ref < 1 (measured: 9 to 17 of 18); where r_ref >= 1 the engine reports exactly 1.0 unless the exponent lies within the
tolerance of 0; with delta = 30 a chain is truncated; an accept flag is left uncompared only when |u - r_ref| is below the tolerance on
r, at most once per case (measured: never).  The proposal law is set BEFORE the state: both engines draw the next proposal under the
new law.

Mutations of the device kernels, each built and run once against this module (none is committed), and what fails:
    acc += epsi2 * g[i] dropped from mala_drift       test_proposal_settled, test_langevin_test, test_adaptation, test_indefinite_... (every size)
    hi > k -> hi >= k in the one-wave solve            test_langevin_test[65]
    k <= kend -> k < kend in trailing's tail           test_adaptation[9, 65, 129]
    deviation from the old mu in adapt_chain_as        test_adaptation, test_indefinite_update_keeps_the_factor
    tr inverted in k_mala_settle                       test_swap_carries_the_gradient
    delta / nrm -> delta / n2                          test_langevin_test[delta = 30]
    LT written when pd is false                        test_indefinite_update_keeps_the_factor
"""
import math
from decimal import Decimal

import numpy as np
import pytest

import sampler_cases as C
import sampler_reference as R

pytestmark = pytest.mark.gpu

ENGINES = ("host", "device")
SEED = 20240917
FD_REL = 1e-7
K_Z = 4 * 3.2          # tests/test_rng.py
# quantity -> (K host, K device) = max(4, 4 r); r as measured on the MI355X, over every size and law (host | device):
#   proposal 7.36 | 7.26   proposal_adapted 1.51 | 1.14   lq 4.64 | -   ln_r 0.07 | 0.11   mu 0.62 | 0.57   cov 1.80 | 1.80
#   sigma 0.48 | 1.04   swap_stats 0.32 | 0.57   carried_gradient 0.97 | 1.03
K = {"proposal": (29.5, 29.1), "proposal_adapted": (6.1, 4.6), "lq": (18.6, None), "ln_r": (4.0, 4.0), "mu": (4.0, 4.0),
     "cov": (7.2, 7.2), "sigma": (4.0, 4.2), "swap_stats": (4.0, 4.0), "carried_gradient": (4.0, 4.2)}
WORST = {}


def _hold(name, engine, ratio, cap=None, what=""):
    """Records the ratio, asserts it against K (when measured) and against the cap."""
    key = (name, engine)
    if ratio > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (ratio, what)
    k = K[name][ENGINES.index(engine)]
    assert math.isfinite(ratio), (name, engine, what)
    if cap is not None:
        assert ratio <= cap, "%s (%s) %s: ratio %.3g above the cap %.3g" % (name, engine, what, ratio, cap)
    if k is not None:
        assert ratio <= k, "%s (%s) %s: ratio %.3g above K = %.3g" % (name, engine, what, ratio, k)


@pytest.fixture(scope="module")
def stars(pkg, oracle, synth):
    cache = {}

    def get(nv):
        if nv not in cache:
            star = C.build_star(oracle, synth, nv)
            ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
            ctx.set_spectrum(star.x, star.y)
            cache[nv] = (star, ctx)
        return cache[nv]

    yield get
    for _, ctx in cache.values():
        ctx.close()
    print("\nworst ratios |got - ref| / (2^-52 scale) over all sizes and laws:")
    for (name, engine), (r, what) in sorted(WORST.items()):
        print("  %-18s %-6s r = %8.3f   4 r = %8.2f   (%s)" % (name, engine, r, 4 * r, what))


def _sampler(pkg, ctx, star, engine, **kw):
    args = dict(nchains=C.NCH, lambda_temp=C.LAM, engine=engine, use_drift=1, seed=SEED, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,),
                dN_mixing=10**6, c0=2.0, fd_step_rel=FD_REL, delta=0.0, epsilon2=C.EPS2)
    args.update(kw)
    return pkg.Sampler(ctx, star, **args)


def _set_law(pkg, s, star, name, mu=None, factor=1.0):
    """Sigma = D R D for every chain, sigma_m = factor x the sampler's initial 2.38^2 T_m^0.2 / Nv."""
    cov = C.law(name, pkg.sampler.default_errors(star))
    sig = factor * 2.38 ** 2 * (C.LAM ** np.arange(C.NCH)) ** 0.2 / s.nvars
    for m in range(C.NCH):
        s.set_proposal(m, mu=None if mu is None else mu[m], cov=cov, sigma=sig[m])
    return cov


def _expected_proposal(s, st, grads, law, it, delta, factors=None):
    """Per chain: (x' Decimal, scale, drift, (L, Lf, |L^-1|) or None) of iteration `it` from the product's state, gradients and law."""
    mu, cov, sig = law
    out = []
    for m in range(C.NCH):
        A = R.matrix_to_factor(cov[m], C.EPS2, sig[m])
        F = C.exact_factor(A) if factors is None else factors[m]
        z, rho = C.normals(SEED, m, it, s.nvars)
        dr = R.drift(cov[m], sig[m], C.EPS2, delta, grads[m]) if grads is not None else R.Drift([R.ZERO] * s.nvars, np.zeros(s.nvars), False, R.ONE)
        xp, scale = R.proposal(st["vars"][m], dr.d, F[0], z, rho, Lf=F[1])
        out.append((xp, scale, dr, F))
    return out


def _check_draws(s, it, engine):
    zs = s.draws(it)[0]
    for m in range(C.NCH):
        z, rho = C.normals(SEED, m, it, s.nvars)
        assert R.ratio(zs[m], z, [float(r) for r in rho]) <= K_Z, (it, m)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("nv", C.SIZES)
def test_proposal_settled(pkg, stars, nv, engine):
    """Langevin sampler: last_test()[0] against x + d + L z.  Random-walk sampler: the host engine's proposals the same way (d = 0); the
    device engine keeps several candidates per chain and no last_test: there the positions of the chains that moved are the proposals."""
    star, ctx = stars(nv)
    for use_drift in (1, 0):
        s = _sampler(pkg, ctx, star, engine, use_drift=use_drift)
        x0 = s.state()["vars"]
        checked = 0
        for li, name in enumerate(C.LAWS):
            _set_law(pkg, s, star, name)               # before set_state: the next proposal is drawn under the new law
            k0 = 1000 * (li + 1) + 1
            s.set_state(x0, iteration=k0)
            if use_drift:
                s.run(1)                               # makes gradient() valid
                k0 += 1
            for it in (k0, k0 + 1):
                st = s.state()
                assert st["iteration"] == it
                grads = None
                if use_drift:
                    g, gp, valid = s.gradient()
                    assert valid.all()
                    grads = g
                law = s.proposal_law()
                exp = _expected_proposal(s, st, grads, law, it, 0.0)
                _check_draws(s, it, engine)
                s.run(1)
                aft = s.state()
                if use_drift or engine == "host":
                    prop = s.last_test()[0]
                    rows = range(C.NCH)
                else:
                    prop = aft["vars"]
                    rows = [m for m in range(C.NCH) if not np.array_equal(aft["vars"][m], st["vars"][m])]
                for m in rows:
                    xp, scale, dr, F = exp[m]
                    _hold("proposal", engine, R.ratio(prop[m], xp, scale), cap=2 * nv, what="Nv %d %s it %d chain %d drift %d" % (nv, name, it, m, use_drift))
                    checked += 1
        assert checked >= (2 if (not use_drift and engine == "device") else 6 * C.NCH), checked
        s.close()


def _logpost_at(ctx, star, s, prop, mu0):
    """(logL, logPr, logPost) of the proposals as the sampler's own batch evaluates them: the base evaluation of the gradient batch."""
    params = np.tile(star.params, (C.NCH, 1))
    params[:, star.index_to_relax] = prop
    h = FD_REL * np.maximum(np.abs(mu0), 1e-3)
    l0, pr0, _ = ctx.fd_gradient_posterior(star, params, h, C.LAM ** np.arange(C.NCH))
    return l0, pr0, l0 + pr0


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("delta", [0.0, 30.0])
@pytest.mark.parametrize("nv", C.SIZES)
def test_langevin_test(pkg, stars, nv, engine, delta):
    star, ctx = stars(nv)
    s = _sampler(pkg, ctx, star, engine, delta=delta)
    x0 = s.state()["vars"]
    n_checked = n_inside = n_truncated = n_knife = 0
    seen_lnr, gnorm = [], 0.0
    for li, name in enumerate(C.LAWS):
        _set_law(pkg, s, star, name, factor=C.SIGMA_FACTOR)
        k0 = 2000 * (li + 1) + 1
        start = x0.copy()
        if delta > 0 and nv <= 9 and li == 0:
            start[0, :3] *= 0.1                        # |gradient| < 30 at these sizes: under the first law the cold chain starts with
        s.set_state(start, iteration=k0)               # three heights ten times too low (|gradient| = 40: truncated, and r < 1e-6)
        s.run(1)
        for it in (k0 + 1, k0 + 2):
            st = s.state()
            g, gp, valid = s.gradient()
            assert valid.all() and st["iteration"] == it
            law = s.proposal_law()
            s.run(1)
            aft = s.state()
            prop, stats_prop, lq, g_prop = s.last_test()
            logL_p, logPr_p, logPost_p = _logpost_at(ctx, star, s, prop, law[0][0])
            if engine == "host":
                live = np.isfinite(stats_prop[:, 2])
                assert np.array_equal(stats_prop[live, 2], logPost_p[live]), "the batch's base evaluation is not the sampler's"
            for m in range(C.NCH):
                F = C.exact_factor(R.matrix_to_factor(law[1][m], C.EPS2, law[2][m]))
                d_cur = R.drift(law[1][m], law[2][m], C.EPS2, delta, g[m])
                d_new = R.drift(law[1][m], law[2][m], C.EPS2, delta, g_prop[m])
                n_truncated += int(d_cur.truncated or d_new.truncated)
                gnorm = max(gnorm, float(np.linalg.norm(g[m])), float(np.linalg.norm(g_prop[m])))
                qf = R.density(F[0], st["vars"][m], prop[m], d_cur, Lf=F[1], Linv_abs=F[2])
                qr = R.density(F[0], prop[m], st["vars"][m], d_new, Lf=F[1], Linv_abs=F[2])
                t = R.mh_test(logL_p[m], logPr_p[m], logPost_p[m] if np.isfinite(logPr_p[m]) else -math.inf, st["logPost"][m], qf, qr)
                what = "Nv %d %s it %d chain %d delta %g" % (nv, name, it, m, delta)
                if engine == "host" and t.ln_r is not None:
                    _hold("lq", engine, max(R.ratio([lq[m, 0]], [qf.lq], [qf.scale]), R.ratio([lq[m, 1]], [qr.lq], [qr.scale])), what=what)
                got = aft["Pmove"][m]
                u = R.accept_uniform(SEED, m, it)
                moved = np.array_equal(aft["vars"][m], prop[m]) and not np.array_equal(prop[m], st["vars"][m])
                n_checked += 1
                tol_lnr = K["ln_r"][ENGINES.index(engine)] * 2.0 ** -52 * t.scale
                seen_lnr.append("%s:%s" % (name[0], "x" if t.ln_r is None else "%.3g" % float(t.ln_r)))
                if t.ln_r is None:
                    assert got == 0.0 and not moved, what
                    continue
                if t.ln_r >= 0:
                    # r_ref >= 1: exactly 1.0, unless the exponent lies within the tolerance of 0
                    assert got == 1.0 or float(t.ln_r) <= tol_lnr, what
                    if got == 1.0:
                        assert moved, what
                        continue
                if got == 0.0:
                    assert t.ln_r < -700 and not moved, what
                    continue
                n_inside += int(Decimal("1e-6") < t.r < 1)
                with R._ctx():
                    ln_got = R.dec(got).ln()
                _hold("ln_r", engine, R.ratio([0.0], [ln_got - t.ln_r], [t.scale]) if got < 1.0 else float(abs(t.ln_r)) / (2.0 ** -52 * t.scale), what=what)
                # the accept flag: u <= r; left uncompared only when |u - r_ref| is below the tolerance on r
                if abs(u - float(t.r)) <= tol_lnr * float(t.r):
                    n_knife += 1
                else:
                    assert moved == t.accepts(u), what
    s.close()
    print("\nNv %d %s delta %g: %d chain-iterations, %d with 1e-6 < r < 1, %d truncated, %d accept flags uncompared" %
          (nv, engine, delta, n_checked, n_inside, n_truncated, n_knife))
    print("  largest |gradient| %.3g; ln r (law: value, x = refused by a rule):" % gnorm, " ".join(seen_lnr))
    assert n_knife <= 1
    if engine == "host":
        assert 2 * n_inside >= n_checked, (n_inside, n_checked)
        if delta > 0:
            assert n_truncated >= 1


def _check_law(engine, nv, before, x_after, r, it, c0, after, m, what):
    mu, cov, sig = before
    ref = R.adapt(mu[m], cov[m], sig[m], x_after, r, it, c0, 0.234, 1e-12, 1e14, mu_new_given=after[0][m])
    _hold("mu", engine, R.ratio(after[0][m], ref.mu, ref.mu_scale), cap=2 * nv, what=what)
    _hold("cov", engine, R.ratio(after[1][m], [v for row in ref.cov for v in row], ref.cov_scale), cap=2 * nv, what=what)
    _hold("sigma", engine, R.ratio([after[2][m]], [ref.sigma], [ref.sigma_scale]), cap=2 * nv, what=what)
    return ref


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("nv", C.SIZES)
def test_adaptation(pkg, stars, nv, engine):
    star, ctx = stars(nv)
    c0 = 2.0
    s = _sampler(pkg, ctx, star, engine, Nt_learn=(0, 10**6), c0=c0)
    x0 = s.state()["vars"]
    err = pkg.sampler.default_errors(star)
    mu_off = x0 + 0.5 * err * np.cos(np.arange(nv))[None, :] * np.array([1.0, -1.0, 0.5])[:, None]
    for li, name in enumerate(C.LAWS):
        _set_law(pkg, s, star, name, mu=mu_off)
        s.set_state(x0, iteration=50)
        for it in (50, 51):
            st = s.state()
            law = s.proposal_law()
            exp = None
            if it == 51:
                g, gp, valid = s.gradient()
                assert valid.all()
                # the factor in force is the one the engine made of ITS OWN updated matrix in iteration 50
                exp = _expected_proposal(s, st, g, law, it, 0.0)
            s.run(1)
            aft = s.state()
            law2 = s.proposal_law()
            assert aft["iteration"] == it + 1
            for m in range(C.NCH):
                what = "Nv %d %s it %d chain %d" % (nv, name, it, m)
                _check_law(engine, nv, law, aft["vars"][m], aft["Pmove"][m], it, c0, law2, m, what)
                if exp is not None:
                    xp, scale, dr, F = exp[m]
                    _hold("proposal_adapted", engine, R.ratio(s.last_test()[0][m], xp, scale), cap=2 * nv, what=what)
    info = s.info()
    if engine == "device":
        assert info["adapt_in_lds"] == (1 if nv <= 129 else 0), info
    s.close()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("nv", C.SIZES)
def test_indefinite_update_keeps_the_factor(pkg, stars, nv, engine):
    """Gain 10 / 3 > 1: (1 - gamma) Sigma + gamma d d^T has Nv - 1 negative directions.  The covariance is updated all the same, the
    factor of the law before the update stays in force (both engines; the reference hands Eigen's partial factor on)."""
    star, ctx = stars(nv)
    c0 = 10.0
    s = _sampler(pkg, ctx, star, engine, Nt_learn=(2, 3), c0=c0)
    x0 = s.state()["vars"]
    for name in C.LAWS[1:]:
        _set_law(pkg, s, star, name)
        s.set_state(x0, iteration=1)
        s.run(1)                                       # iteration 1: no adaptation; the gradient becomes valid
        law = s.proposal_law()
        old = [C.exact_factor(R.matrix_to_factor(law[1][m], C.EPS2, law[2][m])) for m in range(C.NCH)]
        s.run(1)                                       # iteration 2 adapts with gamma = 10 / 3
        st = s.state()
        law2 = s.proposal_law()
        g, gp, valid = s.gradient()
        assert valid.all() and st["iteration"] == 3
        for m in range(C.NCH):
            what = "Nv %d %s chain %d" % (nv, name, m)
            _check_law(engine, nv, law, st["vars"][m], st["Pmove"][m], 2, c0, law2, m, what)
            assert not np.array_equal(law2[1][m], law[1][m]), what                                         # the covariance is updated
            assert C.exact_factor(R.matrix_to_factor(law2[1][m], C.EPS2, law2[2][m])) is None, what        # ... and is not positive definite
        exp = _expected_proposal(s, st, g, law2, 3, 0.0, factors=old)      # drift of the NEW law, random part of the OLD factor
        s.run(1)
        prop = s.last_test()[0]
        for m in range(C.NCH):
            xp, scale, dr, F = exp[m]
            _hold("proposal", engine, R.ratio(prop[m], xp, scale), cap=2 * nv, what="Nv %d %s chain %d after an indefinite update" % (nv, name, m))
    s.close()


def _find_iteration(s, start, want_A, u_lo, u_hi):
    for k in range(start, start + 20000):
        _, _, us, ia = s.draws(k)
        if ia == want_A and u_lo <= us <= u_hi:
            return k
    raise AssertionError("no such iteration")


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("swap_rule", [0, 1])
@pytest.mark.parametrize("nv", (9, 65, 153))
def test_swap_carries_the_gradient(pkg, stars, nv, engine, swap_rule):
    """dN_mixing = 1.  The pair's outcomes of the MH tests (whose algebra test_langevin_test checks) are read off the positions; the swap
    probability, the exchanged logL / logPrior / logPosterior and the gradient each side then holds are the reference's."""
    star, ctx = stars(nv)
    s = _sampler(pkg, ctx, star, engine, dN_mixing=1, swap_rule=swap_rule)
    T = C.LAM ** np.arange(C.NCH)
    _set_law(pkg, s, star, "ar1")
    s.set_state(s.state()["vars"], iteration=1)
    s.run(12, record=False)                            # the chains part
    seen = {True: 0, False: 0}
    start = 5000
    for want_A, (u_lo, u_hi) in ((0, (0.0, 0.03)), (1, (0.97, 1.0)), (1, (0.0, 0.03)), (0, (0.97, 1.0)), (0, (0.9, 1.0)), (1, (0.9, 1.0))):
        k = _find_iteration(s, start, want_A, u_lo, u_hi)
        start = k + 2
        s.set_state(s.state()["vars"], iteration=k - 1)
        s.run(1)                                       # iteration k - 1: the gradient becomes valid
        st = s.state()
        g, gp, valid = s.gradient()
        mu0 = s.proposal_law()[0][0]
        assert valid.all() and st["iteration"] == k
        s.run(1)
        aft = s.state()
        g2, gp2, _ = s.gradient()
        prop, _, _, g_prop = s.last_test()
        A, u = R.swap_draw(SEED, C.NCH, k)
        assert A == want_A and u == s.draws(k)[2]
        B = A + 1
        # what each chain of the pair held after its own test: the proposal (with the batch's statistics and gradient) or what it had
        params = np.tile(star.params, (C.NCH, 1))
        params[:, star.index_to_relax] = prop
        l0, pr0, gb = ctx.fd_gradient_posterior(star, params, FD_REL * np.maximum(np.abs(mu0), 1e-3), T)
        gpb = ctx.last_grad_prior
        held = {}
        for m in (A, B):
            rows = [aft["vars"][A], aft["vars"][B]]
            took = any(np.array_equal(r, prop[m]) for r in rows) and not np.array_equal(prop[m], st["vars"][m])
            if took:
                assert np.array_equal(gb[m], g_prop[m]), "the batch's gradient is not the sampler's"
                held[m] = (prop[m], (l0[m], pr0[m], l0[m] + pr0[m]), g_prop[m], gpb[m])
            else:
                held[m] = (st["vars"][m], (st["logL"][m], st["logPrior"][m], st["logPost"][m]), g[m], gp[m])
        sw = R.resolve_swap(held[A][1], held[B][1], T[A], T[B], u, swap_rule)
        swapped = np.array_equal(aft["vars"][A], held[B][0]) and np.array_equal(aft["vars"][B], held[A][0]) and not np.array_equal(held[A][0], held[B][0])
        what = "Nv %d rule %d it %d pair %d u %.3f r_T %.3g" % (nv, swap_rule, k, A, u, float(sw.rT))
        if abs(u - float(sw.rT)) > 1e-12:
            assert swapped == sw.swapped, what
        seen[swapped] += 1
        assert aft["swaps"] - st["swaps"] == int(swapped) and aft["swap_attempts"] - st["swap_attempts"] == 1, what
        for m, ref, src in ((A, sw.A, B), (B, sw.B, A)):
            got = [aft["logL"][m], aft["logPrior"][m], aft["logPost"][m]]
            scale = [abs(float(ref[0])), abs(float(ref[1])), abs(float(ref[0])) + abs(float(ref[1]))]
            _hold("swap_stats", engine, R.ratio(got, list(ref), scale), cap=8, what=what)
            if swapped:
                gref, gscale = R.carried_gradient(held[src][2], held[src][3], T[src], T[m])
                _hold("carried_gradient", engine, R.ratio(g2[m], gref, gscale), cap=8, what=what)
                assert np.array_equal(gp2[m], held[src][3]), what
            else:
                assert np.array_equal(g2[m], held[m][2]) and np.array_equal(gp2[m], held[m][3]), what
        if seen[True] and seen[False]:
            break
    s.close()
    assert seen[True] >= 1 and seen[False] >= 1, seen

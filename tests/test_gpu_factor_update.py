"""Rank-one steps of the proposal factor in the learning phase (TAMCMC_OPT_FACTOR_REFRESH = R, opt-in), on both engines, -m gpu.

Stars, sizes and laws of tests/sampler_cases.py (three chains, lambda = 1.5, FAST arithmetic); the reference is tests/factor_update_reference.py
(50 digits) fed with what the product itself reads out -- the factor in force, the law, the state -- as tests/test_gpu_sampler_reference.py
does; mu, Sigma, sigma and the proposals are held to that module's own K.

    test_one_rank_one_step          sizes 3 ... 153, both engines, random walk: mu', Sigma', sigma' are the default rule's; the new factor is
                                    rank_one(old factor, w, beta2) within the reference's bound (with its input term); the next proposal is
                                    x + L' z
    test_refresh_0_and_1_are_todays_chain     samples, statistics, law and factor after 40 adapting iterations, bit for bit; no update counted
    test_schedule_and_counters      93 variables, 64 adapting iterations, R = 16, periods 1 and 3: the counts of the shared schedule
    test_option_values              the value range; an existing sampler keeps the value it was created with
    test_forced_refreshes           a rescaled covariance, set_proposal, a restore: the next adapting iteration is full (counters) and the
                                    factor is the exact factor of (Sigma + eps2 I) sigma within the factorisation's bound (Higham thm 10.3,
                                    as tests/test_sampler_reference.py writes it); a gain above 1 forces full steps too
    test_indefinite_update          gain 10 / 3 with R = 8: the old factor stays, the next adapting iteration is full although its slot is a
                                    rank-one slot
    test_accumulated_drift          the 15 rank-one steps of an R = 16 cycle: L L^T / sigma against Sigma + eps2 rho I in Decimal, within 15
                                    single-step bounds on the matrix
    test_langevin_step              21 variables, both engines: a rank-one step, then the MH test's densities are those of the updated factor
    test_envelope_step              id 1 on the device engine (option 13 as well): one rank-one step

Measured |got - exact| / bound (1.0 allowed) is printed when the module ends.
"""
import math
from decimal import Decimal

import numpy as np
import pytest

import factor_update_reference as F
import sampler_cases as C
import sampler_reference as R
from test_gpu_sampler_reference import K as K_REF

pytestmark = pytest.mark.gpu

ENGINES = ("host", "device")
SEED = 20240917
C0 = 2.0
WORST = {}


def _note(name, engine, r, what):
    if r > WORST.get((name, engine), (-1.0, ""))[0]:
        WORST[(name, engine)] = (r, what)


def _k(name, engine):
    return K_REF[name][ENGINES.index(engine)]


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
    print("\nworst ratios of tests/test_gpu_factor_update.py:")
    for (name, engine), (r, what) in sorted(WORST.items()):
        print("  %-22s %-6s r = %8.4f   (%s)" % (name, engine, r, what))


def _sampler(pkg, ctx, star, engine, refresh, **kw):
    args = dict(nchains=C.NCH, lambda_temp=C.LAM, engine=engine, use_drift=0, seed=SEED, Nt_learn=(0, 10**6), periods_learn=(1,),
                dN_mixing=10**6, c0=C0, epsilon2=C.EPS2)
    args.update(kw)
    ctx.set_option(pkg.OPT_FACTOR_REFRESH, refresh)
    try:
        return pkg.Sampler(ctx, star, **args)
    finally:
        ctx.set_option(pkg.OPT_FACTOR_REFRESH, 0)          # read at creation: the sampler keeps its value


def _set_law(pkg, s, star, name, mu=None, factor=1.0):
    cov = C.law(name, pkg.sampler.default_errors(star))
    sig = factor * 2.38 ** 2 * (C.LAM ** np.arange(C.NCH)) ** 0.2 / s.nvars
    for m in range(C.NCH):
        s.set_proposal(m, mu=None if mu is None else mu[m], cov=cov, sigma=sig[m])
    return cov


def _mu_off(pkg, star, x0):
    err = pkg.sampler.default_errors(star)
    return x0 + 0.5 * err * np.cos(np.arange(x0.shape[1]))[None, :] * np.array([1.0, -1.0, 0.5])[:, None]


def _counts(s):
    i = s.info()
    return np.array([i["factor_updates"], i["factor_refreshes"], i["factor_refreshes_forced"]])


def _dec_rows(L):
    return [[R.dec(L[i][k]) for k in range(i + 1)] for i in range(len(L))]


def _check_law(engine, nv, before, x_after, r, it, c0, after, m, what, A1=1e14):
    mu, cov, sig = before
    ref = R.adapt(mu[m], cov[m], sig[m], x_after, r, it, c0, 0.234, 1e-12, A1, mu_new_given=after[0][m])
    for name, got, want, scale in (("mu", after[0][m], ref.mu, ref.mu_scale), ("cov", after[1][m], [v for row in ref.cov for v in row], ref.cov_scale),
                                   ("sigma", [after[2][m]], [ref.sigma], [ref.sigma_scale])):
        rr = R.ratio(got, want, scale)
        _note(name, engine, rr, what)
        assert rr <= min(_k(name, engine), 2 * nv), "%s %s: ratio %.3g" % (name, what, rr)
    return ref


def _step_inputs(law, law2, x_after, it, c0, m):
    """w and beta2 of the step as the engines form them, in double: g = c0 / (1 + i), w = sqrt(g sigma') (x - mu'), beta2 = (1 - g) sigma' / sigma."""
    g = c0 / (1.0 + it)
    d = np.asarray(x_after, dtype=np.float64) - law2[0][m]
    return np.sqrt(g * law2[2][m]) * d, (1.0 - g) * law2[2][m] / law[2][m], g


def _check_rank_one_step(engine, nv, L0, law, law2, x_after, it, c0, L1, m, what):
    w, beta2, g = _step_inputs(law, law2, x_after, it, c0, m)
    assert 0.0 < g <= 0.5
    upd = F.rank_one(L0, w, beta2)
    assert upd is not None, what
    assert np.all(np.triu(L1, 1) == 0.0), what
    r = F.ratio(L1, upd, k_in=F.K_IN)
    _note("factor", engine, r, what)
    assert r <= 1.0, "%s: the new factor is not the rank-one update of the old one, ratio %.3g" % (what, r)
    assert not np.array_equal(L1, L0), what
    return upd


def _check_next_proposal(s, engine, nv, it, st_before, L_in_force, chains, what):
    """Runs iteration `it`; its proposals (host engine: last_test; device engine: the positions of the chains that moved) are x + L z."""
    s.run(1)
    aft = s.state()
    if engine == "host":
        prop, rows = s.last_test()[0], list(chains)
    else:
        prop = aft["vars"]
        rows = [m for m in chains if not np.array_equal(aft["vars"][m], st_before["vars"][m])]
    for m in rows:
        z, rho = C.normals(SEED, m, it, nv)
        xp, scale = R.proposal(st_before["vars"][m], [R.ZERO] * nv, _dec_rows(L_in_force[m]), z, rho, Lf=L_in_force[m])
        r = R.ratio(prop[m], xp, scale)
        _note("proposal", engine, r, what + " chain %d" % m)
        assert r <= min(_k("proposal", engine), 2 * nv), "%s chain %d: proposal ratio %.3g" % (what, m, r)
    return len(rows)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("nv", (3, 8, 9, 64, 65, 93, 129, 153))
def test_one_rank_one_step(pkg, stars, nv, engine):
    star, ctx = stars(nv)
    laws = ("ar1",) if nv >= 153 else ("ar1", "pairs")
    chains = (0,) if nv >= 153 else range(C.NCH)
    proposals = 0
    for name in laws:
        s = _sampler(pkg, ctx, star, engine, 4)            # (a sampler per law: the schedule counts a sampler's adapting iterations)
        x0 = s.state()["vars"]
        _set_law(pkg, s, star, name, mu=_mu_off(pkg, star, x0))
        s.set_state(x0, iteration=50)
        s.run(1)                                           # k = 0: the scheduled full step
        c0 = _counts(s)
        st, law = s.state(), s.proposal_law()
        L0 = [s.factor(m) for m in range(C.NCH)]
        s.run(1)                                           # iteration 51: the rank-one step (gain 2 / 52)
        aft, law2 = s.state(), s.proposal_law()
        L1 = [s.factor(m) for m in range(C.NCH)]
        assert aft["iteration"] == 52
        assert np.array_equal(_counts(s) - c0, [C.NCH, 0, 0]), (_counts(s), c0)
        for m in chains:
            what = "Nv %d %s chain %d %s" % (nv, name, m, engine)
            _check_law(engine, nv, law, aft["vars"][m], aft["Pmove"][m], 51, C0, law2, m, what)
            _check_rank_one_step(engine, nv, L0[m], law, law2, aft["vars"][m], 51, C0, L1[m], m, what)
        proposals += _check_next_proposal(s, engine, nv, 52, aft, L1, range(C.NCH), "Nv %d %s %s" % (nv, name, engine))
        if engine == "device":
            assert s.info()["adapt_in_lds"] == (1 if nv <= 129 else 0)
        s.close()
    assert proposals >= (len(laws) * C.NCH if engine == "host" else 1), proposals


@pytest.mark.parametrize("engine", ENGINES)
def test_refresh_0_and_1_are_todays_chain(pkg, stars, engine):
    star, ctx = stars(21)
    out = []
    for refresh in (0, 1):
        s = _sampler(pkg, ctx, star, engine, refresh, dN_mixing=5)
        s.set_state(s.state()["vars"], iteration=50)
        smp, stt = s.run(40, stats=True)
        info = s.info()
        assert info["factor_updates"] == 0 and info["factor_refreshes_forced"] == 0 and info["factor_refreshes"] == 40 * C.NCH, info
        out.append((smp, stt, s.proposal_law(), [s.factor(m) for m in range(C.NCH)]))
        s.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    for x, y in zip(a[3], b[3]):
        assert np.array_equal(x, y) and np.all(np.diag(x) > 0)
    # the factor read out is the one the law implies (the last full step's)
    mu, cov, sig = a[2]
    for m in range(C.NCH):
        Fx = C.exact_factor(R.matrix_to_factor(cov[m], C.EPS2, sig[m]))
        assert Fx is not None and _factorisation_ratio(a[3][m], Fx) <= 1.0


def _predicted(n_adapt, refresh):
    """The shared schedule (step_schedule.h::factor_step_mode): adapting iteration k is full when R < 2 or k % R == 0."""
    full = sum(1 for k in range(n_adapt) if refresh < 2 or k % refresh == 0)
    return full, n_adapt - full


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("period", (1, 3))
def test_schedule_and_counters(pkg, stars, engine, period):
    star, ctx = stars(93)
    first = 102 if period == 3 else 100
    window = (100, first + 63 * period + 1)
    s = _sampler(pkg, ctx, star, engine, 16, Nt_learn=window, periods_learn=(period,), dN_mixing=7)
    s.set_state(s.state()["vars"], iteration=90)
    s.run(window[1] + 5 - 90, record=False)
    n_adapt = sum(1 for i in range(90, window[1] + 5) if window[0] <= i < window[1] and i % period == 0)
    assert n_adapt == 64
    full, upd = _predicted(n_adapt, 16)
    assert (full, upd) == (4, 60)
    assert np.array_equal(_counts(s), [upd * C.NCH, full * C.NCH, 0]), s.info()
    s.close()


def test_option_values(pkg, stars):
    star, ctx = stars(9)
    for bad in (-1, 65537, 1 << 20):
        with pytest.raises(pkg.TamcmcError) as e:
            ctx.set_option(pkg.OPT_FACTOR_REFRESH, bad)
        assert e.value.code == pkg.ERR_BAD_ARG
    for good in (0, 1, 2, 65536):
        ctx.set_option(pkg.OPT_FACTOR_REFRESH, good)
    ctx.set_option(pkg.OPT_FACTOR_REFRESH, 0)
    s = _sampler(pkg, ctx, star, "device", 4)              # (the context is back at 0 when _sampler returns)
    s.set_state(s.state()["vars"], iteration=50)
    s.run(4, record=False)
    assert np.array_equal(_counts(s), [3 * C.NCH, C.NCH, 0]), s.info()
    s.close()


def _factorisation_ratio(L, Fx):
    """|L - exact| over the first-order bound of a computed Cholesky factor: g_(n+1) |L| tril(|L^-1| |L| |L^T| |L^-T|) (Higham thm 10.3)."""
    n = L.shape[0]
    Lf, Li = np.abs(Fx[1]), Fx[2]
    gk = (n + 1) * 2.0 ** -53 / (1 - (n + 1) * 2.0 ** -53)
    bound = 1.01 * gk * Lf @ np.tril(Li @ Lf @ Lf.T @ Li.T)
    worst = 0.0
    with R._ctx():
        for i in range(n):
            for k in range(i + 1):
                diff = abs(R.dec(L[i][k]) - Fx[0][i][k])
                if diff != 0:
                    worst = max(worst, float(diff / R.dec(bound[i, k])))
    return worst


def _is_full_factor(s, engine, what):
    mu, cov, sig = s.proposal_law()
    for m in range(C.NCH):
        Fx = C.exact_factor(R.matrix_to_factor(cov[m], C.EPS2, sig[m]))
        assert Fx is not None, what
        r = _factorisation_ratio(s.factor(m), Fx)
        _note("full factor", engine, r, what + " chain %d" % m)
        assert r <= 1.0, "%s chain %d: not the factor of (Sigma + eps2 I) sigma, ratio %.3g" % (what, m, r)


@pytest.mark.parametrize("engine", ENGINES)
def test_forced_refreshes(pkg, stars, engine, tmp_path):
    nv = 9
    star, ctx = stars(nv)
    N = C.NCH

    def start(s, x0):
        """full step (iteration 50), rank-one step (iteration 51): the next slots are rank-one slots too (R = 8)"""
        c = _counts(s)
        _set_law(pkg, s, star, "ar1", mu=_mu_off(pkg, star, x0))
        s.set_state(x0, iteration=50)
        s.run(2)
        d = _counts(s) - c
        assert d[0] == N and d[1] + d[2] == N, d
        return _counts(s)

    # set_proposal, then a restore: the next adapting iteration is full, the one after is a rank-one step again
    s = _sampler(pkg, ctx, star, engine, 8)
    x0 = s.state()["vars"]
    c = start(s, x0)                                       # k = 0, 1
    mu, cov, sig = s.proposal_law()
    for m in range(N):
        s.set_proposal(m, mu=mu[m], cov=cov[m], sigma=sig[m])
    s.run(1)                                               # k = 2
    assert np.array_equal(_counts(s) - c, [0, 0, N]), "set_proposal: " + str(_counts(s) - c)
    _is_full_factor(s, engine, "after set_proposal (%s)" % engine)
    s.run(1)                                               # k = 3
    assert np.array_equal(_counts(s) - c, [N, 0, N])
    root = str(tmp_path / "restore_")
    s.write_restore(root)
    s.read_restore(root)
    c = _counts(s)
    s.run(1)                                               # k = 4
    assert np.array_equal(_counts(s) - c, [0, 0, N]), "restore: " + str(_counts(s) - c)
    _is_full_factor(s, engine, "after a restore (%s)" % engine)
    s.run(1)                                               # k = 5
    assert np.array_equal(_counts(s) - c, [N, 0, N])
    s.close()

    # A covariance rescaled by p2_fct.  A1 = |x| - delta with delta^2 = 30 |x|: the mean (it starts at the chains' position) is clipped
    # to norm A1 in every step, so the deviation x - mu' has norm ~ delta and g |d d^T| = (2 / 52) 30 |x| > A1 -- the updated covariance
    # exceeds A1 whatever it was.  The law is scaled to norm 2 A1 (clipped by the first step already) with a small sigma, so that the
    # chains hardly move.  mu and sigma are clipped as they are with R = 0: the three updates are the default's.
    nrm = float(np.min(np.linalg.norm(x0, axis=1)))
    delta = math.sqrt(30.0 * nrm)
    assert delta < 0.5 * nrm
    A1 = nrm - delta
    cov0 = C.law("ar1", pkg.sampler.default_errors(star))
    cov0 = cov0 * (2.0 * A1 / float(np.linalg.norm(cov0)))
    s = _sampler(pkg, ctx, star, engine, 8, A1=A1)
    c = _counts(s)
    for m in range(N):
        s.set_proposal(m, mu=x0[m], cov=cov0, sigma=1e-6)
    s.set_state(x0, iteration=50)
    s.run(1)                                               # k = 0: scheduled
    law = s.proposal_law()
    assert np.all(np.abs(np.linalg.norm(law[1].reshape(N, -1), axis=1) / A1 - 1.0) < 1e-12)
    s.run(1)                                               # k = 1: a rank-one slot, the factor is marked valid, the gain is 2 / 52 -- and the norm clips
    law2, aft = s.proposal_law(), s.state()
    assert np.all(np.abs(np.linalg.norm(law2[1].reshape(N, -1), axis=1) / A1 - 1.0) < 1e-12)
    assert np.array_equal(_counts(s) - c, [0, N, N]), "p2_fct: " + str(_counts(s) - c)
    for m in range(N):
        _check_law(engine, nv, law, aft["vars"][m], aft["Pmove"][m], 51, C0, law2, m, "clipped covariance chain %d %s" % (m, engine), A1=A1)
    _is_full_factor(s, engine, "after p2_fct rescaled (%s)" % engine)
    s.close()

    # a gain above 1 (adaptation before iteration c0): every step is full (test_indefinite_update looks at the factor)
    s = _sampler(pkg, ctx, star, engine, 8, c0=10.0, Nt_learn=(2, 10**6))
    _set_law(pkg, s, star, "ar1")
    s.set_state(x0, iteration=1)
    s.run(1)
    c = _counts(s)
    s.run(3)                                               # iterations 2, 3, 4: k = 0 (scheduled), 1, 2 (rank-one slots, gains 10/4, 10/5)
    assert np.array_equal(_counts(s) - c, [0, N, 2 * N]), _counts(s) - c
    s.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_indefinite_update(pkg, stars, engine):
    nv = 9
    star, ctx = stars(nv)
    N = C.NCH
    s = _sampler(pkg, ctx, star, engine, 8, c0=10.0, Nt_learn=(2, 3, 20, 30), periods_learn=(1, 10**6, 1))
    x0 = s.state()["vars"]
    for name in C.LAWS[1:]:
        c = _counts(s)
        _set_law(pkg, s, star, name)
        s.set_state(x0, iteration=1)
        s.run(1)
        law = s.proposal_law()
        L_old = [s.factor(m) for m in range(N)]
        for m in range(N):
            Fx = C.exact_factor(R.matrix_to_factor(law[1][m], C.EPS2, law[2][m]))
            assert _factorisation_ratio(L_old[m], Fx) <= 1.0
        s.run(1)                                           # iteration 2 adapts with gamma = 10 / 3
        law2 = s.proposal_law()
        for m in range(N):
            assert C.exact_factor(R.matrix_to_factor(law2[1][m], C.EPS2, law2[2][m])) is None           # not positive definite
            assert np.array_equal(s.factor(m), L_old[m]), "the old factor must stay in force"
        d2 = _counts(s) - c
        assert d2[0] == 0 and d2[1] + d2[2] == N, d2
        s.run(17, record=False)                            # iterations 3 ... 19: no adaptation
        assert np.array_equal(_counts(s) - c, d2)
        s.run(1)                                           # iteration 20: gain 10 / 21 < 1 in a rank-one slot, but the mark is cleared
        d20 = _counts(s) - c - d2
        assert np.array_equal(d20, [0, 0, N]), d20
    s.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_accumulated_drift(pkg, stars, engine):
    nv = 21
    star, ctx = stars(nv)
    N = C.NCH
    s = _sampler(pkg, ctx, star, engine, 16)
    x0 = s.state()["vars"]
    _set_law(pkg, s, star, "ar1", mu=_mu_off(pkg, star, x0))
    s.set_state(x0, iteration=50)
    s.run(1)                                               # k = 0: the cycle's full step
    c = _counts(s)
    law = s.proposal_law()
    single = [np.zeros((nv, nv)) for _ in range(N)]        # the largest single-step bound on L L^T / sigma, element by element
    start = []
    for m in range(N):                                     # the full step's own bound: g_(n+1) |L| |L^T| (Higham thm 10.3), two roundings of the matrix
        L = np.abs(s.factor(m))
        start.append(((nv + 1) * F.U * 1.01 * (L @ L.T) + 2 * 2.0 ** -53 * np.abs(R.matrix_to_factor(law[1][m], C.EPS2, law[2][m]))) / law[2][m])
    gains = []
    for it in range(51, 66):
        L0 = [s.factor(m) for m in range(N)]
        s.run(1)
        aft, law2 = s.state(), s.proposal_law()
        gains.append(Decimal(2) / Decimal(1 + it))
        for m in range(N):
            w, beta2, g = _step_inputs(law, law2, aft["vars"][m], it, C0, m)
            S1, S2 = F.magnitudes(L0[m], w, beta2)
            d = aft["vars"][m] - law2[0][m]
            cov_scale = np.abs(law[1][m]) + g * (np.abs(np.outer(d, d)) + np.abs(law[1][m]))
            step = F.U * (F.K1(nv) * S1 + (F.K2(nv) + F.K_IN) * S2) / law2[2][m] + _k("cov", engine) * 2.0 ** -52 * cov_scale
            single[m] = np.maximum(single[m], step)
        law = law2
    assert np.array_equal(_counts(s) - c, [15 * N, 0, 0])
    for m in range(N):
        L = s.factor(m)
        want, rho = F.law_matrix(law[1][m], 1.0, C.EPS2, gains)
        bound = 1.01 * (15 * single[m] + start[m])
        worst = 0.0
        with R._ctx():
            Ld, sg = _dec_rows(L), R.dec(law[2][m])
            for i in range(nv):
                for j in range(i + 1):
                    got = sum((Ld[i][k] * Ld[j][k] for k in range(j + 1)), R.ZERO) / sg
                    worst = max(worst, float(abs(got - want[i][j]) / R.dec(bound[i, j])))
        _note("drift, 15 steps", engine, worst, "chain %d rho %.4f" % (m, float(rho)))
        assert worst <= 1.0, "chain %d: L L^T / sigma is not Sigma + eps2 rho I after 15 rank-one steps, ratio %.3g" % (m, worst)
    s.close()


def _logpost_at(ctx, star, prop, mu0, fd_rel):
    params = np.tile(star.params, (C.NCH, 1))
    params[:, star.index_to_relax] = prop
    h = fd_rel * np.maximum(np.abs(mu0), 1e-3)
    l0, pr0, _ = ctx.fd_gradient_posterior(star, params, h, C.LAM ** np.arange(C.NCH))
    return l0, pr0, l0 + pr0


@pytest.mark.parametrize("engine", ENGINES)
def test_langevin_step(pkg, stars, engine):
    nv, fd_rel = 21, 1e-7
    star, ctx = stars(nv)
    s = _sampler(pkg, ctx, star, engine, 4, use_drift=1, fd_step_rel=fd_rel, delta=0.0)
    x0 = s.state()["vars"]
    _set_law(pkg, s, star, "ar1", mu=_mu_off(pkg, star, x0), factor=C.SIGMA_FACTOR)
    s.set_state(x0, iteration=50)
    s.run(1)                                               # k = 0: full
    c = _counts(s)
    law = s.proposal_law()
    L0 = [s.factor(m) for m in range(C.NCH)]
    s.run(1)                                               # k = 1: the rank-one step, in k_mala_test
    aft, law2 = s.state(), s.proposal_law()
    L1 = [s.factor(m) for m in range(C.NCH)]
    assert np.array_equal(_counts(s) - c, [C.NCH, 0, 0])
    for m in range(C.NCH):
        what = "Langevin Nv %d chain %d %s" % (nv, m, engine)
        _check_law(engine, nv, law, aft["vars"][m], aft["Pmove"][m], 51, C0, law2, m, what)
        _check_rank_one_step(engine, nv, L0[m], law, law2, aft["vars"][m], 51, C0, L1[m], m, what)
    # iteration 52: proposal and both densities with the updated factor, the drift from Sigma as ever
    g, gp, valid = s.gradient()
    assert valid.all()
    s.run(1)
    end = s.state()
    prop, stats_prop, lq, g_prop = s.last_test()
    logL_p, logPr_p, logPost_p = _logpost_at(ctx, star, prop, law2[0][0], fd_rel)
    checked = 0
    for m in range(C.NCH):
        what = "Langevin test Nv %d chain %d %s" % (nv, m, engine)
        Ld, Li = _dec_rows(L1[m]), R.abs_inverse(L1[m])
        d_cur = R.drift(law2[1][m], law2[2][m], C.EPS2, 0.0, g[m])
        d_new = R.drift(law2[1][m], law2[2][m], C.EPS2, 0.0, g_prop[m])
        z, rho = C.normals(SEED, m, 52, nv)
        xp, scale = R.proposal(aft["vars"][m], d_cur.d, Ld, z, rho, Lf=L1[m])
        r = R.ratio(prop[m], xp, scale)
        _note("proposal", engine, r, what)
        assert r <= min(_k("proposal", engine), 2 * nv), "%s: proposal ratio %.3g" % (what, r)
        qf = R.density(Ld, aft["vars"][m], prop[m], d_cur, Lf=L1[m], Linv_abs=Li)
        qr = R.density(Ld, prop[m], aft["vars"][m], d_new, Lf=L1[m], Linv_abs=Li)
        t = R.mh_test(logL_p[m], logPr_p[m], logPost_p[m] if np.isfinite(logPr_p[m]) else -math.inf, aft["logPost"][m], qf, qr)
        if t.ln_r is None:
            continue
        if engine == "host":
            r = max(R.ratio([lq[m, 0]], [qf.lq], [qf.scale]), R.ratio([lq[m, 1]], [qr.lq], [qr.scale]))
            _note("lq", engine, r, what)
            assert r <= _k("lq", engine), "%s: density ratio %.3g" % (what, r)
            checked += 1
        got = end["Pmove"][m]
        if 0.0 < got < 1.0:
            with R._ctx():
                ln_got = R.dec(got).ln()
            r = R.ratio([0.0], [ln_got - t.ln_r], [t.scale])
            _note("ln_r", engine, r, what)
            assert r <= _k("ln_r", engine), "%s: ln r ratio %.3g" % (what, r)
            checked += 1
        elif got == 1.0:
            assert t.ln_r >= 0 or float(-t.ln_r) <= _k("ln_r", engine) * 2.0 ** -52 * t.scale, what
    assert checked >= 1
    s.close()


def test_envelope_step(pkg, synth):
    import test_gpu_envelope as ge
    star = ge._synthetic(synth, 1, nx=2049, seed=12)
    ctx = pkg.HipContext(0)
    ctx.set_spectrum(star.x, star.y)
    ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_ENGINE, 1)
    try:
        s = _sampler(pkg, ctx, star, "device", 4)
        nv = s.nvars
        s.set_state(s.state()["vars"], iteration=50)
        s.run(1)                                           # k = 0: full
        c = _counts(s)
        law = s.proposal_law()
        L0 = [s.factor(m) for m in range(C.NCH)]
        s.run(1)                                           # k = 1: rank-one
        aft, law2 = s.state(), s.proposal_law()
        assert np.array_equal(_counts(s) - c, [C.NCH, 0, 0]) and s.info()["engine"] == 1
        for m in range(C.NCH):
            what = "envelope id 1 chain %d" % m
            _check_law("device", nv, law, aft["vars"][m], aft["Pmove"][m], 51, C0, law2, m, what)
            _check_rank_one_step("device", nv, L0[m], law, law2, aft["vars"][m], 51, C0, s.factor(m), m, what)
        s.close()
    finally:
        ctx.close()

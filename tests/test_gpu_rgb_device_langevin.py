"""Langevin step of the red-giant models (ids 25 / 27) on the device-resident engine, opt-in through TAMCMC_OPT_RGB_DEVICE_LANGEVIN
(csrc/dev_sampler.hip: DevSampler::init / run_mala; the proposals' tables come from the gradient batch, csrc/fd_batch.hip).

One star for the file, the one tests/test_gpu_rgb_gradient.py builds for itself: 4000 bins, 4 radial orders, l = 0..3, period spacing
200 s under the uniform prior [199, 201] -> about 25 mixed modes, a batch of 3 x (Nvars + 1) = 108 vectors (35 free parameters).  Two FAST contexts, one with the option and one without."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCH, LAM = 3, 1.6
T = np.array([math.pow(LAM, m) for m in range(NCH)])     # the engine's ladder: pow(lambda, m)
KW = dict(nchains=NCH, lambda_temp=LAM, use_drift=1, seed=5, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,))
EPS = 2.0 ** -53
# test 4: seed of the two engines, number of iterations and the initial proposal error of Hfactor, chosen on the HOST-DRIVEN engine alone
# (see the test's docstring)
WALK_SEED, WALK_ITER, WALK_HFACTOR_ERROR = 2, 25, 0.1


def _small_star(synth, cte=False):
    star = synth.make_c5_star(nx=4000, nmax=4, dnu=20.0, nferr=4, cte_width=cte)
    o = np.cumsum([0] + list(star.plength))
    star.params[o[3] + 1] = 200.0                 # period spacing
    star.priors[:2, o[3] + 1] = [199.0, 201.0]
    return star


@pytest.fixture(scope="module")
def star(synth, oracle):
    s = _small_star(synth)
    st, m0 = oracle.call_model(s.model_id, s.params, s.plength, s.x)
    assert st == 0
    s.set_spectrum_from_model(m0, 4)
    return s


@pytest.fixture(scope="module")
def ctx_on(pkg, star):
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    c.set_spectrum(star.x, star.y)
    c.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_off(pkg, star):
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    c.set_spectrum(star.x, star.y)
    yield c
    c.close()


def _direct(ctx, star, s, vars_):
    """fd_gradient_posterior at the positions vars_ [NCH x Nvars] with the sampler's steps: (grad, grad_prior, logPrior)."""
    P = np.tile(star.params, (NCH, 1))
    P[:, star.index_to_relax] = vars_
    h = 1e-7 * np.maximum(np.abs(s.get_proposal(0)[0]), 1e-3)     # the engine's steps: fd_step_rel max(|mu_0|, 1e-3)
    _, pr0, g = ctx.fd_gradient_posterior(star, P, h, T)
    return g, ctx.last_grad_prior.copy(), pr0


def _assembly_bound(g_direct, gp_direct):
    """4 * 2^-53 * (|grad - grad_prior| + |grad_prior|): see test_held_gradient_is_the_direct_gradient."""
    return 4 * EPS * (np.abs(g_direct - gp_direct) + np.abs(gp_direct))


def _same_gradient(g, g_direct, gp_direct, what):
    """The device's assembly of a gradient against the host's assembly from the same batch.  Where the host's is not finite (a base
    point outside the prior's support whose perturbed point is inside it) the device holds 0 (mala_gradient's !isfinite rule)."""
    fin = np.isfinite(g_direct)
    assert np.all(g[~fin] == 0.0), what
    d = np.abs(g[fin] - g_direct[fin])
    bound = _assembly_bound(g_direct, gp_direct)[fin]
    print("\n%s: %d of %d components differ, max |d| / bound %.3e" % (what, np.count_nonzero(d), d.size, np.max(d / np.maximum(bound, 1e-300), initial=0.0)))
    assert np.all(d <= bound), what


def test_gate(pkg, synth, star, ctx_on, ctx_off):
    """Fails without the feature: the option does not exist (TAMCMC_ERR_BAD_ARG) and the constructor ends in TAMCMC_ERR_BAD_MODEL."""
    ctx_on.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 1)
    with pytest.raises(pkg.TamcmcError) as e:
        ctx_on.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 2)
    assert e.value.code == pkg.ERR_BAD_ARG
    s = pkg.Sampler(ctx_on, star, engine="device", **KW)
    i0 = s.info()
    assert i0["engine"] == 1 and i0["fused_available"] == 0 and i0["iter_lockstep"] == 0
    smp, stt = s.run(5, stats=True)
    i1 = s.info()
    assert i1["iter_lockstep"] == 5 and i1["iter_fused"] == 0 and s.state()["iteration"] == 5
    assert np.isfinite(smp).all() and np.isfinite(stt).all()
    s.close()
    s27 = _small_star(synth, cte=True)                               # id 27, a context of its own
    c27 = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    try:
        c27.set_spectrum(s27.x, star.y)
        with pytest.raises(pkg.TamcmcError) as e:
            pkg.Sampler(c27, s27, engine="device", **KW)
        assert e.value.code == pkg.ERR_BAD_MODEL
        c27.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 1)
        s = pkg.Sampler(c27, s27, engine="device", **KW)
        assert s27.model_id == 27 and s.info()["engine"] == 1 and s.info()["fused_available"] == 0
        smp, stt = s.run(5, stats=True)
        assert s.info()["iter_lockstep"] == 5 and s.info()["iter_fused"] == 0 and np.isfinite(smp).all() and np.isfinite(stt).all()
        c27.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 0)               # read at creation: the existing sampler goes on
        s.run(2)
        assert s.state()["iteration"] == 7
        s.close()
    finally:
        c27.close()
    with pytest.raises(pkg.TamcmcError) as e:                        # the default: today's refusal
        pkg.Sampler(ctx_off, star, engine="device", **KW)
    assert e.value.code == pkg.ERR_BAD_MODEL
    s = pkg.Sampler(ctx_off, star, engine="device", **dict(KW, use_drift=0))   # ... and today's random walk
    s.run(2)
    s.close()
    ms = synth.make_c2_star()                                        # a main-sequence star on a context with the option
    cms = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    try:
        cms.set_spectrum(ms.x, np.ones_like(ms.x))
        cms.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 1)
        s = pkg.Sampler(cms, ms, engine="device", **KW)
        s.run(2)
        assert s.info()["engine"] == 1 and s.info()["iter_lockstep"] == 2
        s.close()
    finally:
        cms.close()
    env = synth.make_envelope_star(1)
    with pytest.raises(pkg.TamcmcError) as e:
        pkg.Sampler(ctx_on, env, engine="device", **dict(KW, use_drift=0))
    assert e.value.code == pkg.ERR_BAD_MODEL
    with pytest.raises(pkg.TamcmcError) as e:
        pkg.Sampler(ctx_on, env, engine="device", **KW)
    assert e.value.code == pkg.ERR_BAD_MODEL


def test_held_gradient_is_the_direct_gradient(pkg, star, ctx_on):
    """The check tests/test_gpu_rgb_gradient.py::test_host_engine_langevin_sampler makes, on the device engine: the gradient the sampler
    holds for a chain is the direct call's on the chain's position -- the same batch code on the same doubles.

    Not bit for bit: the two ASSEMBLIES of a component from the batch's sums round one operation differently.  The tempered
    log-likelihood difference -p dS / T is formed in long double on the host (assemble_gradient, fd_batch.hip: product and division in
    long double, then ONE rounding to double, as the reference's call_likelihood does) and in double on the device (mala_gradient,
    dev_mala_impl.h: the division by T rounds to double at once).  The host's value is rounded twice (64-bit, then 53-bit significand),
    so the two can differ by one ulp of that difference when T != 1 -- about once in 2^11 components (seen on the MI355X: one of the
    2625 components of test_one_iteration_at_a_time_against_the_host_engine's first walk, at 0.35 of the bound).  Bound per component: the
    operations are a multiply, two divisions and one addition, half an ulp each: 4 * 2^-53 * (|grad - grad_prior| + |grad_prior|).
    With swaps (dN_mixing = 1) a gradient that followed its position through a swap was re-tempered, at most once per iteration:
    the existing test's bound 4 n 2^-53 (|g| + |g_prior|) for the chains `valid` marks."""
    n = 30
    s = pkg.Sampler(ctx_on, star, engine="device", **dict(KW, dN_mixing=10**6))   # no swap within the run: nothing is re-tempered
    s.run(n)
    assert s.state()["swap_attempts"] == 0
    g, gp, valid = s.gradient()
    assert valid.all()
    g_direct, gp_direct, _ = _direct(ctx_on, star, s, s.state()["vars"])
    _same_gradient(g, g_direct, gp_direct, "held vs direct gradient, no swaps")
    _same_gradient(gp, gp_direct, gp_direct, "held vs direct prior share, no swaps")
    s.close()
    s = pkg.Sampler(ctx_on, star, engine="device", **dict(KW, dN_mixing=1))
    smp, stt = s.run(n, stats=True)
    assert np.isfinite(smp).all() and np.isfinite(stt).all()
    st = s.state()
    assert st["accepted0"] > 0 and st["swap_attempts"] == n - 1
    g, gp, valid = s.gradient()
    assert valid.any()
    g_direct, gp_direct, _ = _direct(ctx_on, star, s, st["vars"])
    for m in np.flatnonzero(valid):
        bound = 4 * n * EPS * (np.abs(g_direct[m]) + np.abs(gp_direct[m]))
        print("\nchain %d: held vs direct gradient with swaps, max |d| / bound %.3e" % (m, np.max(np.abs(g[m] - g_direct[m]) / np.maximum(bound, 1e-300))))
        assert np.all(np.abs(g[m] - g_direct[m]) <= bound), m
    s.close()


def test_same_call_twice_and_a_second_call_continues(pkg, star, ctx_on):
    a = pkg.Sampler(ctx_on, star, engine="device", **KW)
    b = pkg.Sampler(ctx_on, star, engine="device", **KW)
    smp_a, stt_a = a.run(30, stats=True)
    smp_b, stt_b = b.run(30, stats=True)
    assert np.array_equal(smp_a, smp_b) and np.array_equal(stt_a, stt_b)
    c = pkg.Sampler(ctx_on, star, engine="device", **KW)
    s1, t1 = c.run(12, stats=True)
    s2, t2 = c.run(18, stats=True)
    assert np.array_equal(np.concatenate([s1, s2]), smp_a) and np.array_equal(np.concatenate([t1, t2]), stt_a)
    assert c.state()["iteration"] == 30 and np.array_equal(c.state()["vars"], a.state()["vars"])
    assert len(np.unique(smp_a[:, 0, 0])) > 1                         # (the chains moved)
    for s in (a, b, c):
        s.close()


def test_one_iteration_at_a_time_against_the_host_engine(pkg, star, ctx_on):
    """WALK_ITER iterations with swaps (dN_mixing = 1), no adaptation, same seed on both engines.  Before each iteration both engines get
    the host-driven engine's previous state (set_state: both recompute their gradients there), then one iteration each.
      * proposals: within 2e-6 of the step's length (the bound tests/test_gpu_sampler_oracle.py states for x + drift + L z against the
        oracle; an outer limit here -- both engines use the same batch, the linear algebra around it differs by rounding);
      * the device's gradient at its proposals against the direct call at those proposals: the relation of
        test_held_gradient_is_the_direct_gradient;
      * records after the test: positions and the three statistics to rtol 1e-9 for every chain whose comparator is not within
        5e-3 r of its move probability (the rule of _one_langevin_iteration_against_oracle; a swap pair leaves together).
    At most 3 chain-iterations may fall under that exclusion; accepted and refused moves, a proposal outside the prior's support,
    an accepted and a refused swap must all occur.

    What was chosen on the host-driven engine alone (its walk does not depend on the device engine).  With the default proposal
    law NO proposal leaves the prior's support: seeds 0..399 over 60 iterations each (seed 5 first) gave none -- the period
    spacing's initial error is 0.002 against a support of +-1, and the nearest edge of any other support is Hfactor's and Wfactor's
    (0.9 under [0, 1], initial error 0.02: five standard deviations).  So this test, and no other, starts BOTH engines with Hfactor's
    initial error at 0.1 instead of 0.02; everything else is the default.  Seeds 5, 1, 2, 3 were then tried over 60 iterations:
    all four walks hold every event (first proposal outside the support at iteration 32 / 14 / 7 / 9) and no knife-edge
    comparator among their first 25 iterations; seed 2 holds them all within 25 iterations (first accepted move at iteration 2,
    swap 1, refused swap 2, outside 7)."""
    from tamcmc_c_amd.sampler import default_errors
    errors = default_errors(star)
    free = [star.names[i] for i in np.flatnonzero(star.relax == 1)]
    errors[free.index("Hfactor")] = WALK_HFACTOR_ERROR
    kw = dict(KW, seed=WALK_SEED, dN_mixing=1, init_errors=errors)
    host = pkg.Sampler(ctx_on, star, engine="host", **kw)
    dev = pkg.Sampler(ctx_on, star, engine="device", **kw)
    seen = dict(accepted=0, refused=0, outside=0, swapped=0, kept=0)
    knife_total, dprop_max = 0, 0.0
    vars_now = host.state()["vars"].copy()
    for k in range(WALK_ITER):
        host.set_state(vars_now, iteration=k)
        dev.set_state(vars_now, iteration=k)
        before = host.state()
        _, u, _, ind_A = host.draws(k)
        sh, th = host.run(1, stats=True)
        sd, td = dev.run(1, stats=True)
        ah, ad = host.state(), dev.state()
        assert ah["iteration"] == k + 1 and ad["iteration"] == k + 1
        ph, stat_h, _, _ = host.last_test()
        pd, _, _, gd = dev.last_test()
        step = np.linalg.norm(ph - vars_now, axis=1)
        dprop = np.max(np.linalg.norm(pd - ph, axis=1) / step)
        dprop_max = max(dprop_max, dprop)
        assert dprop < 2e-6, (k, dprop)
        g_direct, gp_direct, _ = _direct(ctx_on, star, dev, pd)
        _same_gradient(gd, g_direct, gp_direct, "iteration %d: gradient at the proposals" % k)
        swapped = ah["swaps"] - before["swaps"]
        assert ah["swap_attempts"] - before["swap_attempts"] == (1 if k else 0)
        r = ah["Pmove"].copy()
        if swapped:
            r[[ind_A, ind_A + 1]] = r[[ind_A + 1, ind_A]]             # Pmove travels with the rows
        knife = np.abs(r - u) < 5e-3 * r
        if k and (knife[ind_A] or knife[ind_A + 1]):
            knife[[ind_A, ind_A + 1]] = True
        knife_total += int(knife.sum())
        c = np.flatnonzero(~knife)
        assert np.allclose(ad["vars"][c], ah["vars"][c], rtol=1e-9, atol=0), k
        assert np.allclose(sd[0][c], sh[0][c], rtol=1e-9, atol=0), k
        assert np.allclose(td[0][c], th[0][c], rtol=1e-9, atol=0), k
        for key in ("logL", "logPrior", "logPost"):
            assert np.allclose(ad[key][c], ah[key][c], rtol=1e-9, atol=0), (k, key)
        if not knife.any():
            assert ad["swaps"] == ah["swaps"] and ad["accepted0"] == ah["accepted0"]
        acc = u <= r
        seen["accepted"] += int(acc.sum())
        seen["refused"] += int((~acc).sum())
        seen["outside"] += int(np.sum(stat_h[:, 1] == -np.inf))
        seen["swapped"] += int(swapped)
        seen["kept"] += int(k > 0 and not swapped)
        vars_now = ah["vars"].copy()
    print("\nwalk: largest proposal difference %.3e of the step, knife-edge exclusions %d of %d, %s" % (dprop_max, knife_total, NCH * WALK_ITER, seen))
    assert knife_total <= 3
    assert all(v >= 1 for v in seen.values()), seen
    host.close()
    dev.close()


def test_other_users_of_the_context_in_between(pkg, star, ctx_on):
    """The pre-step workspace belongs to the context: a direct gradient call of another batch size and a random-walk device sampler
    of another chain count run between two calls of the Langevin sampler, whose records stay those of an undisturbed run."""
    ref = pkg.Sampler(ctx_on, star, engine="device", **KW)
    smp, stt = ref.run(20, stats=True)
    ref.close()
    s = pkg.Sampler(ctx_on, star, engine="device", **KW)
    rw = pkg.Sampler(ctx_on, star, engine="device", **dict(KW, use_drift=0, nchains=4))
    s1, t1 = s.run(10, stats=True)
    P = np.tile(star.params, (5, 1))
    P[1:, star.index_to_relax] *= 1 + 1e-3 * np.random.default_rng(2).standard_normal((4, star.index_to_relax.size))
    _, _, g = ctx_on.fd_gradient_posterior(star, P, 1e-7 * np.maximum(np.abs(star.params[star.index_to_relax]), 1e-3), 1.3 ** np.arange(5))
    assert g.shape == (5, star.index_to_relax.size) and np.isfinite(g).all()
    r_smp, _ = rw.run(5)
    assert np.isfinite(r_smp).all() and rw.state()["iteration"] == 5
    s2, t2 = s.run(10, stats=True)
    assert np.array_equal(np.concatenate([s1, s2]), smp) and np.array_equal(np.concatenate([t1, t2]), stt)
    s.close()
    rw.close()


def test_refusals_leave_the_chain_alone(pkg, star, ctx_on):
    """STRICT (the host's long-double unpack cannot be had for proposals that live on the device) -> TAMCMC_ERR_BAD_ARG; the adjoint
    route (none for tables of variable length) -> TAMCMC_ERR_BAD_MODEL.  Neither touches the chains, which then continue bit for bit."""
    ref = pkg.Sampler(ctx_on, star, engine="device", **KW)
    smp, stt = ref.run(16, stats=True)
    ref.close()
    s = pkg.Sampler(ctx_on, star, engine="device", **KW)
    s1, t1 = s.run(6, stats=True)

    def snapshot():
        st = s.state()
        return [st["vars"], st["logL"], st["logPrior"], st["logPost"], np.array([st["iteration"], st["accepted0"], st["swap_attempts"], st["swaps"]]),
                s.gradient()[0]]

    try:
        for opt, value, restore, code in ((pkg.OPT_PRECISION, pkg.PRECISION_STRICT, pkg.PRECISION_FAST, pkg.ERR_BAD_ARG),
                                          (pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT, pkg.GRADIENT_FD, pkg.ERR_BAD_MODEL)):
            was = snapshot()
            ctx_on.set_option(opt, value)
            with pytest.raises(pkg.TamcmcError) as e:
                s.run(3)
            assert e.value.code == code
            now = snapshot()
            ctx_on.set_option(opt, restore)
            assert all(np.array_equal(x, y) for x, y in zip(was, now))
            assert now[4][0] == 6 and s.info()["iter_lockstep"] == 6
    finally:
        ctx_on.set_option(pkg.OPT_PRECISION, pkg.PRECISION_FAST)
        ctx_on.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_FD)
    s2, t2 = s.run(10, stats=True)
    assert np.array_equal(np.concatenate([s1, s2]), smp) and np.array_equal(np.concatenate([t1, t2]), stt)
    s.close()


@pytest.mark.parametrize("k", range(5))
def test_langevin_iteration_equals_the_oracle(pkg, oracle, star, ctx_on, k):
    """oracle/sampler_oracle.c::orc_langevin_iteration (any model id, prior class 4) through the helper of tests/test_gpu_sampler_oracle.py
    with its stated tolerances unchanged: the five iterations 0..4 from the start point, each checked in a case of its own (the oracle
    takes 3.3 s per iteration of this star; the k iterations before the checked one run unchecked -- a second call continues the
    chain bit for bit, test_same_call_twice_and_a_second_call_continues).  Iteration 0 has no swap step; 1..4 have one and it is
    accepted in each.  The precondition: the host-driven engine passes the same five on this star (measured on the MI355X: proposals
    within 9.1e-9 of the step's length, log-posteriors within 1.7e-16, move probabilities within 2.4e-6; the device engine's figures
    are the same to the digits printed)."""
    from test_gpu_sampler_oracle import _one_langevin_iteration_against_oracle
    s = pkg.Sampler(ctx_on, star, engine="device", **dict(KW, dN_mixing=1))
    init_logL = s.state()["logL"].copy()
    if k:
        s.run(k, record=False)
    rep = []
    exp, _ = _one_langevin_iteration_against_oracle(oracle, star, star.y, T, s, init_logL, False, 10.0, 1e-7, 0.0, rep)
    print("\ndevice engine against the oracle: it learn moved swapped dprop dlogPost dPmove  %6d %d %3d %d  %.2e %.2e %.2e" % rep[0])
    assert rep[0][0] == k and bool(exp["swapped"]) == (k > 0)
    s.close()

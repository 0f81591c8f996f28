"""Langevin step of the Gaussian-envelope fits (ids 0 / 1) on the device-resident engine, opt-in through
TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN (csrc/dev_sampler.hip: DevSampler::init / RunCall::run_mala; csrc/dev_mala_impl.h: k_env_mala_front,
k_env_mala_chain, the READY instantiations of k_mala_test / k_mala_ginit; csrc/envelope.hip: envelope_grad_stage_enqueue).

The sampler tests run on the star of tests/test_gpu_envelope_gradient.py::_sampler_star (1024 bins) with four chains at lambda_temp = 1.5;
the gradient tests on that file's _star (every parameter relaxed: 10 / 19 variables) with three chains at lambda_temp = 2.5 and the sizes
around the tile edge (1023, 1024, 1025), two bins, and 4097 bins (the chunk edge of id 0's xi pass).  One context per model id with
options 17 (the feature) and 15 (the host routes' analytic gradient, which the direct calls and the host-driven engine are compared
through) at 1."""
import math

import mpmath as mp
import numpy as np
import pytest

import envelope_chain_rule as cr
import envelope_grad_numpy as gn
from mc_stats import compare_chains
from test_gpu_envelope_gradient import _reference, _sampler_star, _star

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
NCH, LAM = 4, 1.5
T4 = np.array([math.pow(LAM, m) for m in range(NCH)])
KW = dict(nchains=NCH, lambda_temp=LAM, use_drift=1, seed=5, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,))
NCG, LAMG = 3, 2.5
TG = np.array([math.pow(LAMG, m) for m in range(NCG)])
KWG = dict(KW, nchains=NCG, lambda_temp=LAMG)
NX_GRAD = (2, 1023, 1024, 1025, 4097)
# test 3: K of the likelihood share's bound K u_j, K = max(4, 4 r) capped at 64, r the worst ratio measured on the MI355X over the
# vectors of test 2 (see test_device_assembly_against_the_host's docstring)
R_MEASURED = 11.065      # id 0 at 2 bins; the other nine cases: 0.94 (id 0, 1025 bins), 0.32 (id 0, 4097 bins), 0 elsewhere
K_LIKE = min(64.0, max(4.0, 4.0 * R_MEASURED))
# test 6: seeds of the two engines per model id and the widened initial errors, chosen on the HOST-DRIVEN engine alone (see the docstring)
WALK_ITER = 25
WALK = {0: dict(seed=0, widen={"N0": 2.0}), 1: dict(seed=0, widen={"tc2": 10.0})}


def _open(pkg, star, langevin=1, analytic=1):
    c = pkg.HipContext(0)
    c.set_spectrum(star.x, star.y)
    c.set_option(pkg.OPT_ENVELOPE_DEVICE_LANGEVIN, langevin)
    c.set_option(pkg.OPT_ENVELOPE_GRADIENT, analytic)
    return c


@pytest.fixture(scope="module")
def stars(synth):
    return {mid: _sampler_star(synth, mid) for mid in (0, 1)}


@pytest.fixture(scope="module")
def ctxs(pkg, stars):
    cs = {mid: _open(pkg, stars[mid]) for mid in (0, 1)}
    yield cs
    for c in cs.values():
        c.close()


def _full(star, vars_):
    P = np.tile(star.params, (vars_.shape[0], 1))
    P[:, star.index_to_relax] = vars_
    return P


def _steps(s):
    return 1e-7 * np.maximum(np.abs(s.get_proposal(0)[0]), 1e-3)      # the engine's steps: fd_step_rel max(|mu_0|, 1e-3)


def _direct(ctx, star, vars_, h, T):
    """fd_gradient_posterior (option 15 = 1: the host's long-double chain rule) at vars_ with the steps h: (grad, grad_prior, logL0, logPr0)."""
    l0, pr0, g = ctx.fd_gradient_posterior(star, _full(star, vars_), h, Tcoefs=T)
    return g, ctx.last_grad_prior.copy(), l0, pr0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return cr.build(tmp_path_factory.mktemp("envchain_gpu"))


def _replay(exe, s, star, T):
    """The host's long-double chain rule (tests/envelope_chain_rule_driver.cpp, "l": the text the host's gradient entries run) on what the
    device's own chain rule started from -- the folded sums and the rows of the sampler's last batch, read through the two audit entries.
    Returns (dlogL/dtheta [C x Nvars] in long double, tempered; u [C x Nvars], u_j = 2^-53 (p / T) sum_q |dS/drow_q J_qj|)."""
    _, tile, xi = s.envelope_gradient_sums()
    rows = s.envelope_rows()
    G, M, _ = cr.run(exe, "l", star.model_id, rows["params"][:, :(19 if star.model_id == 0 else 10)], float(star.x[1] - star.x[0]), tile, xi, rows["rows"])
    idx = star.index_to_relax
    Tl = np.asarray(T, dtype=np.float64).astype(cr.LD)[:, None]
    with np.errstate(invalid="ignore"):
        return -G[:, idx] / Tl, (EPS * M[:, idx] / Tl).astype(np.float64)


def _budget(star, vars_, T):
    """B_j (include/tamcmc_hip.h) of the likelihood's share at vars_, tempered: p B_j / T [C x Nvars]."""
    P = _full(star, vars_)
    B = np.array([np.asarray(gn.gradient_and_budget(star.model_id, p, star.x, star.y)[1], dtype=np.float64) for p in P])
    return B[:, star.index_to_relax] / np.asarray(T)[:, None]


def _prior_bound(g_like, gp):
    """tests/test_gpu_rgb_device_langevin.py::_assembly_bound: 4 x 2^-53 per component for the prior's share and the final sum."""
    return 4 * EPS * (np.abs(g_like) + np.abs(gp))


def _same_assembly(g, g_like_host, gp, u, what, K=K_LIKE):
    """The device's gradient against the host's long-double chain rule on the same sums and rows plus the prior's share: K u_j for
    the likelihood's share, _prior_bound for the rest.  Where the host's is not finite the device holds 0 (mala_gradient's rule).
    Returns the worst (|d| - the prior's bound) / u_j: the r of test 3."""
    want = (g_like_host + gp.astype(cr.LD))
    fin = np.isfinite(want.astype(np.float64)) & np.isfinite(u)
    assert np.all(g[~fin] == 0.0), what
    d = np.abs(g.astype(cr.LD) - want).astype(np.float64)
    prior = _prior_bound(g_like_host.astype(np.float64), gp)
    live = fin & (u > 0)
    r = float(np.max((np.maximum(d - prior, 0.0)[live]) / u[live], initial=0.0))
    print("\n%s: %d of %d components differ, worst (|d| - prior's bound) / u_j = r = %.3f (K = %.0f)" % (what, np.count_nonzero(d[fin]), int(fin.sum()), r, K))
    assert np.all(d[fin] <= (K * u + prior)[fin]), (what, r)
    assert np.all(g[fin & (u == 0) & (gp == 0)] == 0.0), what
    return r


def _close_to_direct(g, g_direct, gp_direct, budget, what):
    """The device's gradient against the direct call's at the same vectors.  The direct call builds its rows on the host (libm), the
    sampler on the device: a row field may differ in its last bit, and with it every bin's model, so the two are two evaluations of
    the same derivative, each within B_j of it (the header's gate: test 2 here, tests/test_gpu_envelope_gradient.py there): 2 p B_j / T
    apart at most, plus the prior's share (the same statements on the same doubles) at _prior_bound.  The worst ratio is printed."""
    fin = np.isfinite(g_direct)
    assert np.all(g[~fin] == 0.0), what
    d = np.abs(g - g_direct)
    bound = 2 * budget + _prior_bound(g_direct - gp_direct, gp_direct)
    print("\n%s: worst |d| / (2 p B_j / T + prior's bound) = %.3e" % (what, np.max((d / np.maximum(bound, 1e-300))[fin], initial=0.0)))
    assert np.all(d[fin] <= bound[fin]), what


# ------------------------------------------------------------------------------------------------------------------ 1. gate
def test_gate(pkg, synth, stars, ctxs):
    """Fails without the feature: the option does not exist (TAMCMC_ERR_BAD_ARG) and the constructor ends in TAMCMC_ERR_BAD_MODEL."""
    assert pkg.OPT_ENVELOPE_DEVICE_LANGEVIN == 17
    for mid in (0, 1):
        star, ctx = stars[mid], ctxs[mid]
        ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_LANGEVIN, 0)
        ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_LANGEVIN, 1)
        with pytest.raises(pkg.TamcmcError) as e:
            ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_LANGEVIN, 2)
        assert e.value.code == pkg.ERR_BAD_ARG
        s = pkg.Sampler(ctx, star, engine="device", **KW)
        i0 = s.info()
        assert i0["engine"] == 1 and i0["fused_available"] == 0 and i0["iter_lockstep"] == 0
        smp, stt = s.run(5, stats=True)
        i1 = s.info()
        assert i1["iter_lockstep"] == 5 and i1["iter_fused"] == 0 and s.state()["iteration"] == 5
        assert np.isfinite(smp).all() and np.isfinite(stt).all()
        with pytest.raises(pkg.TamcmcError) as e:                      # 17 alone does not admit the random walk
            pkg.Sampler(ctx, star, engine="device", **dict(KW, use_drift=0))
        assert e.value.code == pkg.ERR_BAD_MODEL
        ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_LANGEVIN, 0)            # read at creation: the existing sampler goes on
        try:
            s.run(2)
            assert s.state()["iteration"] == 7 and s.info()["iter_lockstep"] == 7
            for opt in (None, pkg.OPT_ENVELOPE_DEVICE_ENGINE, pkg.OPT_RGB_DEVICE_LANGEVIN):    # with 0: today's refusal, whatever 13 or 11 say
                if opt is not None:
                    ctx.set_option(opt, 1)
                with pytest.raises(pkg.TamcmcError) as e:
                    pkg.Sampler(ctx, star, engine="device", **KW)
                assert e.value.code == pkg.ERR_BAD_MODEL
                if opt is not None:
                    ctx.set_option(opt, 0)
        finally:
            ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_LANGEVIN, 1)
        s.close()
    ms = synth.make_c2_star()                                          # a main-sequence star on a context with the option
    cms = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    try:
        cms.set_spectrum(ms.x, np.ones_like(ms.x))
        cms.set_option(pkg.OPT_ENVELOPE_DEVICE_LANGEVIN, 1)
        s = pkg.Sampler(cms, ms, engine="device", **dict(KW, nchains=3))
        s.run(2)
        assert s.info()["engine"] == 1 and s.info()["iter_lockstep"] == 2
        s.close()
    finally:
        cms.close()


# ------------------------------------------------------------------------------------ 2. and 3. the gradient at the proposals
@pytest.fixture(scope="module")
def proposals(pkg, synth, driver):
    """Per (model id, nx): one iteration from the start point on the device engine, then everything tests 2 and 3 compare, computed
    once: the proposals, the device's gradient there, the host's long-double chain rule replayed on the batch's own sums and rows with
    the units u_j, the direct call's gradient and the budget B_j at the proposals, the settled state."""
    cache = {}

    def get(model_id, nx):
        key = (model_id, nx)
        if key in cache:
            return cache[key]
        star = _star(synth, model_id, nx, seed=70 + model_id, mu=1.5 if model_id == 0 else 0.0)
        ctx = _open(pkg, star)
        try:
            s = pkg.Sampler(ctx, star, engine="device", **dict(KWG, dN_mixing=10**6))
            h = _steps(s)
            s.run(1)
            vp, _, _, gprop = s.last_test()
            st = s.state()
            rows = s.envelope_rows()
            S_dev, _, _ = s.envelope_gradient_sums()
            g_like_host, u = _replay(driver, s, star, TG)
            g_dir, gp_dir, _, pr_prop = _direct(ctx, star, vp, h, TG)
            _, _, l_state, pr_state = _direct(ctx, star, st["vars"], h, TG)
            ll_prop, _, _ = ctx.loglike_params_batch(model_id, _full(star, vp), star.plength, Tcoefs=TG)
            s.close()
        finally:
            ctx.close()
        cache[key] = dict(star=star, vp=vp, gprop=gprop, g_dir=g_dir, gp_dir=gp_dir, u=u, g_like_host=g_like_host, state=st, rows=rows, S_dev=S_dev,
                          l_state=l_state, pr_state=pr_state, pr_prop=pr_prop, ll_prop=ll_prop, budget=_budget(star, vp, TG))
        return cache[key]

    return get


@pytest.mark.parametrize("model_id", [0, 1])
@pytest.mark.parametrize("nx", NX_GRAD)
def test_gradient_at_the_proposals_against_the_50_digit_derivative(proposals, model_id, nx):
    """grad_prop of last_test() minus the prior's share (the direct call's at the same proposals and steps: the two run the same
    statements in double), un-tempered, within B_j of the derivative of S at vars_prop: the 50-digit one up to 1100 bins, the
    long-double yardstick above.  The gate and the references are tests/test_gpu_envelope_gradient.py's."""
    d = proposals(model_id, nx)
    star = d["star"]
    P = _full(star, d["vp"])
    assert np.isfinite(d["gprop"]).all()
    gl = d["gprop"] - d["gp_dir"]
    ref, bud = _reference(model_id, P, star.x, star.y, nx)
    worst = 0.0
    for c in range(NCG):
        for j in range(P.shape[1]):
            if bud[c][j] == 0:
                assert gl[c, j] == 0.0, (c, j, gl[c, j])               # a parameter the model does not read (id 0's p18): exactly 0
                continue
            dS = -mp.mpf(float(TG[c])) * mp.mpf(float(gl[c, j]))
            ratio = float(abs(dS - ref[c][j]) / mp.mpf(float(bud[c][j])))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (model_id, nx, c, j, gl[c, j], float(ref[c][j]), ratio)
    if model_id == 0:
        assert np.all(d["gprop"][:, 18] == d["gp_dir"][:, 18])
    print("\nid %d nx %d: device Langevin gradient at the proposals, worst |d dS/dtheta_j| / B_j = %.3e" % (model_id, nx, worst))
    # the audit entry: the rows of these proposals
    np.testing.assert_array_equal(d["rows"]["params"], P)


@pytest.mark.parametrize("model_id", [0, 1])
@pytest.mark.parametrize("nx", NX_GRAD)
def test_device_assembly_against_the_host(proposals, model_id, nx):
    """The device's chain rule in double against the host's in long double, on test 2's proposals.

    Likelihood's share: K u_j with u_j = 2^-53 (p / T) sum_q |dS/drow_q J_qj| and K = max(4, 4 r) capped at 64, r the worst ratio measured
    on the MI355X over these ten cases: r = 11.07 (id 0 at 2 bins, where every bin lies far above b_k and the ln b_k branch subtracts two
    nearly equal products; next 0.94 at id 0 / 1025 bins, 0.32 at id 0 / 4097 bins, 0 in the seven others, every id 1 case among them), so
    K = 44.3 (R_MEASURED, K_LIKE).  r counts what |d| exceeds the prior's bound by, in units of u_j.  The host's chain rule is the text the gradient entries run
    (env_grad_rows, env_row_jacobian, env_chain_contract in long double), compiled by g++ and fed what the device's chain rule started
    from: the folded sums and the rows of the sampler's own batch (tamcmc_sampler_get_envelope_gradient_sums, _get_envelope_rows).
    Prior's share and the final sum: tests/test_gpu_rgb_device_langevin.py::_assembly_bound, 4 x 2^-53 per component; the prior's share
    is the direct call's (fd_gradient_posterior with option 15 = 1 and the sampler's steps) at the same proposals.

    Why not fd_gradient_posterior for the likelihood's share as well: it builds its rows on the host (libm's log and pow), the sampler
    on the device, and a row field may differ in its last bit -- then every bin's model does, and the folded sums, which nearly
    cancel near the posterior's mode, differ by far more than their own last bits.  Measured that way on the MI355X the ratio is 0.000
    where the rows happen to agree (id 1 at 2, 1024 and 4097 bins) and 12 ... 490 where they do not: the rows' difference, not the chain
    rule's.  That comparison is kept with the bound it can carry, _close_to_direct's.

    logPrior of the settled state is k_env_prior's bits for the same vector.  logL: the proposal's S is within 1e-12 |S| of the batched
    evaluation's (the same kernels on rows that may differ in a last bit: the header's statement for the device engine), and the state of
    a chain that moved holds (-p S) / T of the batch's S bit for bit."""
    d = proposals(model_id, nx)
    star, st = d["star"], d["state"]
    tag = "id %d nx %d" % (model_id, nx)
    _same_assembly(d["gprop"], d["g_like_host"], d["gp_dir"], d["u"], tag + ": gradient at the proposals, device against host chain rule")
    _close_to_direct(d["gprop"], d["g_dir"], d["gp_dir"], d["budget"], tag + ": gradient at the proposals, device against the direct call")
    np.testing.assert_array_equal(d["rows"]["logprior"], d["pr_prop"])
    np.testing.assert_array_equal(st["logPrior"], d["pr_state"])
    ll_dev = -d["S_dev"] / TG
    assert np.all(np.abs(ll_dev - d["ll_prop"]) <= 1e-12 * np.abs(d["ll_prop"])), (ll_dev, d["ll_prop"])
    moved = np.all(st["vars"] == d["vp"], axis=1)
    np.testing.assert_array_equal(st["logL"][moved], ll_dev[moved])
    assert np.all(np.abs(st["logL"] - d["l_state"]) <= 1e-12 * np.abs(d["l_state"]))


# ------------------------------------------------------------------------------------------------------- 4. held gradient
@pytest.mark.parametrize("model_id", [0, 1])
def test_held_gradient_is_the_direct_gradient(pkg, stars, ctxs, model_id):
    """30 iterations without swaps: the gradient the sampler holds is the direct call's at state()["vars"] within the bound test 3 has
    for the direct call (_close_to_direct: the sums of a held gradient are gone, so the chain rule cannot be replayed; the prior's share
    within 4 x 2^-53).  With a swap every iteration a gradient that followed its position was re-tempered at most once per iteration:
    the existing bound 4 n 2^-53 (|g| + |g_prior|) is added, on the chains `valid` marks."""
    star, ctx, n = stars[model_id], ctxs[model_id], 30
    s = pkg.Sampler(ctx, star, engine="device", **dict(KW, dN_mixing=10**6))
    h = _steps(s)
    s.run(n)
    st = s.state()
    assert st["swap_attempts"] == 0
    g, gp, valid = s.gradient()
    assert valid.all()
    g_dir, gp_dir, l0, pr0 = _direct(ctx, star, st["vars"], h, T4)
    _close_to_direct(g, g_dir, gp_dir, _budget(star, st["vars"], T4), "id %d: held vs direct gradient, no swaps" % model_id)
    assert np.all(np.abs(gp - gp_dir) <= 4 * EPS * np.abs(gp_dir))
    assert np.all(np.abs(st["logL"] - l0) <= 1e-12 * np.abs(l0))
    np.testing.assert_array_equal(st["logPrior"], pr0)
    s.close()
    s = pkg.Sampler(ctx, star, engine="device", **dict(KW, dN_mixing=1))
    smp, stt = s.run(n, stats=True)
    assert np.isfinite(smp).all() and np.isfinite(stt).all()
    st = s.state()
    assert st["accepted0"] > 0 and st["swap_attempts"] == n - 1
    g, gp, valid = s.gradient()
    assert valid.any()
    g_dir, gp_dir, _, _ = _direct(ctx, star, st["vars"], h, T4)
    budget = _budget(star, st["vars"], T4)
    for m in np.flatnonzero(valid):
        bound = 4 * n * EPS * (np.abs(g_dir[m]) + np.abs(gp_dir[m])) + 2 * budget[m]
        print("\nid %d chain %d: held vs direct gradient with swaps, max |d| / bound %.3e" % (model_id, m, np.max(np.abs(g[m] - g_dir[m]) / np.maximum(bound, 1e-300))))
        assert np.all(np.abs(g[m] - g_dir[m]) <= bound), m
    s.close()


# ---------------------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("model_id", [0, 1])
def test_determinism_and_other_users_of_the_context(pkg, stars, ctxs, model_id):
    star, ctx = stars[model_id], ctxs[model_id]
    a = pkg.Sampler(ctx, star, engine="device", **KW)
    b = pkg.Sampler(ctx, star, engine="device", **KW)
    smp_a, stt_a = a.run(30, stats=True)
    smp_b, stt_b = b.run(30, stats=True)
    assert np.array_equal(smp_a, smp_b) and np.array_equal(stt_a, stt_b)          # the same seed twice
    assert len(np.unique(smp_a[:, 0, 0])) > 1                                    # (the chains moved)
    c = pkg.Sampler(ctx, star, engine="device", **KW)
    ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_ENGINE, 1)
    try:
        rw = pkg.Sampler(ctx, star, engine="device", **dict(KW, use_drift=0, nchains=5))
    finally:
        ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_ENGINE, 0)
    s1, t1 = c.run(12, stats=True)
    # between the two calls: a direct gradient call of another size and a random-walk device sampler of another chain count
    P = np.tile(star.params, (7, 1))
    P[1:, star.index_to_relax] *= 1 + 1e-3 * np.random.default_rng(2).standard_normal((6, star.index_to_relax.size))
    _, _, g = ctx.fd_gradient_posterior(star, P, 1e-7 * np.maximum(np.abs(star.params[star.index_to_relax]), 1e-3), Tcoefs=1.3 ** np.arange(7))
    assert g.shape == (7, star.index_to_relax.size) and np.isfinite(g).all()
    r_smp, _ = rw.run(8)
    assert np.isfinite(r_smp).all() and rw.state()["iteration"] == 8
    s2, t2 = c.run(18, stats=True)
    assert np.array_equal(np.concatenate([s1, s2]), smp_a) and np.array_equal(np.concatenate([t1, t2]), stt_a)   # 12 + 18 = 30
    assert c.state()["iteration"] == 30 and np.array_equal(c.state()["vars"], a.state()["vars"])
    for s in (a, b, c, rw):
        s.close()


# ------------------------------------------------------------------------------ 6. one iteration at a time against the host engine
def _walk_errors(star, widen):
    from tamcmc_c_amd.sampler import default_errors
    errors = default_errors(star)
    free = [star.names[i] for i in np.flatnonzero(star.relax == 1)]
    for name, value in widen.items():
        errors[free.index(name)] = value
    return errors


@pytest.mark.parametrize("learn", [False, True])
@pytest.mark.parametrize("model_id", [0, 1])
def test_one_iteration_at_a_time_against_the_host_engine(pkg, stars, ctxs, model_id, learn):
    """WALK_ITER iterations with a swap step every iteration (dN_mixing = 1), the same seed on both engines, the host-driven engine with
    option 15 = 1.  Before each iteration both engines get the host-driven engine's previous state (set_state: both recompute their
    gradients there), then one iteration each.  Once without adaptation, once with the learning window open over the whole walk; in
    the second run the host's proposal law is copied into the device sampler (get_proposal / set_proposal) before each iteration, and
    after the step mu and the covariance of the chains that are compared agree to rtol 1e-9.
      * proposals: within 2e-6 of the step's length, the outer bound tests/test_gpu_sampler_oracle.py states; the value is printed;
      * records after the test: positions and the three statistics to rtol 1e-9 for every chain whose comparator is not within
        5e-3 r of its move probability (a swap pair leaves together); at most 3 chain-iterations may fall under that exclusion;
      * an accepted and a refused move, an accepted and a refused swap and a proposal outside the prior's support must all occur.
    The seed and the widened initial errors (WALK) were chosen on the host-driven engine alone, whose walk does not depend on the
    device engine: the first of seeds 0..9 whose 25 iterations without adaptation hold every event and no knife-edge comparator.
    With the default initial errors no seed has a proposal outside the prior's support (seeds 0..9, both ids: 0 of 100 each), so ONE
    initial error is widened, as tests/test_gpu_rgb_device_langevin.py did -- id 0: N0's to 2.0 (support [0, 10 N0], N0 = 5), seed 0:
    48 accepted / 52 refused moves, 3 proposals outside, 18 swaps / 6 refused; id 1: tc2's to 10.0 (support [0, 100], tc2 = 29.6), seed 0:
    9 / 91, 2 outside, 16 / 8.  Also tried and passed over, seed 0 first: id 0 a2 60 (no seed with every event), a2 120 and a1 120 (one and
    ten accepted moves in a hundred); id 1 tc2 25 and B0 100 (two and four accepted), tc1 40 (seed 0 lacks an event, seed 1 has all)."""
    star, ctx = stars[model_id], ctxs[model_id]
    kw = dict(KW, seed=WALK[model_id]["seed"], dN_mixing=1, init_errors=_walk_errors(star, WALK[model_id]["widen"]))
    if learn:
        kw.update(Nt_learn=(0, 10**6), periods_learn=(1,))
    host = pkg.Sampler(ctx, star, engine="host", **kw)
    dev = pkg.Sampler(ctx, star, engine="device", **kw)
    seen = dict(accepted=0, refused=0, outside=0, swapped=0, kept=0)
    knife_total, dprop_max = 0, 0.0
    vars_now = host.state()["vars"].copy()
    for k in range(WALK_ITER):
        host.set_state(vars_now, iteration=k)
        dev.set_state(vars_now, iteration=k)
        if learn:
            sig = host.state()["sigma"]
            for m in range(NCH):
                mu, cov = host.get_proposal(m)
                dev.set_proposal(m, mu, cov, sig[m])
        before = host.state()
        _, u, _, ind_A = host.draws(k)
        sh, th = host.run(1, stats=True)
        sd, td = dev.run(1, stats=True)
        ah, ad = host.state(), dev.state()
        assert ah["iteration"] == k + 1 and ad["iteration"] == k + 1
        ph, stat_h, _, _ = host.last_test()
        pd, _, _, _ = dev.last_test()
        step = np.linalg.norm(ph - vars_now, axis=1)
        dprop = np.max(np.linalg.norm(pd - ph, axis=1) / step)
        dprop_max = max(dprop_max, dprop)
        assert dprop < 2e-6, (k, dprop)
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
        if learn:
            mu_h, cov_h, sig_h = host.proposal_law()
            mu_d, cov_d, sig_d = dev.proposal_law()
            assert np.allclose(mu_d[c], mu_h[c], rtol=1e-9, atol=0), k
            assert np.allclose(cov_d[c], cov_h[c], rtol=1e-9, atol=0), k
            assert np.allclose(sig_d[c], sig_h[c], rtol=1e-9, atol=0), k
        acc = u <= r
        seen["accepted"] += int(acc.sum())
        seen["refused"] += int((~acc).sum())
        seen["outside"] += int(np.sum(stat_h[:, 1] == -np.inf))
        seen["swapped"] += int(swapped)
        seen["kept"] += int(k > 0 and not swapped)
        vars_now = ah["vars"].copy()
    print("\nid %d learn %d walk: largest proposal difference %.3e of the step, knife-edge exclusions %d of %d, %s"
          % (model_id, learn, dprop_max, knife_total, NCH * WALK_ITER, seen))
    assert knife_total <= 3
    if not learn:
        assert all(v >= 1 for v in seen.values()), seen
    host.close()
    dev.close()


# ----------------------------------------------------------------------------------------- 7. refusals leave the chain alone
@pytest.mark.parametrize("model_id", [0, 1])
def test_refusals_leave_the_chain_alone(pkg, stars, ctxs, model_id):
    """TAMCMC_GRADIENT_ADJOINT (no mode table, so no table-space adjoint) -> TAMCMC_ERR_BAD_MODEL before anything is enqueued: state,
    counters and the held gradient stay, and the chains then continue bit for bit."""
    star, ctx = stars[model_id], ctxs[model_id]
    ref = pkg.Sampler(ctx, star, engine="device", **KW)
    smp, stt = ref.run(16, stats=True)
    ref.close()
    s = pkg.Sampler(ctx, star, engine="device", **KW)
    s1, t1 = s.run(6, stats=True)

    def snapshot():
        st = s.state()
        g, gp, valid = s.gradient()
        return [st["vars"], st["logL"], st["logPrior"], st["logPost"], np.array([st["iteration"], st["accepted0"], st["swap_attempts"], st["swaps"]]), g, gp, valid]

    was = snapshot()
    ctx.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT)
    try:
        with pytest.raises(pkg.TamcmcError) as e:
            s.run(3)
        assert e.value.code == pkg.ERR_BAD_MODEL
        now = snapshot()
    finally:
        ctx.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_FD)
    assert all(np.array_equal(x, y) for x, y in zip(was, now))
    assert now[4][0] == 6 and s.info()["iter_lockstep"] == 6 and now[7].all()
    s2, t2 = s.run(10, stats=True)
    assert np.array_equal(np.concatenate([s1, s2]), smp) and np.array_equal(np.concatenate([t1, t2]), stt)
    s.close()


# ------------------------------------------------------------------------------------------------------------ 8. posterior
def _chain0(pkg, star, engine, n, seed):
    ctx = _open(pkg, star)
    try:
        s = pkg.Sampler(ctx, star, nchains=4, lambda_temp=1.5, seed=seed, use_drift=1, Nt_learn=(200, 1000, 3000), periods_learn=(1, 5),
                        target_acceptance=0.574, engine=engine)
        s.run(3000, record=False)
        smp, _ = s.run(n, record=True)
        s.close()
    finally:
        ctx.close()
    return smp[:, 0, :]


@pytest.mark.parametrize("model_id", [0, 1])
def test_posterior_against_the_host_langevin_sampler(pkg, stars, model_id):
    """Chain 0 of the device Langevin sampler (seed 4) against chain 0 of the host-driven one with option 15 = 1 (seed 3): the criterion
    of tests/test_gpu_envelope_gradient.py::test_langevin_posterior_with_and_without_the_option, |z| < 5 on means and variances from
    compare_chains, at that test's settings (target acceptance 0.574, Nt_learn (200, 1000, 3000), 6000 recorded iterations after 3000;
    its control of 15 host pairs lies below 3.5)."""
    star = stars[model_id]
    host = _chain0(pkg, star, "host", 6000, seed=3)
    dev = _chain0(pkg, star, "device", 6000, seed=4)
    zm, zv, ea, eb = compare_chains(host, dev)
    print("\nid %d: device against host Langevin, max |z| of the means %.2f, of the variances %.2f" % (model_id, np.abs(zm).max(), np.abs(zv).max()))
    assert np.all(np.abs(zm) < 5.0), (zm, ea, eb)
    assert np.all(np.abs(zv) < 5.0), (zv, ea, eb)

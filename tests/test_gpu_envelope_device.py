"""Gaussian-envelope fits (model ids 0 = model_Kallinger2014_Gaussian, 1 = model_Harvey_Gaussian) on the device-resident engine, opt-in
through TAMCMC_OPT_ENVELOPE_DEVICE_ENGINE (-m gpu).

Two routes run these chains (csrc/dev_sampler.hip, (C)): the lockstep kernels (k_iterate -> k_env_ksi / k_env_eval, every learning
iteration and every spectrum above 32 768 bins -- 6 144 for id 0 --) and the one-launch step k_env_step (quiet stretches of three iterations or more).

    test_creation                               the option table of tamcmc_sampler.h; fails without the feature
    test_bookkeeping_against_the_restatement    300 recorded iterations across learning and frozen stretches: every record against
                                                tests/envelope_numpy.py (logL, 1e-12 |logL|) and the 50-digit prior reference
    test_rows                                   get_envelope_rows field by field against the same expression in long double
    test_one_launch_equals_lockstep             automatic routing against OPT_STEP_SCHEME = 1, and chain groups 1 / 2 / 3: array_equal
    test_timing_option_changes_no_chain         TAMCMC_OPT_TIMING on both routes: times reported, same chains
    test_device_follows_host                    same seed, no adaptation: only a knife-edge decision may separate the engines
    test_dead_priors                            a proposal law wide enough to leave the uniform priors
    test_routing_limit                          32 769 bins: lockstep only; 32 768: the one-launch step (id 0, whose limit is the measured
                                                crossover of 6 144 bins: 6 145 and 6 144)
    test_posterior_device_vs_host               id 1 at Monte-Carlo resolution

A mutation of k_env_step, built and run once against this module (not committed): every sibling tile, not tile 0 alone, adds to the
chain's move counter -> test_one_launch_equals_lockstep fails on the move counts ([81, 71, 83] against [67, 61, 76]).

Sizes: 1000 bins (one partial tile, one chunk), 2049 (a last tile of one bin), 4097 (a second chunk of one bin), 5400.

Rows tolerance: K 2^-52 |ref| with K = max(4, 4 r), r the worst ratio measured on the MI355X over both ids and all four sizes (the
convention of tests/test_gpu_sampler_reference.py); the test prints the r of its run.  Measured r = R_MEASURED below; a ratio above 64
is a bug, not a tolerance.
"""
import copy

import numpy as np
import pytest

import envelope_numpy as en
from envelope_row_reference import row_reference as _row_reference
from mc_stats import compare_chains

pytestmark = pytest.mark.gpu

SIZES = (1000, 2049, 4097, 5400)
TOL = 1e-12          # include/tamcmc_hip.h: logL of ids 0 / 1 against the reference
R_MEASURED = 1.79    # worst |field - long double| / (2^-52 |ref|) of test_rows on the MI355X
K_ROWS = max(4.0, 4.0 * R_MEASURED)
ROW_CAP = 64.0
NEVER = (10**9, 10**9 + 1)
_STARS = {}
_LOGL = {}
_PRIOR = {}


@pytest.fixture(scope="module")
def mods(pkg):
    from tamcmc_c_amd import sampler, synth
    return pkg, sampler, synth


def _star(synth, model_id, nx):
    """The synthetic star of tests/test_gpu_envelope.py::_synthetic, made once per (id, size) and left unchanged."""
    key = (model_id, nx)
    if key not in _STARS:
        import test_gpu_envelope as ge
        _STARS[key] = ge._synthetic(synth, model_id, nx=nx, seed=11 + model_id)
    return _STARS[key]


def _context(pkg, star, opt=1):
    ctx = pkg.HipContext(0)
    ctx.set_spectrum(star.x, star.y)
    ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_ENGINE, opt)
    return ctx


def _params(star, v):
    p = star.params.copy()
    p[star.index_to_relax] = v
    return p


def _ref_logl(star, key, v, T):
    k = (key, v.tobytes(), float(T))
    if k not in _LOGL:
        _LOGL[k] = float(en.loglike(star.model_id, _params(star, v), star.x, star.y, T=T)[0])
    return _LOGL[k]


def _ref_prior(star, key, v):
    import prior_reference as ref
    k = (key, v.tobytes())
    if k not in _PRIOR:
        _PRIOR[k] = ref.star_log_prior(star, _params(star, v))
    return _PRIOR[k]


def _check_records(synth, star, key, smp, stt, T):
    """Every recorded (iteration, chain): logL against the long-double restatement at the recorded variables and the chain's temperature,
    logPost = logL + logPrior exactly, logPrior against the 50-digit reference at the tolerance of tests/test_gpu_priors.py."""
    import prior_cases as pc
    K = pc.device_K(synth)
    worst_l = worst_p = 0.0
    for i in range(smp.shape[0]):
        for m in range(smp.shape[1]):
            L = _ref_logl(star, key, smp[i, m], T[m])
            assert np.isfinite(stt[i, m]).all(), (i, m, stt[i, m])
            dl = abs(stt[i, m, 0] - L)
            worst_l = max(worst_l, dl / abs(L))
            assert dl <= TOL * abs(L), (i, m, stt[i, m, 0], L)
            assert stt[i, m, 2] == stt[i, m, 0] + stt[i, m, 1], (i, m, stt[i, m])
            r = _ref_prior(star, key, smp[i, m])
            assert r.failed is None, (i, m, r.failed)
            dp = abs(stt[i, m, 1] - float(r.value))
            worst_p = max(worst_p, dp / (2.0 ** -52 * float(r.scale)))
            assert dp <= pc.tol_prior(r, K), (i, m, stt[i, m, 1], float(r.value), dp, pc.tol_prior(r, K))
    return worst_l, worst_p


# ---------------------------------------------------------------- creation
@pytest.mark.parametrize("model_id", [0, 1])
def test_creation(mods, model_id):
    pkg, sampler, synth = mods
    star = _star(synth, model_id, 1000)
    ctx = _context(pkg, star, opt=0)
    try:
        with pytest.raises(pkg.TamcmcError) as e:
            sampler.Sampler(ctx, star, nchains=3, engine="device")
        assert e.value.code == pkg.ERR_BAD_MODEL
        with pytest.raises(pkg.TamcmcError) as e:
            sampler.Sampler(ctx, star, nchains=3, engine="device", use_drift=1)
        assert e.value.code == pkg.ERR_BAD_MODEL
        ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_ENGINE, 1)
        with pytest.raises(pkg.TamcmcError) as e:
            sampler.Sampler(ctx, star, nchains=3, engine="device", use_drift=1)
        assert e.value.code == pkg.ERR_BAD_MODEL
        s = sampler.Sampler(ctx, star, nchains=3, engine="device")
        info = s.info()
        assert info["engine"] == 1 and info["fused_available"] == 1 and info["iter_fused"] == 0 and info["iter_lockstep"] == 0
        with pytest.raises(pkg.TamcmcError) as e:
            s.tables()
        assert e.value.code == pkg.ERR_BAD_MODEL
        with pytest.raises(pkg.TamcmcError) as e:
            s.envelope_rows()                                         # nothing has run yet
        assert e.value.code == pkg.ERR_BAD_ARG
        ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_ENGINE, 0)             # read at creation: the existing sampler goes on
        s.run(5, record=False)
        assert s.state()["iteration"] == 5
        with pytest.raises(pkg.TamcmcError) as e:
            sampler.Sampler(ctx, star, nchains=3, engine="device")
        assert e.value.code == pkg.ERR_BAD_MODEL
        h = sampler.Sampler(ctx, star, nchains=3, engine="host")      # the host engine never depended on it
        with pytest.raises(pkg.TamcmcError) as e:
            h.envelope_rows()
        assert e.value.code == pkg.ERR_BAD_MODEL
        h.close()
        s.close()
        with pytest.raises(pkg.TamcmcError):
            ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_ENGINE, 2)
    finally:
        ctx.close()


# ---------------------------------------------------------------- bookkeeping
@pytest.mark.parametrize("nx", SIZES)
@pytest.mark.parametrize("model_id", [0, 1])
def test_bookkeeping_against_the_restatement(mods, model_id, nx):
    pkg, sampler, synth = mods
    star = _star(synth, model_id, nx)
    ctx = _context(pkg, star)
    try:
        s = sampler.Sampler(ctx, star, nchains=4, lambda_temp=1.5, seed=7, Nt_learn=(50, 100, 300), periods_learn=(1, 5), dN_mixing=1,
                            engine="device")
        smp, stt = s.run(300, stats=True)
        info = s.info()
        s.close()
    finally:
        ctx.close()
    assert info["iter_fused"] > 0 and info["iter_lockstep"] > 0 and info["iter_fused"] + info["iter_lockstep"] == 300, info
    assert info["fused_stretches"] > 1 and info["quick_fallbacks"] == info["quick_sure"] == info["quick_mismatch"] == 0, info
    assert (smp[-1] != smp[0]).any()
    wl, wp = _check_records(synth, star, (model_id, nx), smp, stt, 1.5 ** np.arange(4))
    print("\nid %d, %d bins: worst |dlogL| / |logL| = %.2e, worst prior error = %.2f x 2^-52 scale" % (model_id, nx, wl, wp))


# ---------------------------------------------------------------- rows
@pytest.mark.parametrize("nx", SIZES)
@pytest.mark.parametrize("model_id", [0, 1])
def test_rows(mods, model_id, nx):
    import prior_cases as pc
    import prior_reference as ref
    pkg, sampler, synth = mods
    star = _star(synth, model_id, nx)
    K = pc.device_K(synth)
    ctx = _context(pkg, star)
    worst, moved = 0.0, 0
    try:
        s = sampler.Sampler(ctx, star, nchains=4, lambda_temp=1.5, seed=5, Nt_learn=NEVER, periods_learn=(1,), engine="device")
        fixed = star.relax != 1
        for it in range(12):
            s.run(1, record=False)
            er = s.envelope_rows()
            assert er["rows"].shape == (4, len(s.ENVELOPE_ROW_FIELDS))
            for m in range(4):
                p = er["params"][m]
                assert np.array_equal(p[fixed], star.params[fixed])
                moved += int((p != star.params).any())
                want = _row_reference(model_id, p)
                for f, name in enumerate(s.ENVELOPE_ROW_FIELDS):
                    got, w = er["rows"][m, f], want[f]
                    if name.startswith("hon") or w == 0:
                        assert got == float(w), (it, m, name, got, w)
                        continue
                    ratio = float(abs(np.longdouble(got) - w) / (np.longdouble(2.0) ** -52 * abs(w)))
                    worst = max(worst, ratio)
                    assert ratio <= ROW_CAP, (it, m, name, got, float(w), ratio)
                    assert ratio <= K_ROWS, (it, m, name, got, float(w), ratio)
                r = ref.star_log_prior(star, p)
                assert er["status"][m] == 0
                if r.failed is not None:
                    assert er["logprior"][m] == -np.inf, (it, m, er["logprior"][m], r.failed)
                else:
                    assert abs(er["logprior"][m] - float(r.value)) <= pc.tol_prior(r, K), (it, m, er["logprior"][m], float(r.value))
        s.close()
    finally:
        ctx.close()
    assert moved >= 40          # the vectors are proposals, not the start
    print("\nid %d, %d bins: worst row field ratio r = %.2f (K = %.1f)" % (model_id, nx, worst, K_ROWS))


# ---------------------------------------------------------------- one launch = lockstep
def _run_scheme(pkg, sampler, ctx, star, scheme, groups, kw):
    ctx.set_option(pkg.OPT_STEP_SCHEME, scheme)
    d = sampler.Sampler(ctx, star, engine="device", chain_groups=groups, **kw)
    s1, t1 = d.run(60, stats=True)
    s2, t2 = d.run(31, stats=True)          # a second call continues the same chains
    st, mv, er, info = d.state(), d.move_counts(), d.envelope_rows(), d.info()
    d.close()
    return (s1, t1, s2, t2, st, mv, er), info


def _assert_same(a, b, what):
    for k in range(4):
        assert np.array_equal(a[k], b[k]), (what, "records", k)
    for k in a[4]:
        assert np.array_equal(a[4][k], b[4][k]), (what, "state", k)
    assert np.array_equal(a[5], b[5]), (what, "move counts")
    for k in a[6]:
        assert np.array_equal(a[6][k], b[6][k], equal_nan=True), (what, "rows", k)


@pytest.mark.parametrize("dN_mixing", [1, 3, 0])
@pytest.mark.parametrize("nchains", [3, 9])
@pytest.mark.parametrize("nx", [2049, 5400])
@pytest.mark.parametrize("model_id", [0, 1])
def test_one_launch_equals_lockstep(mods, model_id, nx, nchains, dN_mixing):
    """k_env_step against the lockstep kernels, with and without a learning window in the middle: samples, statistics, state, counters
    and the audit's rows bit for bit.  Nine chains on the lockstep route: 1, 2 and 3 chain groups (a swap pair that straddles two
    streams, the per-chain xi and tile slots) are the same chains too."""
    pkg, sampler, synth = mods
    star = _star(synth, model_id, nx)
    ctx = _context(pkg, star)
    try:
        for learn in (NEVER, (30, 50)):
            kw = dict(nchains=nchains, lambda_temp=1.4, seed=23, Nt_learn=learn, periods_learn=(2,), dN_mixing=dN_mixing)
            auto, ia = _run_scheme(pkg, sampler, ctx, star, 0, 0, kw)
            lock, il = _run_scheme(pkg, sampler, ctx, star, 1, 0, kw)
            assert ia["iter_fused"] > 0 and ia["iter_fused"] + ia["iter_lockstep"] == 91, ia
            assert (ia["iter_lockstep"] > 0) == (learn is not NEVER), ia
            assert il["iter_fused"] == 0 and il["iter_lockstep"] == 91, il
            _assert_same(auto, lock, (learn, "automatic vs lockstep"))
            assert auto[4]["swap_attempts"] == (0 if dN_mixing == 0 else len([i for i in range(1, 91) if i % dN_mixing == 0]))
            assert (auto[2][-1] != auto[0][0]).any()
            if nchains == 9:
                assert il["chain_groups"] == 2
                for g in (1, 3):
                    other, ig = _run_scheme(pkg, sampler, ctx, star, 1, g, kw)
                    assert ig["chain_groups"] == g and ig["iter_fused"] == 0
                    _assert_same(lock, other, (learn, "chain groups", g))
    finally:
        ctx.set_option(pkg.OPT_STEP_SCHEME, 0)
        ctx.close()


@pytest.mark.parametrize("model_id", [0, 1])
def test_timing_option_changes_no_chain(mods, model_id):
    """TAMCMC_OPT_TIMING brackets the envelope kernels of both routes with events (sampled lockstep launches, whole one-launch
    stretches): kernel time and evaluations are reported, the chains are the same bit for bit."""
    pkg, sampler, synth = mods
    star = _star(synth, model_id, 2049)
    kw = dict(nchains=9, lambda_temp=1.4, seed=29, Nt_learn=(30, 50), periods_learn=(2,), dN_mixing=1, engine="device")
    out = []
    for timing in (0, 1):
        ctx = _context(pkg, star)
        try:
            ctx.set_option(pkg.OPT_TIMING, timing)
            s = sampler.Sampler(ctx, star, **kw)
            out.append(s.run(91, stats=True))
            ms, launches, evals = ctx.kernel_stats()
            info = s.info()
            s.close()
        finally:
            ctx.close()
        if timing:
            assert ms > 0 and launches > 0 and evals >= 91 * 9, (ms, launches, evals)   # (+ the evaluations of the start positions)
            assert info["iter_fused"] > 0 and info["iter_lockstep"] > 0
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---------------------------------------------------------------- device follows host
def _first_divergence(sh, sd):
    same = np.all(np.isclose(sh, sd, rtol=1e-9, atol=1e-12), axis=tuple(range(1, sh.ndim)))
    return len(sh) if same.all() else int(np.argmin(same))


@pytest.mark.parametrize("model_id", [0, 1])
def test_device_follows_host(mods, model_id):
    """The pattern of tests/test_gpu_sampler.py::test_device_engine_follows_host_engine: the device's rows differ from the host's by ulps,
    so the trajectories agree to rounding until a knife-edge decision."""
    pkg, sampler, synth = mods
    star = _star(synth, model_id, 5400)
    ctx = _context(pkg, star)
    try:
        kw = dict(nchains=6, lambda_temp=1.5, seed=11, Nt_learn=NEVER, periods_learn=(1,), dN_mixing=1)
        h = sampler.Sampler(ctx, star, engine="host", **kw)
        d = sampler.Sampler(ctx, star, engine="device", **kw)
        n = 120
        sh, th = h.run(n, stats=True)
        sd, td = d.run(n, stats=True)
        first_div = _first_divergence(sh, sd)
        assert first_div >= 60, f"engines diverge at iteration {first_div}"
        assert np.allclose(th[:first_div], td[:first_div], rtol=1e-9, atol=0.0)
        a, b = h.state(), d.state()
        assert a["iteration"] == b["iteration"] == n
        assert a["swap_attempts"] == b["swap_attempts"] == n - 1
        assert (sh[:, 0] != sh[0, 0]).any()  # chain 0 moved
        assert d.info()["iter_fused"] == n
        h.close(); d.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- dead priors
def _walk(s, n):
    """n run(1) calls: Pmove, positions and stored logL after each."""
    pm, pos, ll = [], [], []
    for _ in range(n):
        s.run(1, record=False)
        st = s.state()
        pm.append(st["Pmove"].copy()); pos.append(st["vars"].copy()); ll.append(st["logL"].copy())
    return np.array(pm), np.array(pos), np.array(ll)


@pytest.mark.parametrize("model_id", [0, 1])
def test_dead_priors(mods, model_id):
    """Proposals that leave the uniform priors: log-prior -inf, the evaluation runs on whatever row that vector gives, and the test
    settles as on the host (Pmove = 0, position and logL kept)."""
    from tamcmc_c_amd.sampler import default_errors
    pkg, sampler, synth = mods
    star = _star(synth, model_id, 2049)
    ctx = _context(pkg, star)
    n, nc = 120, 4
    kw = dict(nchains=nc, lambda_temp=1.5, seed=31, Nt_learn=NEVER, periods_learn=(1,), dN_mixing=1)
    err = default_errors(star)
    try:
        found = None
        for f in (4.0, 8.0, 16.0, 32.0, 64.0):     # widened until the host engine, the reference here, meets both conditions
            h = sampler.Sampler(ctx, star, engine="host", **kw)
            for m in range(nc):
                h.set_proposal(m, cov=np.diag((f * err) ** 2))
            pm, pos, ll = _walk(h, n)
            h.close()
            dead, alive = float((pm == 0.0).mean()), float((pm > 0.0).mean())
            if dead >= 0.10 and alive >= 0.10:
                found = f
                break
        assert found is not None, (dead, alive)
        d = sampler.Sampler(ctx, star, engine="device", **kw)
        for m in range(nc):
            d.set_proposal(m, cov=np.diag((found * err) ** 2))
        pmd, posd, lld = _walk(d, n)
        assert d.info()["iter_lockstep"] == n
        d.close()
    finally:
        ctx.close()
    assert not np.isnan(lld).any() and not np.isnan(ll).any()
    first_div = _first_divergence(pos, posd)
    assert first_div >= 60, f"engines diverge at iteration {first_div}"
    assert np.array_equal(pm[:first_div] == 0.0, pmd[:first_div] == 0.0)
    assert np.allclose(pm[:first_div], pmd[:first_div], rtol=1e-6, atol=1e-300)   # (Pmove = exp of a difference of two logL of ~1e4)
    assert np.allclose(ll[:first_div], lld[:first_div], rtol=1e-9, atol=0.0)
    print("\nid %d: law widened %gx, host Pmove == 0 in %.0f%%, > 0 in %.0f%% of %d chain-iterations" % (model_id, found, 100 * dead, 100 * alive, n * nc))


# ---------------------------------------------------------------- routing limit
@pytest.mark.parametrize("model_id", [0, 1])
def test_routing_limit(mods, model_id):
    pkg, sampler, synth = mods
    limit = 32768 if model_id == 1 else 6144   # csrc/envelope_row.h: env_step_max_bins
    big = _star(synth, model_id, limit + 1)
    cut = copy.copy(big)
    cut.x, cut.y = big.x[:limit].copy(), big.y[:limit].copy()
    T = 1.5 ** np.arange(3)
    for star, key, fused in ((big, (model_id, limit + 1), False), (cut, (model_id, limit), True)):
        ctx = _context(pkg, star)
        try:
            s = sampler.Sampler(ctx, star, nchains=3, lambda_temp=1.5, seed=3, Nt_learn=NEVER, periods_learn=(1,), engine="device")
            s.run(15, record=False)
            smp, stt = s.run(5, stats=True)
            info = s.info()
            s.close()
        finally:
            ctx.close()
        assert info["fused_available"] == (1 if fused else 0)
        assert (info["iter_fused"] > 0) == fused and info["iter_fused"] + info["iter_lockstep"] == 20, info
        _check_records(synth, star, key, smp, stt, T)


# ---------------------------------------------------------------- posterior
def test_posterior_device_vs_host(mods):
    """Id 1, 5400 bins, the lengths of tests/test_gpu_envelope.py::test_posterior_recovers_injection_mh_vs_langevin."""
    pkg, sampler, synth = mods
    star = _star(synth, 1, 5400)
    out = {}
    for engine, seed in (("host", 3), ("device", 4)):
        ctx = _context(pkg, star)
        try:
            s = sampler.Sampler(ctx, star, nchains=4, lambda_temp=1.5, seed=seed, Nt_learn=(200, 1000, 3000), periods_learn=(1, 5), engine=engine)
            s.run(3000, record=False)
            smp, _ = s.run(12000, record=True)
            s.close()
        finally:
            ctx.close()
        out[engine] = smp[:, 0, :]
    zm, zv, ea, eb = compare_chains(out["host"], out["device"])
    assert np.all(np.abs(zm) < 5.0), (zm, ea, eb)
    assert np.all(np.abs(zv) < 5.0), (zv, ea, eb)

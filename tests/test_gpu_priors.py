"""Device log-prior against the 50-digit reference (tests/prior_reference.py) on the cases of tests/prior_cases.py (-m gpu).

The term sum of the log-prior is parallelised in four ways (csrc/dev_unpack.h, dev_step_impl.h, dev_iterate_impl.h, fd_batch.hip,
envelope.hip); each test says which of them it runs:
    path 1  wg_log_prior: un-split over the gradient batch's workgroup (k_fd_unpack) / split beside the helper waves (k_iterate);
    path 2  wave_log_prior_part, two single waves replaying the 128-lane layout (the fused step's role_prior);
    path 3  class 4: generic terms one per lane, then prior_serial on lane 0 (k_fd_rgb_perturb, k_iterate);
    path 4  k_env_prior, one thread per vector (classes 0 and 1).

Tolerance.  tol_prior = K 2^-52 scale, scale = sum over the additive terms of max(1, |term|) from the reference.  K = max(4, 4 r) with
r the largest |float64 restatement - reference| / (2^-52 scale) over all finite cases, measured on the CPU by the plain float64 run of the
reference's own formulas (prior_cases.measured_r): r = 7.26 and K = 29.0 when this was written (the 30-sigma Gaussian tails: terms of
-450 added left to right).  The factor 4 allows for another summation order and for device log / sqrt at 1-2 ulp.  tests/test_priors.py
asserts that this is not looser than what test_device_priors_match_host asserts on its own vectors.
"""
import copy
from decimal import Decimal

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(synth):
    import prior_cases
    z = prior_cases.zoo(synth)
    ex, _ = prior_cases.references(synth)
    return prior_cases, z, ex, prior_cases.device_K(synth)


@pytest.fixture()
def ctx(pkg):
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    yield c
    c.close()


def _give_spectrum(oracle, zoo, seed=5):
    """The spectrum only has to exist: the model of the start vector times Exp(1) noise."""
    star = zoo.star
    if star.y is not None:
        return star
    if star.model_id in (0, 1):
        import envelope_numpy as en
        m0 = np.asarray(en.model(star.model_id, star.params, star.x), dtype=np.float64)
    else:
        src = zoo.spectrum_of or star
        assert np.array_equal(src.x, star.x)
        _, m0 = oracle.call_model(src.model_id, src.params, src.plength, src.x)
    assert np.all(np.isfinite(m0)) and np.all(m0 > 0)
    star.set_spectrum_from_model(m0, seed)
    return star


def _check_values(name, labels, refs, got, K, pc):
    worst = 0.0
    for label, r, v in zip(labels, refs, got):
        if r.failed is not None:
            assert v == -np.inf, (name, label, v, r.failed)
            continue
        assert np.isfinite(v), (name, label, v)
        tol = pc.tol_prior(r, K)
        err = float(abs(Decimal(float(v)) - r.value))
        worst = max(worst, err / (2.0 ** -52 * float(r.scale)))
        assert err <= tol, (name, label, v, float(r.value), err, tol)
    return worst


@pytest.mark.parametrize("name", __import__("prior_cases").ZOO_NAMES)
def test_gradient_batch_prior_matches_reference(pkg, oracle, ctx, cases, name):
    """a. One fd_gradient_posterior call per star with all of its vectors as rows: pr0 against the reference.  Path 1 un-split (classes 2
    and 3: k_fd_unpack), path 3 (zoo_rgb: k_fd_rgb_perturb), path 4 (zoo_env0, zoo_env1: k_env_prior)."""
    pc, z, ex, K = cases
    zoo = z[name]
    star = _give_spectrum(oracle, zoo)
    ctx.set_spectrum(star.x, star.y)
    P = zoo.P
    _, pr0, _ = ctx.fd_gradient_posterior(star, P, zoo.fd_step(), np.ones(len(P)), 1.0)
    worst = _check_values(name, [c.label for c in zoo.cases], ex[name], pr0, K, pc)
    print("\n%s: %d vectors, worst |device - reference| = %.2f x 2^-52 scale (K = %.2f)" % (name, len(P), worst, K))


def _expected_prior_gradient(ref, star, row, i, h):
    """The prior's share for parameter i: forward difference where the forward point is finite, backward where only the backward point
    is, 0 where neither is; with the step actually applied.  Returns (value, step) as Decimals."""
    x0 = row[i]
    xp = np.float64(x0 + h)
    happ = Decimal(float(xp)) - Decimal(float(x0))
    r0 = ref.star_log_prior(star, row)
    assert r0.failed is None
    f = row.copy()
    f[i] = xp
    rp = ref.star_log_prior(star, f)
    if rp.failed is None:
        return (rp.value - r0.value) / happ, happ, "forward"
    f[i] = np.float64(x0 - h)
    rm = ref.star_log_prior(star, f)
    if rm.failed is None:
        return (r0.value - rm.value) / happ, happ, "backward"
    return Decimal(0), happ, "flat"


def _gradient_rows(pc, zoo):
    """Vectors 0.25 h inside an upper / a lower support edge of ids 1, 4, 8 and inside a constraint's edge; (label, row, parameter)."""
    star = zoo.star
    idx = star.index_to_relax
    h = dict(zip(idx, zoo.fd_step()))
    sw, pri = star.priors_switch, star.priors
    rows = []

    def row(label, i, v, **other):
        p = star.params.copy()
        for k, w in other.items():
            p[int(k[1:])] = w
        p[i] = v
        rows.append((label, p, i))

    for kind in (1, 4, 8):
        i = [j for j in idx if sw[j] == kind][0]
        lo, hi = (0.0, pri[1, i]) if kind == 4 else (pri[0, i], pri[1, i])
        row("id %d upper edge" % kind, i, hi - 0.25 * h[i])
        if kind != 8:
            row("id %d lower edge" % kind, i, lo + 0.25 * h[i])
    o = pc._offsets(star)
    if zoo.name == "zoo_global":     # |a_j/a1| < 0.2: a1_0 a quarter step above the largest |a_j| / 0.2 (the backward point breaks the limit)
        assert all(star.params[o[6] + 2 * j + 1] == 0 for j in range(6))
        crit = max(abs(star.params[o[6] + 2 * j]) / star.extra_priors[2 + j] for j in range(1, 6))
        row("a_j/a1 constraint edge, from inside", o[6], crit + 0.25 * h[o[6]])
    if zoo.name == "zoo_local":      # |a3| / (c^2 + s^2) < 0.2 with c < 0: the forward point (c towards 0) breaks the limit
        c, s, lim = o[6] + 3, o[6] + 4, star.extra_priors[2]
        a3 = 0.2
        c_edge = -np.sqrt(a3 / lim - star.params[s] ** 2)
        row("a3/a1 constraint edge, forward point outside", c, c_edge - 0.25 * h[c], **{"p%d" % (o[6] + 2): a3})
        row("id 8 lower edge from the negative side", s, -(pri[0, s] + 0.25 * h[s]))
    return rows


@pytest.mark.parametrize("name", ["zoo_global", "zoo_local"])
def test_prior_share_of_the_gradient(pkg, oracle, ctx, cases, name):
    """b. last_grad_prior of the gradient batch (path 1 un-split, forward AND backward evaluation of k_fd_unpack) at vectors a quarter of
    a step inside a support edge: the one-sided fallback must be taken exactly where the reference's forward point is outside."""
    import prior_reference as ref
    pc, z, ex, K = cases
    zoo = z[name]
    star = _give_spectrum(oracle, zoo)
    ctx.set_spectrum(star.x, star.y)
    rows = _gradient_rows(pc, zoo)
    idx, h = star.index_to_relax, zoo.fd_step()
    P = np.array([r[1] for r in rows])
    ctx.fd_gradient_posterior(star, P, h, np.ones(len(P)), 1.0)
    gp = ctx.last_grad_prior
    modes = set()
    for b, (label, p, i) in enumerate(rows):
        tol = Decimal(pc.tol_prior(ref.star_log_prior(star, p), K))
        cols = sorted(set([int(np.flatnonzero(idx == i)[0])] + list(range(0, idx.size, 8))))
        for k in cols:
            want, happ, mode = _expected_prior_gradient(ref, star, p, idx[k], h[k])
            if idx[k] == i:
                modes.add(mode)
            assert abs(Decimal(float(gp[b, k])) - want) <= 2 * tol / happ, (name, label, k, mode, gp[b, k], float(want), float(2 * tol / happ))
    assert {"forward", "backward"} <= modes


SAMPLER_KW = dict(lambda_temp=1.4, seed=23, Nt_learn=(10**9, 10**9 + 1), periods_learn=(2,), dN_mixing=1, engine="device")


def _records_match_reference(pc, name, star, smp, stt, K, cache):
    import prior_reference as ref
    idx = star.index_to_relax
    n = 0
    for k in range(smp.shape[0]):
        for m in range(smp.shape[1]):
            key = smp[k, m].tobytes()
            if key not in cache:
                p = star.params.copy()
                p[idx] = smp[k, m]
                cache[key] = ref.star_log_prior(star, p)
                n += 1
            r = cache[key]
            assert r.failed is None, (name, k, m, r.failed)            # an accepted vector has a finite prior
            err = float(abs(Decimal(float(stt[k, m, 1])) - r.value))
            assert err <= pc.tol_prior(r, K), (name, k, m, stt[k, m, 1], float(r.value), err)
    return n


@pytest.mark.parametrize("name,nchains,fused_scheme", [("zoo_global", 7, 0), ("zoo_small", 7, 0), ("zoo_local", 7, 0), ("zoo_v2", 7, 0),
                                                       ("zoo_rgb", 7, 0), ("zoo_global", 9, 3)])
def test_sampler_records_carry_the_reference_prior(pkg, oracle, ctx, cases, name, nchains, fused_scheme):
    """c. The device engine without adaptation, once on the lockstep kernels (k_iterate: path 1 split, 128 term lanes beside the helper
    waves; zoo_rgb: path 3) and once on the fused step (role_prior: path 2, two single waves): the logPrior of every record against the
    reference at that record's vector, and the two runs identical."""
    pc, z, ex, K = cases
    star = _give_spectrum(oracle, z[name])
    ctx.set_spectrum(star.x, star.y)
    n_iter = 80
    out, cache = [], {}
    for scheme in (1, fused_scheme):
        ctx.set_option(pkg.OPT_STEP_SCHEME, scheme)
        d = pkg.Sampler(ctx, star, nchains=nchains, **SAMPLER_KW)
        smp, stt = d.run(n_iter, stats=True)
        info = d.info()
        d.close()
        ctx.set_option(pkg.OPT_STEP_SCHEME, 0)
        if scheme == 1:
            assert info["iter_fused"] == 0
        elif info["fused_available"]:
            assert info["iter_fused"] == n_iter
        fresh = _records_match_reference(pc, name, star, smp, stt, K, cache)
        out.append((smp, stt))
        print("\n%s, scheme %d: %d distinct vectors checked, %d fused iterations" % (name, scheme, fresh, info["iter_fused"]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    moves = int((out[0][0][1:, 0] != out[0][0][:-1, 0]).any(axis=1).sum())
    assert moves >= 10, moves


BAD_IDS = (3, 9, 11, 12)


def _status_cases(z):
    """(label, star) whose prior the host refuses with TAMCMC_ERR_BAD_MODEL."""
    out = []
    for name in ("zoo_global", "zoo_local", "zoo_rgb", "zoo_env1"):
        star = z[name].star
        for k in BAD_IDS:
            s = copy.copy(star)
            s.priors_switch = star.priors_switch.copy()
            s.priors_switch[star.index_to_relax[1]] = k
            out.append(("%s, prior id %d" % (name, k), s))
    s = copy.copy(z["zoo_v2"].star)
    s.extra_priors = s.extra_priors.copy()
    s.extra_priors[8] = 2.0
    out.append(("zoo_v2, impose_normHnlm = 2", s))
    for k in range(9):
        s = copy.copy(z["zoo_global"].star)
        s.extra_priors = s.extra_priors.copy()
        s.extra_priors[9] = float(k)
        out.append(("zoo_global, model_index %d" % k, s))
    return out


def test_unsupported_priors_report_bad_model(pkg, oracle, ctx, cases):
    """e. What tamcmc_log_prior refuses (ids 3, 9, 11, 12; impose_normHnlm = 2; model_index 0..8) the gradient batch must refuse with the
    same status, not answer with TAMCMC_OK and -inf (k_fd_unpack: path 1; k_fd_rgb_perturb: path 3; k_env_prior: path 4)."""
    from tamcmc_c_amd import sampler
    pc, z, ex, K = cases
    wrong = []
    current = None
    for label, star in _status_cases(z):
        v, st = sampler.log_prior(star)
        assert st == pkg.ERR_BAD_MODEL and v == -np.inf, (label, v, st)
        if current is not star.x:
            star.y = _give_spectrum(oracle, z[label.split(",")[0]]).y
            ctx.set_spectrum(star.x, star.y)
            current = star.x
        h = 1e-7 * np.maximum(np.abs(star.params[star.index_to_relax]), 1e-3)
        try:
            _, pr0, _ = ctx.fd_gradient_posterior(star, star.params[None, :], h, np.ones(1), 1.0)
            wrong.append((label, "no error", float(pr0[0])))
        except pkg.TamcmcError as e:
            if e.code != pkg.ERR_BAD_MODEL:
                wrong.append((label, e.code))
    print("\nwrong status:", wrong)
    assert not wrong, wrong


# ---- d. proposals that break a hard constraint: rejected on the device exactly where the reference says -inf ----
REJECT_KW = dict(nchains=20, lambda_temp=1.2, seed=31, Nt_learn=(10**9, 10**9 + 1), periods_learn=(2,), dN_mixing=1)


def _moved(star, **values):
    s = copy.copy(star)
    s.params = star.params.copy()
    for k, v in values.items():
        s.params[int(k[1:])] = v
    return s


def _first_displacements(pkg, ctx, star, errors, kw):
    """proposal - start of every chain at iteration 0 (host engine).  Without adaptation it depends on the random numbers, the initial
    errors and the temperatures only -- not on the start vector -- so a start can be PLACED so that a chosen share of the proposals
    crosses a threshold."""
    s = pkg.Sampler(ctx, star, engine="host", init_errors=errors, **kw)
    start = s.state()["vars"].copy()
    s.run(1)
    prop = s.last_test()[0].copy()
    s.close()
    return prop - start


def _between(values, n_below):
    v = np.sort(values)
    return 0.5 * (v[n_below - 1] + v[n_below])


def _scenario(pkg, ctx, pc, zoo, which, kw):
    """(star at the chosen start, initial errors, start of the constraint's reference name): 7 of 20 first proposals break the constraint."""
    from tamcmc_c_amd import sampler
    star = zoo.star
    errors = sampler.default_errors(star)
    d = _first_displacements(pkg, ctx, star, errors, kw)
    idx = list(star.index_to_relax)
    o = pc._offsets(star)
    n_bad = max(3, round(kw["nchains"] * 7 / 20))
    if which == "a_j/a1 through a small a1_0":        # a1_0 + d < max |a_j| / limit for the n_bad smallest displacements
        assert all(star.params[o[6] + 2 * j + 1] == 0 for j in range(6))
        crit = max(abs(star.params[o[6] + 2 * j]) / star.extra_priors[2 + j] for j in range(1, 6))
        return _moved(star, **{"p%d" % o[6]: crit - _between(d[:, idx.index(o[6])], n_bad)}), errors, "|a"
    if which == "a visibility near 0":                # V_l3 + d < 0
        i = o[2] - 1
        return _moved(star, **{"p%d" % i: -_between(d[:, idx.index(i)], n_bad)}), errors, "negative visibility"
    if which == "local a3/a1":                        # |a3| / (c'^2 + s'^2) >= limit for the n_bad smallest c'^2 + s'^2 (a3 is fixed)
        c, s = o[6] + 3, o[6] + 4
        q = (star.params[c] + d[:, idx.index(c)]) ** 2 + (star.params[s] + d[:, idx.index(s)]) ** 2
        return _moved(star, **{"p%d" % (o[6] + 2): star.extra_priors[2] * _between(q, n_bad)}), errors, "|a3/a1| over its limit (sqrt"
    raise ValueError(which)


@pytest.mark.parametrize("name,which", [("zoo_global", "a_j/a1 through a small a1_0"), ("zoo_global", "a visibility near 0"),
                                        ("zoo_local", "local a3/a1")])
def test_constraint_breaking_proposals_are_rejected(pkg, oracle, ctx, cases, name, which):
    """d. Twenty chains at a start where about a third of the first proposals break one hard constraint.  Host engine: run(1), proposals
    from last_test().  Device engine, lockstep kernels (k_iterate: path 1 split; the device-only (degree, order) dealing of the a_j / a1
    checks), from the same state: Pmove == 0 must mark exactly the chains whose host proposal the reference rejects."""
    import prior_reference as ref
    pc, z, ex, K = cases
    _give_spectrum(oracle, z[name])
    ctx.set_spectrum(z[name].star.x, z[name].star.y)
    star, errors, expect = _scenario(pkg, ctx, pc, z[name], which, REJECT_KW)
    assert ref.star_log_prior(star).failed is None
    h = pkg.Sampler(ctx, star, engine="host", init_errors=errors, **REJECT_KW)
    h.run(1)
    prop = h.last_test()[0].copy()
    h.close()
    ctx.set_option(pkg.OPT_STEP_SCHEME, 1)
    d = pkg.Sampler(ctx, star, engine="device", init_errors=errors, **REJECT_KW)
    d.run(1)
    pmove = d.state()["Pmove"].copy()
    d.close()
    ctx.set_option(pkg.OPT_STEP_SCHEME, 0)
    idx = star.index_to_relax
    rejected = kept = left_out = 0
    for m in range(REJECT_KW["nchains"]):
        p = star.params.copy()
        p[idx] = prop[m]
        r = ref.star_log_prior(star, p)
        if r.near_threshold() < 1e-9:
            left_out += 1
            continue
        if r.failed is not None:
            assert r.failed.startswith(expect), (m, r.failed)      # ... and by the chosen constraint, nothing else
            rejected += 1
        else:
            kept += 1
        assert (pmove[m] == 0.0) == (r.failed is not None), (name, which, m, pmove[m], r.failed)
    print("\n%s, %s: %d rejected, %d not, %d left out" % (name, which, rejected, kept, left_out))
    assert left_out <= 1 and rejected >= 3 and kept >= 3


@pytest.mark.parametrize("nchains", [7, 9])
def test_constraint_rejections_inside_fused_launches(pkg, oracle, ctx, cases, nchains):
    """d, fused form (role_prior: path 2 with the hard constraints on half 0).  The pattern of
    test_zero_probability_proposals_inside_fused_launches on the zoo_global star at the edge of its a_j / a1 limit: the events are
    counted from the lockstep kernels one iteration at a time, then one fused call (7 chains: one launch per iteration; 9: two chain
    groups), with the default margin and with the forced fallback, must be the lockstep chain bit for bit and count the same kind-2 tile
    decisions."""
    pc, z, ex, K = cases
    _give_spectrum(oracle, z["zoo_global"])
    ctx.set_spectrum(z["zoo_global"].star.x, z["zoo_global"].star.y)
    kw = dict(REJECT_KW, nchains=nchains, lambda_temp=1.4)
    star, errors, _ = _scenario(pkg, ctx, pc, z["zoo_global"], "a_j/a1 through a small a1_0", kw)
    kw.update(engine="device", init_errors=errors)
    N = 120
    ctx.set_option(pkg.OPT_STEP_SCHEME, 1)
    d = pkg.Sampler(ctx, star, **kw)
    smp, stt, zero, pairA, swaps = [], [], np.zeros((N, nchains), dtype=bool), np.full(N, -1), 0
    for k in range(N):
        a, b = d.run(1, stats=True)
        smp.append(a); stt.append(b)
        st = d.state()
        pm = st["Pmove"].copy()
        if k > 0:
            A = d.draws(k)[3]
            pairA[k] = A
            if st["swaps"] != swaps:
                pm[[A, A + 1]] = pm[[A + 1, A]]      # Pmove travels with the rows
            swaps = st["swaps"]
        zero[k] = pm == 0.0
    ref_run = (np.concatenate(smp), np.concatenate(stt), d.state())
    assert d.info()["iter_fused"] == 0
    d.close()
    alone = sum(int(zero[k, m]) for k in range(N - 1) for m in range(nchains) if not (pairA[k] >= 0 and m in (pairA[k], pairA[k] + 1)))
    in_pair = sum(int(zero[k, pairA[k]]) + int(zero[k, pairA[k] + 1]) for k in range(N - 1) if pairA[k] >= 0)
    print("\n%d chains: %d rejected-by-prior tests alone, %d inside the swap pair, %d tests in all" % (nchains, alone, in_pair, nchains * (N - 1)))
    assert alone >= 10 and in_pair >= 3 and (~zero).sum() > N and (ref_run[0][1:, 0] != ref_run[0][:-1, 0]).any()
    scheme = 0 if nchains < 8 else 3
    for forced in (0, 1):
        ctx.set_option(pkg.OPT_STEP_SCHEME, scheme)
        ctx.set_option(pkg.OPT_QUICK_DECIDE, forced)
        d = pkg.Sampler(ctx, star, **kw)
        a, b = d.run(N, stats=True)
        info, state = d.info(), d.state()
        d.close()
        ctx.set_option(pkg.OPT_STEP_SCHEME, 0)
        ctx.set_option(pkg.OPT_QUICK_DECIDE, 0)
        assert info["iter_fused"] == N and info["fused_stretches"] == 1 and info["iter_lockstep"] == 0, info
        assert info["quick_sure"] == alone, (info, alone)
        assert np.array_equal(a, ref_run[0]) and np.array_equal(b, ref_run[1]), forced
        for key in ("iteration", "swaps", "swap_attempts", "accepted0"):
            assert state[key] == ref_run[2][key], key
        for key in ("vars", "logL", "logPrior", "logPost", "Pmove"):
            assert np.array_equal(state[key], ref_run[2][key]), key

"""The windowed finite-difference route (k_fd_compare, k_fd_moments, k_fd_far, k_loglike<DELTA>) against the exact per-slot reference of
tests/delta_reference.py, on the directed cases of tests/delta_cases.py.

Every slot's dS, read back from the gradient entry, lies inside the reference's budget of named parts (truncation, far field, rounding,
planes: delta_reference.py derives each; none is fitted to the device).  The tables are read back from the same context and inputs
(fd_batch_tables / rgb_batch_tables): the very bits every route goes on from.  The launch's own statistics must show the paths the
restated classification predicts.  Each test prints error / budget and budget / |dS| of its worst slot.

Measured on an MI355X (worst error / budget per case over the five configurations): see DESIGN section 9.
"""
import types

import numpy as np
import pytest

import delta_cases as dc
import delta_reference as dr

pytestmark = pytest.mark.gpu

CONFIGS = [("fast", 64, 8), ("fast", 64, 4), ("fast", 256, 4), ("fast_direct", 256, 4), ("fast_direct", 64, 8)]
IDS = ["%s-%d-%d" % c for c in CONFIGS]


@pytest.fixture(scope="module")
def ctxs(pkg):
    c = {"fast": pkg.HipContext(0, precision=pkg.PRECISION_FAST), "fast_direct": pkg.HipContext(0, precision=pkg.PRECISION_FAST_DIRECT)}
    yield c
    for v in c.values():
        v.close()


def _prepare(pkg, ctxs, cfg, x, y):
    name, wg, K = cfg
    c = ctxs[name]
    c.set_option(pkg.OPT_WORKGROUP, wg)
    c.set_option(pkg.OPT_BINS_PER_THREAD, K)
    c.set_option(pkg.OPT_FD_WINDOWED, 1)
    c.set_spectrum(x, y)
    return c


_DEV = {}


def _device_case(pkg, synth, ctxs, name):
    """(case, tables, references) with the tables read back from the device, once per process."""
    if name not in _DEV:
        if name == "red_giant":
            c = dc.red_giant(synth)
            ctx = _prepare(pkg, ctxs, CONFIGS[0], c.star.x, np.ones(c.star.x.size))
            rows, noise, nh, status = ctx.rgb_batch_tables(c.star.model_id, c.P, c.star.plength, c.idx, c.h)
            assert (status == 0).all()
            tabs = [dr.Table(r, nz, int(h), nz.size) for r, nz, h in zip(rows, noise, nh)]
            m = dr.base_row(tabs[0], c.star.x).astype(np.float64)
            c = c._replace(y=m * np.random.default_rng(1).exponential(1.0, m.size))
        else:
            c = dc.case(pkg, synth, name)
            ctx = _prepare(pkg, ctxs, CONFIGS[0], c.star.x, c.y)
            rows, noise, nh, nn, status = ctx.fd_batch_tables(c.star.model_id, c.P, c.star.plength, c.idx, c.h)
            assert (status == 0).all()
            tabs = [dr.Table(r, nz[:n].copy(), int(h), int(n)) for r, nz, h, n in zip(rows, noise, nh, nn)]
            # the other arithmetic mode builds the same tables
            other = _prepare(pkg, ctxs, CONFIGS[3], c.star.x, c.y).fd_batch_tables(c.star.model_id, c.P, c.star.plength, c.idx, c.h)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(rows, other[0])) and np.array_equal(noise, other[1])
        _DEV[name] = (c, tabs, dc.references((name, "device"), c, tabs))
    return _DEV[name]


def _gradient(pkg, ctx, c, P, T, posterior=False):
    try:
        return _gradient_call(ctx, c, P, T, posterior)
    except pkg.TamcmcError as e:   # a device error ends the session: nothing more is started on the GPU after it
        pytest.exit("device error: %s" % e, 3)


def _gradient_call(ctx, c, P, T, posterior):
    if posterior:
        view = types.SimpleNamespace(model_id=c.star.model_id, prior_class=c.star.prior_class, plength=c.star.plength, index_to_relax=c.idx,
                                     priors=c.star.priors, priors_switch=c.star.priors_switch, extra_priors=c.star.extra_priors)
        _, _, g = ctx.fd_gradient_posterior(view, P, c.h, T, 1.0)
        return g - ctx.last_grad_prior, np.abs(g) + np.abs(ctx.last_grad_prior)
    _, g = ctx.fd_gradient(c.star.model_id, P, c.star.plength, c.idx, c.h, T, 1.0)
    return g, np.zeros_like(g)


def _check(pkg, synth, ctxs, name, cfg, posterior=False):
    c, tabs, refs = _device_case(pkg, synth, ctxs, name)
    conf = dr.config(*cfg)
    ctx = _prepare(pkg, ctxs, cfg, c.star.x, c.y)
    ctx.set_option(pkg.OPT_TIMING, 1)
    ctx.reset_kernel_stats()
    g, gsub = _gradient(pkg, ctx, c, c.P, c.T, posterior)
    bins, evals = ctx.fd_stats()
    n_full = ctx.fd_full_tables()
    ctx.set_option(pkg.OPT_TIMING, 0)
    assert np.all(np.isfinite(g))
    E = c.idx.size + 1
    worst = (0.0, None)
    widest = (0.0, None)
    dS_dev = np.zeros(g.shape)
    budgets = np.zeros(g.shape)
    walked_min = walked_max = full = 0
    for ch in range(c.P.shape[0]):
        for k in range(E - 1):
            r = refs[ch][k]
            b = dr.slot_budget(r, tabs[ch * E], tabs[ch * E + 1 + k], c.star.x, conf)
            d = dr.device_dS(g[ch, k], c.P[ch, c.idx[k]], c.h[k], c.T[ch])
            happ = (c.P[ch, c.idx[k]] + c.h[k]) - c.P[ch, c.idx[k]]
            # (posterior entry: the likelihood share is a difference of two doubles of the size of the prior's share)
            tol = b.total + 2 * dr.EPS * gsub[ch, k] * abs(happ) * c.T[ch]
            err = abs(d - float(r.dS))
            dS_dev[ch, k], budgets[ch, k] = d, tol
            if tol > 0 and err / tol >= worst[0]:
                worst = (err / tol, (ch, k, c.why[k], err, b))
            if float(r.dS) != 0.0 and tol / abs(float(r.dS)) >= widest[0]:
                widest = (tol / abs(float(r.dS)), (ch, k, c.why[k]), b)
            walked_min += b.walked_min
            walked_max += b.walked_max
            full += dr.slot_of(r, conf).full
    print("\n%s %s%s: worst error / budget %.3g at %s; widest budget / |dS| %.3g at %s" %
          (name, conf.name, " posterior" if posterior else "", worst[0], worst[1][:3] if worst[1] else None, widest[0], widest[1]))
    if worst[1]:
        b = worst[1][4]
        print("    its parts: truncation %.2e far %.2e rounding %.2e planes %.2e; error %.2e" % (b.truncation, b.far, b.rounding, b.planes, worst[1][3]))
    if widest[1]:
        b = widest[2]
        print("    the widest one's parts: truncation %.2e far %.2e rounding %.2e planes %.2e" % (b.truncation, b.far, b.rounding, b.planes))
    for ch in range(c.P.shape[0]):
        for k in range(E - 1):
            assert abs(dS_dev[ch, k] - float(refs[ch][k].dS)) <= budgets[ch, k], (name, conf.name, ch, k, c.why[k], dS_dev[ch, k], float(refs[ch][k].dS), budgets[ch, k])
    # the paths, from the launch's own statistics
    assert evals == c.P.shape[0] * E
    assert n_full == full, (n_full, full)
    assert walked_min <= bins <= walked_max, (bins, walked_min, walked_max)
    if conf.wg != 64 or not conf.farfield:
        assert walked_min == walked_max == sum(dr.slot_of(r, conf).hi - dr.slot_of(r, conf).lo for row in refs for r in row)
    return c, ctx, g, dS_dev, budgets


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", list(dc.MAKERS))
def test_every_slot_inside_its_budget(pkg, synth, ctxs, name, cfg):
    c, ctx, g, _, _ = _check(pkg, synth, ctxs, name, cfg)
    # a chain's differences are the same bits alone and as one of three, and on a second call
    g1, _ = _gradient(pkg, ctx, c, c.P[1:2], c.T[1:2])
    assert np.array_equal(g1[0], g[1])
    g2, _ = _gradient(pkg, ctx, c, c.P, c.T)
    assert np.array_equal(g2, g)


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[2], CONFIGS[3]], ids=[IDS[0], IDS[2], IDS[3]])
def test_red_giant_slots_inside_their_budget(pkg, synth, ctxs, cfg):
    """id 25: tables from the device pre-step.  The classification is checked here (no host builder makes these tables): the height is a
    heights-only change, the period spacing moves every mixed mode; which path the 0.5 % step takes, and whether it changes the number
    of rows, is printed (DESIGN section 9 records it)."""
    c, tabs, refs = _device_case(pkg, synth, ctxs, "red_giant")
    E = c.idx.size + 1
    for ch in range(c.P.shape[0]):
        n0 = len(tabs[ch * E].rows)
        for k in range(E - 1):
            s = refs[ch][k].slot
            print("red_giant chain %d %-14s rows %d -> %d %s full %d light %d delta rows %d" %
                  (ch, c.why[k], n0, len(tabs[ch * E + 1 + k].rows), s.counts, s.full, s.light, len(s.drows)))
            if c.why[k] == "heights":
                assert s.counts["heights_only"] >= 1 and s.counts["pair"] == 0
            if c.why[k] == "period_spacing":
                assert s.counts["pair"] + s.counts["one_sided"] >= 4
    _check(pkg, synth, ctxs, "red_giant", cfg)


def test_posterior_entry_gives_the_same_differences(pkg, synth, ctxs):
    """fd_gradient_posterior with grad - last_grad_prior on the moments case: the same budget (plus the subtraction's own rounding)."""
    c, ctx, g, dS, _ = _check(pkg, synth, ctxs, "moments", CONFIGS[0], posterior=True)


def test_moment_path_is_taken_and_matters(pkg, synth, ctxs):
    """FAST (64, 8) and FAST_DIRECT on the moments case agree within the sum of their budgets and are not bit-identical."""
    _, _, ga, da, ba = _check(pkg, synth, ctxs, "moments", CONFIGS[0])
    _, _, gb, db, bb = _check(pkg, synth, ctxs, "moments", CONFIGS[4])
    assert np.all(np.abs(da - db) <= ba + bb)
    c = dc.case(pkg, synth, "moments")
    light = [k for k, w in enumerate(c.why) if w == "light"]
    assert not np.array_equal(ga[:, light], gb[:, light])


def test_brute_route_noise_covers_the_exact_reference(pkg, synth, ctxs):
    """OPT_FD_WINDOWED = 0 on the series case: the exact reference lies within the brute route's documented noise, 5e-15 Nx / h."""
    c, tabs, refs = _device_case(pkg, synth, ctxs, "series")
    ctx = _prepare(pkg, ctxs, CONFIGS[0], c.star.x, c.y)
    ctx.set_option(pkg.OPT_FD_WINDOWED, 0)
    _, g = ctx.fd_gradient(c.star.model_id, c.P, c.star.plength, c.idx, c.h, c.T, 1.0)
    ctx.set_option(pkg.OPT_FD_WINDOWED, 1)
    worst = 0.0
    for ch in range(c.P.shape[0]):
        for k in range(c.idx.size):
            happ = (c.P[ch, c.idx[k]] + c.h[k]) - c.P[ch, c.idx[k]]
            exact = -float(refs[ch][k].dS) / c.T[ch] / happ
            tol = 5e-15 * c.star.x.size / c.h[k]
            worst = max(worst, abs(g[ch, k] - exact) / tol)
            assert abs(g[ch, k] - exact) <= tol, (ch, k, g[ch, k], exact, tol)
    print("\nbrute route on series: worst |g - exact| / (5e-15 Nx / h) = %.3g" % worst)

"""The device-resident sampler in every arithmetic mode and tile geometry (-m gpu).

tamcmc_hip_set_option accepts three modes (STRICT, FAST_DIRECT, FAST) x six geometries (workgroup 256 x 1, 2, 4 bins per lane, workgroup
64 x 4, 8, 16), the lockstep engine (k_iterate -> k_loglike) reads whatever the context holds, and the fused step dispatches on
(mode, K) into nine kernels (dev_step_impl.h::launch_step; K = 16 is k_step_wide, with launch attributes of its own).  The sampler tests
beside this module open FAST contexts at the library's default geometry.  Here:

  (a) lockstep      all 18 (mode, geometry) pairs x two stars: 30 iterations one at a time; a chain that accepts holds the logL of the
                    long-double twin (tile_reference.py) of the table the engine itself built for the proposal, within the header's
                    tolerance (1e-12 |L| STRICT, 1e-11 |L| FAST_DIRECT and FAST: check_logl's numbers), the slot's log-prior bit for
                    bit and logPost = logL + logPrior; every other chain keeps its state bit for bit
  (b) fused         all nine (mode, K) at workgroup 64 x two stars x two parametrisations: the body of
                    test_gpu_sampler.test_fused_steps_are_bitwise_the_lockstep_chain (lockstep, fused, fused with the forced fallback:
                    array_equal), its counters, and quick_mismatch == 0
  (c) host engine   test_gpu_sampler.test_device_engine_follows_host_engine's criterion on a default-constructed context (STRICT,
                    256 x 4), FAST_DIRECT 64 x 8, FAST 64 x 16, FAST 256 x 1
  (d) mode switch   FAST_DIRECT -> FAST -> STRICT between calls of one fused-scheme and one scheme-1 sampler: the same records (the
                    background-series buffers of dev_sampler_run.h::prepare are reserved only under FAST)

The stars.  Both have 3075 bins = 12 x 256 + 3 = 6 x 512 + 3 = 3 x 1024 + 3: every geometry ends in a tile of three bins.
  A  synth.make_c2_star(nx=3075): model id 11, 21 free of 28 parameters, six rows, window edges inside the grid, no Harvey term
  B  synth.make_c3_star(nx=3075, nmax=2, step=0.04, fmin=1990.0): model id 23, 21 free of 39 parameters, eight rows, two Harvey terms
What makes them exercise the FAST paths is asserted on the host (star_facts, also run without a GPU by test_the_stars_reach_the_far_
field_and_the_series): every tile of B at every tile size has a far row and an open series gate; every tile of A at 256 and 512 bins
has a far row, and at 1024 bins tiles 0, 2 and 3 of the four (tile 1, bins 1024 .. 2047, is the near field of all four rows whose windows
cover it: beta^2 = (2 h / gamma)^2 ~ 450 .. 1090 against (A^2 + 1) / 36 ~ 250 .. 405).  A has no Harvey term: no series.

(a), the seed.  SEED = 1 was chosen on FAST at 64 x 8 as the first of 1, 2, 3, .. with which every one of the three chains of BOTH
stars accepts at least once and refuses at least once in the 30 iterations; the same seed serves every combination (their trajectories
agree to rounding).  Accepted / refused per chain there: star A 13 / 17, 18 / 12, 20 / 10; star B 9 / 21, 12 / 18, 12 / 18
(chains 0, 1, 2; seeds 1 .. 16 all qualify).

Mutation check (built and run once, not committed): TAMCMC_PRECISION_FAST_DIRECT mapped to tile::M_FAST in launch_step.  All twelve
FAST_DIRECT cases of (b) fail (the fused records differ from the lockstep chain's: the array_equal of the samples or of the statistics),
the 24 STRICT and FAST cases pass.
"""
import math

import numpy as np
import pytest

import tile_reference as tr
from test_gpu_sampler import (_check_scheme_counters, device_engine_follows_host_engine,
                              fused_steps_are_bitwise_the_lockstep_chain)

gpu = pytest.mark.gpu

NX = 3075
TILE_SIZES = (256, 512, 1024)
GEOMS = ((256, 1), (256, 2), (256, 4), (64, 4), (64, 8), (64, 16))   # (workgroup, bins per lane)
MODES = (("strict", 1e-12), ("fast_direct", 1e-11), ("fast", 1e-11))  # logL against the twin, relative: the header's, as check_logl
FAR_TILES_A_1024 = (0, 2, 3)

SEED = 1
N_ITER = 30
NCHAINS, LAMBDA = 3, 1.6


def _precision(pkg, mode):
    return {"strict": pkg.PRECISION_STRICT, "fast_direct": pkg.PRECISION_FAST_DIRECT, "fast": pkg.PRECISION_FAST}[mode]


_STARS = {}


def stars(pkg, oracle, synth):
    """{"A": star, "B": star}, each with its spectrum drawn around the oracle's model (as test_gpu_sampler._star_with_data); built once."""
    if not _STARS:
        for name, star in (("A", synth.make_c2_star(nx=NX)), ("B", synth.make_c3_star(nx=NX, nmax=2, step=0.04, fmin=1990.0))):
            st, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
            assert st == 0
            star.set_spectrum_from_model(m0, 5)
            _STARS[name] = star
    return _STARS


def star_facts(pkg, star):
    """{tile_bins: (tiles that have a far row, tiles whose series gate is open, number of tiles)} of the star's start point, from the
    host table builder and the restated gates of tile_reference.py."""
    st, mults, noise, nh = pkg.build_mode_table(star.model_id, star.params, star.plength, star.x)
    assert st == 0
    x0, step = float(star.x[0]), float(star.x[1] - star.x[0])
    out = {}
    for tb in TILE_SIZES:
        nt = (NX + tb - 1) // tb
        far = sorted({t for _, t in tr.far_map(mults, NX, tb, x0, step)})
        active = nh > 0 and any(noise[3 * k + 1] != 0.0 for k in range(nh))
        series = [t for t in range(nt) if active and tr.series_gate(noise, nh, *tr.tile_geometry(t, tb, x0, step))]
        out[tb] = (far, series, nt)
    return out, len(mults), nh


def check_star_facts(pkg, oracle, synth):
    ss = stars(pkg, oracle, synth)
    a, b = ss["A"], ss["B"]
    assert (a.model_id, a.nvars, a.params.size, a.x.size) == (11, 21, 28, NX)
    assert (b.model_id, b.nvars, b.params.size, b.x.size) == (23, 21, 39, NX)
    fa, rows_a, nh_a = star_facts(pkg, a)
    fb, rows_b, nh_b = star_facts(pkg, b)
    assert (rows_a, nh_a, rows_b, nh_b) == (6, 0, 8, 2)
    for tb in TILE_SIZES:
        assert NX % tb == 3
        nt = fb[tb][2]
        assert fb[tb][0] == list(range(nt)) and fb[tb][1] == list(range(nt)), ("B", tb, fb[tb])
        assert fa[tb][0] == (list(FAR_TILES_A_1024) if tb == 1024 else list(range(nt))) and fa[tb][1] == [], ("A", tb, fa[tb])


def test_the_stars_reach_the_far_field_and_the_series(pkg, oracle, synth):
    """No GPU needed: a later change of synth.py must not empty the tests below (they assert the same before they run)."""
    check_star_facts(pkg, oracle, synth)


@pytest.fixture(scope="module")
def facts(pkg, oracle, synth):
    check_star_facts(pkg, oracle, synth)
    return stars(pkg, oracle, synth)


@pytest.fixture(scope="module")
def ctxs(pkg):
    c = {mode: pkg.HipContext(0, precision=_precision(pkg, mode)) for mode, _ in MODES}
    yield c
    for v in c.values():
        v.close()


def _configured(pkg, ctxs, mode, wg, K, star):
    c = ctxs[mode]
    c.set_option(pkg.OPT_WORKGROUP, wg)
    c.set_option(pkg.OPT_BINS_PER_THREAD, K)
    c.set_option(pkg.OPT_STEP_SCHEME, 0)
    c.set_option(pkg.OPT_QUICK_DECIDE, 0)
    c.set_spectrum(star.x, star.y)
    return c


# ------------------------------------------------------------------ (a) lockstep chains against the twin ------------------------------------------------------------------
def lockstep_chain_against_the_twin(pkg, ctx, star, tol, seed=SEED, n=N_ITER):
    """N_ITER iterations of three chains under TAMCMC_OPT_STEP_SCHEME = 1, no adaptation, no swap, one run(1, stats=True) at a time, with
    the assertions of (a) after each.  Returns (worst |logL - L| / (tol |L|), accepted per chain, refused per chain)."""
    ctx.set_option(pkg.OPT_STEP_SCHEME, 1)
    s = pkg.Sampler(ctx, star, engine="device", nchains=NCHAINS, lambda_temp=LAMBDA, seed=seed, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,),
                    dN_mixing=10**6)
    try:
        T = [math.pow(LAMBDA, m) for m in range(NCHAINS)]
        idx = star.index_to_relax
        prev = s.state()
        worst = 0.0
        accepted, refused = np.zeros(NCHAINS, dtype=int), np.zeros(NCHAINS, dtype=int)
        for it in range(n):
            _, stt = s.run(1, stats=True)
            t, st = s.tables(), s.state()
            assert t["scheme"] == 1 and len(t["tables"]) == NCHAINS and t["written"].all()
            assert st["iteration"] == it + 1 and st["swap_attempts"] == 0
            for m in range(NCHAINS):
                rows, noise, nh, nn = t["tables"][m], t["noise"][m], int(t["nharvey"][m]), int(t["nnoise"][m])
                placeholder = len(rows) == 0 and nn == 1 and noise[0] == 1.0 and nh == 0
                if not np.isfinite(t["logprior"][m]) or t["status"][m] != 0:
                    assert placeholder, (it, m, t["logprior"][m], t["status"][m])
                moved = not np.array_equal(st["vars"][m], prev["vars"][m])
                if moved and np.array_equal(st["vars"][m], t["params"][m][idx]):
                    assert not placeholder, (it, m, "a chain accepted a proposal whose slot holds the placeholder")
                    M = tr.model_row_ld(rows, noise, nh, nn, star.x)
                    L = tr.loglike_ld(M, star.y, T[m], 1)
                    for what, got in (("state", st["logL"][m]), ("record", stt[0, m, 0])):
                        r = abs(float((tr.LD(got) - L) / L)) / tol
                        worst = max(worst, r)
                        assert r <= 1.0, (it, m, what, r, got, float(L))
                    assert st["logPrior"][m] == t["logprior"][m], (it, m)
                    assert st["logPost"][m] == st["logL"][m] + st["logPrior"][m], (it, m)
                    accepted[m] += 1
                else:
                    for k in ("vars", "logL", "logPrior", "logPost"):
                        assert np.array_equal(st[k][m], prev[k][m]), (it, m, k, "a chain that did not accept its proposal changed")
                    refused[m] += 1
            prev = st
        info = s.info()
        assert info["iter_lockstep"] == n and info["iter_fused"] == 0, info
        return worst, accepted, refused
    finally:
        s.close()
        ctx.set_option(pkg.OPT_STEP_SCHEME, 0)


@gpu
@pytest.mark.parametrize("wg,K", GEOMS)
@pytest.mark.parametrize("mode,tol", MODES)
def test_lockstep_chain_holds_the_twins_likelihood(pkg, facts, ctxs, mode, tol, wg, K):
    """(a).  The worst ratio of the combination is printed (DESIGN section 9 records the 18 figures)."""
    worst = 0.0
    for name in ("A", "B"):
        star = facts[name]
        c = _configured(pkg, ctxs, mode, wg, K, star)
        w, acc, ref = lockstep_chain_against_the_twin(pkg, c, star, tol)
        print("\n%-11s %3d x %-2d star %s: accepted %s refused %s, worst |logL - L| / (%.0e |L|) = %.4f" % (mode, wg, K, name, acc, ref, tol, w))
        assert np.all(acc >= 1) and np.all(ref >= 1), (name, acc, ref)
        worst = max(worst, w)
    print("%-11s %3d x %-2d worst ratio %.4f" % (mode, wg, K, worst))


# ------------------------------------------------------------------ (b) fused launches are the lockstep chain ------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nchains,learn", [(7, None), (9, (40, 90))])
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("K", [4, 8, 16])
@pytest.mark.parametrize("mode", [m for m, _ in MODES])
def test_fused_steps_are_bitwise_the_lockstep_chain_in_every_mode(pkg, facts, ctxs, mode, K, name, nchains, learn):
    """(b).  7 chains: one launch per iteration (scheme 0); 9 chains: two chain groups (scheme 3) and an adaptation window.  Under STRICT
    and FAST_DIRECT the fused step has no background-series buffer; star B's two Harvey terms go through the tiles' per-bin code."""
    star = facts[name]
    c = _configured(pkg, ctxs, mode, 64, K, star)
    infos = fused_steps_are_bitwise_the_lockstep_chain(pkg, c, star, nchains, 1, learn, n1=150)
    for k, (scheme, forced) in enumerate(((1, 0), (0 if nchains < 8 else 3, 0), (0 if nchains < 8 else 3, 1))):
        _check_scheme_counters(infos[k], nchains, scheme, forced)
        assert infos[k]["quick_mismatch"] == 0, (k, infos[k])
    assert infos[1]["chain_groups"] == (1 if nchains < 8 else 2), infos[1]


# ------------------------------------------------------------------ (c) the device engine follows the host engine ------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,wg,K", [(None, 256, 4), ("fast_direct", 64, 8), ("fast", 64, 16), ("fast", 256, 1)])
def test_device_engine_follows_host_engine_in_other_modes(pkg, facts, mode, wg, K):
    """(c), star A.  mode None: a default-constructed context, no option set -- STRICT at 256 x 4 by the library's own defaults."""
    star = facts["A"]
    c = pkg.HipContext(0) if mode is None else pkg.HipContext(0, precision=_precision(pkg, mode), workgroup=wg, bins_per_thread=K)
    try:
        c.set_spectrum(star.x, star.y)
        first_div, info = device_engine_follows_host_engine(pkg, c, star)
        print("\n%s %d x %d: first divergence %d, %r" % (mode or "default", wg, K, first_div, info))
        assert info["iter_fused"] + info["iter_lockstep"] == 120
        assert (info["iter_fused"] > 0) == (wg == 64), info      # (the fused step exists for the one-wave geometries only)
    finally:
        c.close()


# ------------------------------------------------------------------ (d) a mode switch between two calls ------------------------------------------------------------------
@gpu
def test_mode_switch_between_calls(pkg, facts):
    """(d), star B at 64 x 8, 7 chains, a swap step in every iteration.  The fused sampler's candidates of the next iteration are carried
    from call to call; a switch of the arithmetic mode reserves (FAST) or drops (the others) the series buffers they were built with."""
    star = facts["B"]
    cs = [pkg.HipContext(0, precision=pkg.PRECISION_FAST_DIRECT, workgroup=64, bins_per_thread=8) for _ in range(2)]
    try:
        kw = dict(engine="device", nchains=7, lambda_temp=1.4, seed=23, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,), dN_mixing=1)
        smp = []
        for c, scheme in zip(cs, (0, 1)):
            c.set_spectrum(star.x, star.y)
            c.set_option(pkg.OPT_STEP_SCHEME, scheme)
            smp.append(pkg.Sampler(c, star, **kw))
        fused_before = 0
        for seg, mode in enumerate(("fast_direct", "fast", "strict")):
            for c in cs:
                c.set_option(pkg.OPT_PRECISION, _precision(pkg, mode))
            (sa, ta), (sb, tb) = (s.run(20, stats=True) for s in smp)
            assert np.all(np.isfinite(ta)) and np.all(np.isfinite(tb)) and np.all(np.isfinite(sa)), mode
            assert np.array_equal(sa, sb) and np.array_equal(ta, tb), (mode, int(np.argmax(np.any(sa != sb, axis=(1, 2)))))
            ia, ib = smp[0].info(), smp[1].info()
            assert ia["iter_fused"] > fused_before and ia["quick_mismatch"] == 0, (mode, ia)
            assert ib["iter_fused"] == 0 and ib["iter_lockstep"] == 20 * (seg + 1), (mode, ib)
            fused_before = ia["iter_fused"]
        a, b = smp[0].state(), smp[1].state()
        for k in ("iteration", "swaps", "swap_attempts", "accepted0"):
            assert a[k] == b[k], k
        for k in ("vars", "logL", "logPrior", "logPost", "Pmove"):
            assert np.array_equal(a[k], b[k]), k
        assert a["iteration"] == 60 and a["swaps"] > 0 and (sa[:, 0] != sa[0, 0]).any()
    finally:
        for c in cs:
            c.close()

"""GPU tests of the head of the fused step's likelihood tiles (-m gpu): the decision shortcut reads ONE value per tile of the previous
launch (FusedArgs::psum, stored beside the two partial sums), sums one chain only for a chain outside the swap pair, and the tile requests
its x values and both possible slots' table words before it.  None of that may move a bit of a chain: the lockstep kernels, the fused
steps (one launch per iteration and two chain groups) and the fused steps with every tile test forced into the exact decide() must
produce the same samples and statistics, at every count of tiles at which the shortcut's loads take another shape."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 512  # workgroup = 64 lanes x 8 bins: the geometry of the headline configuration, pinned here (short spectra default to 256)


def _star(oracle, synth, nx):
    star = synth.make_c2_star(nx=nx)
    _, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    star.set_spectrum_from_model(m0, nx)
    return star


def _ctx(pkg, star):
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST, workgroup=64)
    c.set_spectrum(star.x, star.y)
    return c


# nx = 4000: 8 tiles, the last one partial (416 bins); 500: ONE partial tile; 33500: 66 tiles, the last partial -- more than 64, so
# some lanes of the shortcut load a second value.  7 chains: one launch per iteration; 8: two chain groups under scheme 3.  dN_mixing = 1
# and 3: iterations with a swap pair (two chains inside it, the others outside) and without one, in the same run.
@pytest.mark.parametrize("nx,nchains,dN_mixing", [(4000, 7, 1), (4000, 8, 3), (500, 8, 1), (500, 7, 3), (33500, 7, 3), (33500, 8, 1)])
def test_tile_head_leaves_the_chains_bitwise_unchanged(pkg, oracle, synth, nx, nchains, dN_mixing):
    """Two calls of one sampler: 64 iterations with a learning window in the middle (fused stretch -> lockstep stretch -> fused stretch:
    the second fused stretch starts from chains the lockstep kernels settled), then 27 more (the candidates armed by the first call's
    last launch, and the per-tile sums that go with them, are carried over).  Lockstep | one fused launch per iteration | two chain
    groups | each of the two with TAMCMC_OPT_QUICK_DECIDE = 1: five runs, one chain.  Under the forced option every tile test is
    either a fallback or a kind-2 decision: quick_fallbacks + quick_sure == nchains x (iter_fused - fused_stretches)."""
    assert (nx + TILE - 1) // TILE in (1, 8, 66) and nx % TILE != 0
    star = _star(oracle, synth, nx)
    ctx = _ctx(pkg, star)
    kw = dict(nchains=nchains, lambda_temp=1.4, seed=41, Nt_learn=(24, 40), periods_learn=(2,), dN_mixing=dN_mixing, engine="device")
    runs = ((1, 0), (2, 0), (3, 0), (2, 1), (3, 1))
    out, infos = [], []
    for scheme, forced in runs:
        ctx.set_option(pkg.OPT_STEP_SCHEME, scheme)
        ctx.set_option(pkg.OPT_QUICK_DECIDE, forced)
        d = pkg.Sampler(ctx, star, **kw)
        s1, t1 = d.run(64, stats=True)
        s2, t2 = d.run(27, stats=True)
        out.append((np.concatenate([s1, s2]), np.concatenate([t1, t2]), d.state()))
        infos.append(d.info())
        d.close()
    ctx.set_option(pkg.OPT_STEP_SCHEME, 0)
    ctx.set_option(pkg.OPT_QUICK_DECIDE, 0)
    ctx.close()
    ref = out[0]
    assert infos[0]["iter_fused"] == 0 and infos[0]["quick_fallbacks"] == 0
    assert np.isfinite(ref[1]).all() and (ref[0][1:, 0] != ref[0][:-1, 0]).any()    # the cold chain moves
    for k, (scheme, forced) in enumerate(runs):
        if k == 0:
            continue
        info = infos[k]
        print("\nscheme %d forced %d: %s" % (scheme, forced, {q: info[q] for q in ("iter_fused", "fused_stretches", "quick_fallbacks", "quick_sure")}))
        assert info["fused_available"] == 1 and info["iter_fused"] + info["iter_lockstep"] == 91, info
        assert info["fused_stretches"] >= 3 and info["iter_lockstep"] > 0, info     # two stretches around the learning window + the second call
        tests = nchains * (info["iter_fused"] - info["fused_stretches"])
        assert tests > 0
        if forced:
            assert info["quick_fallbacks"] + info["quick_sure"] == tests, (info, tests)
            assert info["quick_fallbacks"] > 0
        assert info["quick_sure"] == infos[1]["quick_sure"] and info["iter_fused"] == infos[1]["iter_fused"]
        assert np.array_equal(out[k][0], ref[0]), (scheme, forced)
        assert np.array_equal(out[k][1], ref[1]), (scheme, forced)
        for key in ("iteration", "swaps", "swap_attempts", "accepted0"):
            assert out[k][2][key] == ref[2][key], (scheme, forced, key)
        for key in ("vars", "logL", "logPrior", "logPost", "Pmove", "sigma"):
            assert np.array_equal(out[k][2][key], ref[2][key]), (scheme, forced, key)


def test_kind2_records_still_decide_without_sums(pkg, oracle, synth):
    """A star with two prior edges 0.02 muHz from the start point: a fifth of the proposals lie outside a prior's support and leave a
    kind-2 record ("cannot be accepted").  The tiles of an empty slot are skipped, so neither the partial sums nor the per-tile value of
    such a proposal exist: a chain outside the swap pair must be decided from the record alone.  The events are counted from the
    lockstep kernels, one iteration per call (Pmove == 0, the pair's entries put back where a swap took them from); the fused run with
    the DEFAULT margin must report exactly that many (quick_sure) and be the same chain."""
    star = _star(oracle, synth, 4000)
    fidx = [i for i, nm in enumerate(star.names) if nm == "Frequency_l"]
    for i in (fidx[2], fidx[5]):
        star.priors[0, i] = star.params[i] - 0.02
    ctx = _ctx(pkg, star)
    N, nchains = 120, 7
    kw = dict(nchains=nchains, lambda_temp=1.4, seed=31, Nt_learn=(10**9, 10**9 + 1), periods_learn=(2,), dN_mixing=1, engine="device")
    ctx.set_option(pkg.OPT_STEP_SCHEME, 1)
    d = pkg.Sampler(ctx, star, **kw)
    smp, stt, alone, swaps = [], [], 0, 0
    for k in range(N):
        a, b = d.run(1, stats=True)
        smp.append(a); stt.append(b)
        st = d.state()
        pm = st["Pmove"].copy()
        A = -1
        if k > 0:                                    # dN_mixing = 1: a swap step at every iteration but the first
            A = d.draws(k)[3]
            if st["swaps"] != swaps:
                pm[[A, A + 1]] = pm[[A + 1, A]]
            swaps = st["swaps"]
        if k < N - 1:                                # (the last iteration is decided by the closing launch, which has no tiles)
            alone += sum(1 for m in range(nchains) if pm[m] == 0.0 and not (A >= 0 and m in (A, A + 1)))
    ref = (np.concatenate(smp), np.concatenate(stt))
    assert d.info()["iter_fused"] == 0
    d.close()
    assert alone >= 8, alone
    ctx.set_option(pkg.OPT_STEP_SCHEME, 0)
    d = pkg.Sampler(ctx, star, **kw)
    a, b = d.run(N, stats=True)
    info = d.info()
    d.close()
    ctx.close()
    assert info["iter_fused"] == N and info["fused_stretches"] == 1, info
    assert info["quick_sure"] == alone, (info, alone)
    assert info["quick_fallbacks"] * 1000 <= nchains * (N - 1) + 1000, info
    assert np.array_equal(a, ref[0]) and np.array_equal(b, ref[1])

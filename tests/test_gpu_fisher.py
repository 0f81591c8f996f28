"""Expected (Fisher) information on the GPU (tamcmc_hip_fisher, tamcmc_hip_weighted_gram, tamcmc_sampler_seed_proposal_fisher;
csrc/fisher.hip) against the numpy yardstick of tests/fisher_numpy.py (validated on the CPU by tests/test_fisher_numpy.py).  Every test
here fails without the feature: the entries and the option do not exist.

  exact Gram    the Gram and fold kernels on small integers, where every sum is exact in double: block layout, lane map of the fp64 matrix
                instruction, padding to 16, slab boundaries;
  yardstick     |F_dev - F_ref| <= 2 B elementwise, B the FAST tolerance of a model row carried through the difference and the product
                (fisher_numpy.bound); the factor 2 is for the device table builder's last-ulp differences in the frequencies;
  properties    symmetry, positive semi-definiteness, independence of batch, position and passes, the p / T scaling;
  refusals, sampler seeding on both engines.
"""
import numpy as np
import pytest

import adjoint_numpy as an
import fisher_numpy as fn

pytestmark = pytest.mark.gpu

CONFIGS = [("fast", 64, 8), ("fast", 256, 4), ("fast_direct", 64, 8), ("fast_direct", 256, 4)]   # arithmetic, workgroup, bins per thread
# the geometries that have no DELTA kernel (the Rows route is allowed in any geometry, fd_route.h): on the smallest case, c2
NO_DELTA_CONFIGS = [(mode, wg, K) for mode in ("fast", "fast_direct") for wg, K in ((256, 1), (256, 2), (64, 16))]


@pytest.fixture(scope="module")
def ctxs(pkg):
    c = {"fast": pkg.HipContext(0, precision=pkg.PRECISION_FAST), "fast_direct": pkg.HipContext(0, precision=pkg.PRECISION_FAST_DIRECT)}
    yield c
    for v in c.values():
        v.close()


def _configured(pkg, ctxs, cfg, star, y):
    name, wg, K = cfg
    c = ctxs[name]
    c.set_option(pkg.OPT_WORKGROUP, wg)
    c.set_option(pkg.OPT_BINS_PER_THREAD, K)
    c.set_spectrum(star.x, y)
    return c


@pytest.mark.parametrize("N", [1, 16, 17, 33, 93, 130])
def test_weighted_gram_is_exact_on_small_integers(pkg, ctxs, N):
    """A in [-8, 8], w in {1, 2, 4}: every product and every partial sum is an integer below 2^53, so any order gives the same double.
    K = 1, 5 (less than one matrix instruction / than a staged chunk), 4000, one slab + 3."""
    c = ctxs["fast"]
    rng = np.random.default_rng(100 + N)
    for K in (1, 5, 4000, pkg.FISHER_SLAB + 3):
        A = rng.integers(-8, 9, size=(N, K)).astype(np.float64)
        w = rng.choice([1.0, 2.0, 4.0], size=K)
        Ai = A.astype(np.int64)
        for wt, wi in ((w, w.astype(np.int64)), (None, np.ones(K, dtype=np.int64))):
            want = ((Ai * wi[None, :]) @ Ai.T).astype(np.float64)
            G = c.weighted_gram(A, wt)
            assert np.array_equal(G, want), (N, K, wt is None, np.argwhere(G != want)[:4])
            assert np.array_equal(c.weighted_gram(A, wt), G)


def test_weighted_gram_does_not_see_the_tile_geometry(pkg, ctxs):
    """The Gram kernel has its own slabs (FISHER_SLAB bins per workgroup): the likelihood tile's geometry option must not leak into it.
    N = 17 on a context set to 64 x 16, then back at 64 x 8."""
    c = ctxs["fast"]
    c.set_option(pkg.OPT_WORKGROUP, 64)
    c.set_option(pkg.OPT_BINS_PER_THREAD, 16)
    try:
        test_weighted_gram_is_exact_on_small_integers(pkg, ctxs, 17)
    finally:
        c.set_option(pkg.OPT_BINS_PER_THREAD, 8)


@pytest.mark.parametrize("name", ["c2", "corner", "c3_asym"])
def test_fisher_within_the_row_tolerance_of_the_yardstick(pkg, oracle, synth, ctxs, name):
    """c2: Nv 21, 4000 bins; corner: Nv 33, 4000 bins, l = 3 rows, clamped windows, asymmetry, a switched-off Harvey term (two variables whose
    rows of F are zero); c3_asym: Nv 57, 20 000 bins, four 16x16 blocks per side.
    The largest |F_dev - F_ref| / B of every configuration is printed; DESIGN section 9 records it (it has to stay below 0.5).
    c2 also at 256 x 1, 256 x 2 and 64 x 16 in both FAST modes."""
    star, y, F_ref, U, happ, h = fn.cached(pkg, oracle, synth, name)
    idx = star.index_to_relax
    B = fn.bound(U, happ, star.x.size)
    dead = np.flatnonzero(np.diag(F_ref) == 0)
    if name == "corner":
        assert dead.size == 2 and not F_ref[dead].any()
    print("\n%s: Nv %d, bound at most %.2e, median %.2e of sqrt(F_jj F_kk)" % (name, idx.size, np.max(B / fn.scale(F_ref)), np.median(B / fn.scale(F_ref))))
    for cfg in CONFIGS + (NO_DELTA_CONFIGS if name == "c2" else []):
        c = _configured(pkg, ctxs, cfg, star, y)
        F = c.fisher(star.model_id, star.params, star.plength, idx, h)[0]
        assert c.last_fisher_status == 0 and np.all(np.isfinite(F))
        ratio = np.max(np.abs(F - F_ref) / B)
        print("%s %s: largest |F_dev - F_ref| / B = %.3f (%.2e)" % (name, cfg, ratio, ratio))
        assert np.all(np.abs(F - F_ref) <= 2 * B), (cfg, np.argwhere(np.abs(F - F_ref) > 2 * B)[:4])
        assert not F[dead].any() and not F[:, dead].any()


def test_fisher_properties(pkg, oracle, synth, ctxs):
    """Symmetry bit for bit, positive semi-definiteness, same bits twice, a chain's F the same bits alone / as one of three / one chain per
    pass (TAMCMC_OPT_FISHER_WORKSPACE_MB = 1 on c2: 1 344 000 B per chain), F(T, p) = F(1, 1) p / T."""
    star, y, _, _, _, h = fn.cached(pkg, oracle, synth, "c2")
    idx = star.index_to_relax
    P = np.tile(star.params, (3, 1))
    P[1:, idx] *= 1 + 0.003 * np.random.default_rng(7).standard_normal((2, idx.size))
    T = np.array([1.0, 3.5, 150.0])
    for cfg in CONFIGS:
        c = _configured(pkg, ctxs, cfg, star, y)
        F = c.fisher(star.model_id, P, star.plength, idx, h, T, 2.0)
        assert np.all(np.isfinite(F))
        assert np.array_equal(c.fisher(star.model_id, P, star.plength, idx, h, T, 2.0), F)
        for ch in range(3):
            assert np.array_equal(F[ch], F[ch].T)
            assert np.all(np.diag(F[ch]) >= 0)
            assert np.linalg.eigvalsh(F[ch] / fn.scale(F[ch]))[0] >= -1e-12
            alone = c.fisher(star.model_id, P[ch], star.plength, idx, h, T[ch:ch + 1], 2.0)[0]
            assert np.array_equal(alone, F[ch]), (cfg, ch)
            F11 = c.fisher(star.model_id, P[ch], star.plength, idx, h)[0]
            want = F11 * 2.0 / T[ch]
            assert np.all(np.abs(F[ch] - want) <= np.spacing(np.abs(want))), (cfg, ch)
        assert not np.array_equal(F[0] * T[0], F[1] * T[1])      # (the three chains are different points)
        c.set_option(pkg.OPT_FISHER_WORKSPACE_MB, 1)
        try:
            assert np.array_equal(c.fisher(star.model_id, P, star.plength, idx, h, T, 2.0), F), cfg
        finally:
            c.set_option(pkg.OPT_FISHER_WORKSPACE_MB, 2048)


def test_failed_tables_mark_their_rows_and_nothing_else(pkg, oracle, synth, ctxs):
    """The failure contract.  A perturbed vector whose table fails (a step of NaN on a width: TAMCMC_ERR_NAN_WINDOW at theta +- h e_k) makes
    the call return that status and row and column k of F NaN; every other element keeps its bits.  A chain whose BASE table fails (a NaN
    width in its vector) is NaN throughout, and the chains beside it keep their bits."""
    star, y, _, _, _, h = fn.cached(pkg, oracle, synth, "c2")
    idx = star.index_to_relax
    kW = [k for k, i in enumerate(idx) if star.names[i].startswith("Width")][1]
    P = np.tile(star.params, (3, 1))
    P[1:, idx] *= 1 + 0.003 * np.random.default_rng(8).standard_normal((2, idx.size))
    T = np.array([1.0, 3.5, 150.0])
    for cfg in (CONFIGS[0], CONFIGS[3]):
        c = _configured(pkg, ctxs, cfg, star, y)
        good = c.fisher(star.model_id, P, star.plength, idx, h, T, 1.0)
        assert c.last_fisher_status == 0
        hb = h.copy()
        hb[kW] = np.nan
        F = c.fisher(star.model_id, P, star.plength, idx, hb, T, 1.0)
        assert c.last_fisher_status == pkg.ERR_NAN_WINDOW
        keep = np.ones(idx.size, dtype=bool)
        keep[kW] = False
        assert np.all(np.isnan(F[:, kW, :])) and np.all(np.isnan(F[:, :, kW]))
        assert np.array_equal(F[:, keep][:, :, keep], good[:, keep][:, :, keep])
        Pb = P.copy()
        Pb[1, idx[kW]] = np.nan
        F = c.fisher(star.model_id, Pb, star.plength, idx, h, T, 1.0)
        assert c.last_fisher_status == pkg.ERR_NAN_WINDOW
        assert np.all(np.isnan(F[1])) and np.array_equal(F[0], good[0]) and np.array_equal(F[2], good[2])


def test_refusals(pkg, oracle, synth, ctxs):
    star, y, _, _, _, h = fn.cached(pkg, oracle, synth, "c2")
    idx = star.index_to_relax
    c = _configured(pkg, ctxs, CONFIGS[0], star, y)
    for model_id in (1, 25):
        with pytest.raises(pkg.TamcmcError) as e:
            c.fisher(model_id, star.params, star.plength, idx, h)
        assert e.value.code == pkg.ERR_BAD_MODEL
    strict = pkg.HipContext(0, precision=pkg.PRECISION_STRICT)
    try:
        strict.set_spectrum(star.x, y)
        with pytest.raises(pkg.TamcmcError) as e:
            strict.fisher(star.model_id, star.params, star.plength, idx, h)
        assert e.value.code == pkg.ERR_BAD_ARG
    finally:
        strict.close()


@pytest.mark.parametrize("engine", ["host", "device"])
def test_sampler_seeds_its_proposal_law(pkg, oracle, synth, engine):
    """Sigma_m = E (I + E F_m E)^-1 E from the returned F within 1e-9 e_j e_k (I + E F E has eigenvalues in [1, ~150]: four digits of room),
    symmetric, never wider than the default law, mu and sigma untouched, and the chains run on from it."""
    from tamcmc_c_amd.sampler import default_errors
    star = synth.make_c2_star(nx=4000)
    _, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    star.set_spectrum_from_model(m0, 5)
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    try:
        ctx.set_spectrum(star.x, star.y)
        kw = dict(nchains=4, lambda_temp=3.5, seed=21, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,), engine=engine)
        s = pkg.Sampler(ctx, star, **kw)
        e = default_errors(star)
        mu0, cov0, sig0 = s.proposal_law()
        assert np.array_equal(cov0[0], np.diag(e * e))
        F = s.seed_proposal_fisher()
        assert F.shape == (4, s.nvars, s.nvars) and np.all(np.isfinite(F))
        T = 3.5 ** np.arange(4)
        assert np.allclose(F[3] * T[3], F[0], rtol=1e-12)        # (all chains start at the same point: F_m = F_0 / T_m)
        mu1, cov1, sig1 = s.proposal_law()
        assert np.array_equal(mu1, mu0) and np.array_equal(sig1, sig0)
        ee = e[:, None] * e[None, :]
        for m in range(4):
            A = np.eye(s.nvars) + ee * F[m]
            assert np.linalg.eigvalsh(A)[0] >= 1 - 1e-9
            want = ee * np.linalg.inv(A)
            assert np.all(np.abs(cov1[m] - want) <= 1e-9 * ee), (m, np.max(np.abs(cov1[m] - want) / ee))
            assert np.array_equal(cov1[m], cov1[m].T)
            assert np.all(np.diag(cov1[m]) <= e * e)
        assert np.min(np.diag(cov1[0]) / (e * e)) < 0.5          # (the data do narrow the law somewhere)
        smp, stt = s.run(50, stats=True)
        assert np.all(np.isfinite(smp)) and np.all(np.isfinite(stt))
        assert s.state()["accepted0"] >= 1
        s.close()
        # never called: nothing changes
        a, b = pkg.Sampler(ctx, star, **kw), pkg.Sampler(ctx, star, **kw)
        sa, ta = a.run(50, stats=True)
        sb, tb = b.run(50, stats=True)
        assert np.array_equal(sa, sb) and np.array_equal(ta, tb)
        assert np.array_equal(a.proposal_law()[1][0], np.diag(e * e))
        a.close(); b.close()
    finally:
        ctx.close()

"""Height-per-m models on the GPU (-m gpu): ids 12, 13, 14 (model_MS_Global_a1etaa3_HarveyLike_Classic_v2 / _v3, model_MS_local_Hnlm)
through every entry that takes a model id.  The oracle does not know these ids; the checkers are (1) the inclination models it does know,
by conversion (synth.classic_to_v2 / classic_to_v3 / local_to_hnlm with the oracle's amplitude_ratio), and (2) the independent numpy
restatement tests/hnlm_numpy.py evaluated by strict_numpy.eval_table.
Which builder made the rows: HipContext.loglike_params_batch builds its tables on the HOST (mode_tables.cpp) and runs the likelihood tile on
them -- the tests that use it check the host builder and the tile on the device.  The DEVICE unpack (the same source compiled into
k_fd_unpack, k_iterate, k_step) is reached through fd_gradient / fd_gradient_posterior and the device-resident sampler:
test_device_unpack_against_host_tables_and_numpy, the gradient test and the engine tests.  Tolerances: those of smoke() -- |dlogL| / |logL| <= 1e-12 STRICT,
1e-11 FAST -- and bit identity where the operations are the same (id 12 against id 3; fused step against lockstep kernels)."""
import numpy as np
import pytest

import hnlm_numpy
from strict_numpy import eval_table
from test_hnlm_models import random_vector

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctxs(pkg):
    c = {"strict": pkg.HipContext(0, precision=pkg.PRECISION_STRICT), "fast": pkg.HipContext(0, precision=pkg.PRECISION_FAST)}
    yield c
    for v in c.values():
        v.close()


def _spectrum(oracle, star, model_id=None, params=None, plength=None, seed=7):
    _, m0 = oracle.call_model(model_id or star.model_id, star.params if params is None else params,
                              star.plength if plength is None else plength, star.x)
    return star.set_spectrum_from_model(m0, seed)


def _white_noise_above_one(p, pl):
    """Sets the white-noise level to 2: the model is then > 1 in every bin, every term y/M + ln M of logL is positive and |logL| is of
    the size of its partial sums.  With a level below 1 the ln M terms are negative, the sum can cancel to a small fraction of them (a
    perturbed vector of the stock star gave |logL| = 183 against partial sums of 3e4), and a tolerance RELATIVE to |logL| -- what the
    library states and smoke() checks -- then measures the cancellation, not the arithmetic."""
    p[int(np.sum(pl[:9])) - 1] = 2.0
    return p


def _perturbed(p, idx, B, rng, amp):
    P = np.tile(p, (B, 1))
    P[1:, idx] *= 1.0 + amp * rng.standard_normal((B - 1, len(idx)))
    return P


@pytest.mark.parametrize("nx,nmax,step", [(100000, 14, 0.02), (20000, 14, 0.1)])
def test_v2_is_bitwise_classic_on_the_device(pkg, oracle, synth, ctxs, nx, nmax, step):
    """Headline shape (1e5 bins, 56 multiplets) and a coarser grid: id 12 with ratios = amplitude_ratio(l, i) against id 3 -- STRICT and
    FAST logL and the STRICT model rows identical, and both within the stated tolerance of oracle.loglike_batch(3, ...)."""
    s3 = synth.make_classic_star(nx=nx, nmax=nmax, step=step)
    _white_noise_above_one(s3.params, s3.plength)
    y = _spectrum(oracle, s3)
    rng = np.random.default_rng(3)
    B = 6
    free = [i for i in s3.index_to_relax if s3.names[i] != "Inclination"]
    P3 = _perturbed(s3.params, free, B, rng, 0.002)
    o = int(s3.plength[:9].sum())
    P3[:, o] = rng.uniform(5.0, 85.0, B)
    conv = [synth.classic_to_v2(p, s3.plength, oracle.amplitude_ratio) for p in P3]
    P12, pl12 = np.stack([c[0] for c in conv]), conv[0][1]
    T = 1.3 ** np.arange(B)
    ref, _, _ = oracle.loglike_batch(3, P3[:2], s3.plength, s3.x, y, 1.0, T[:2])
    for name, tol in (("strict", 1e-12), ("fast", 1e-11)):
        c = ctxs[name]
        c.set_spectrum(s3.x, y)
        a, ma, sa = c.loglike_params_batch(3, P3, s3.plength, T, 1.0, want_model=(name == "strict"))
        b, mb, sb = c.loglike_params_batch(12, P12, pl12, T, 1.0, want_model=(name == "strict"))
        assert (sa == 0).all() and (sb == 0).all()
        assert np.array_equal(a, b), name
        if name == "strict":
            assert np.array_equal(ma, mb)
        err = np.max(np.abs(b[:2] - ref) / np.abs(ref))
        print("\nid 12 vs oracle id 3 (%s): %.2e" % (name, err))
        assert err < tol, (name, err)


@pytest.mark.parametrize("model_id", [13, 14])
def test_component_heights_against_the_inclination_models(pkg, oracle, synth, ctxs, model_id):
    """l <= 1 stars, where the offsets of the model functions and of the loaders coincide: ids 13 / 14 against oracle ids 3 / 11."""
    rng = np.random.default_rng(17 + model_id)
    B = 5
    if model_id == 13:
        s = synth.make_classic_star(nx=60000, nmax=10, lmax=1, step=0.03, fmin=2000.0)
        src_id, conv = 3, synth.classic_to_v3
    else:
        s = synth.make_c2_star(nx=10000)
        keep = np.r_[0:4, 6:10, 12:18, 18:22, 24:28]
        s.params, s.relax = s.params[keep], s.relax[keep]
        s.plength = np.array([4, 0, 2, 2, 0, 0, 6, 4, 1, 1, 2], dtype=np.int32)
        src_id, conv = 11, synth.local_to_hnlm
    _white_noise_above_one(s.params, s.plength)
    y = _spectrum(oracle, s, src_id)
    for do_amp in (0.0, 1.0):
        base = s.params.copy()
        base[-1] = do_amp
        if do_amp:
            base[:s.plength[0]] *= 3.0
        P = _perturbed(base, s.index_to_relax, B, rng, 0.003)
        out = [conv(p, s.plength, oracle.amplitude_ratio) for p in P]
        Pn, pln = np.stack([c[0] for c in out]), out[0][1]
        T = 1.4 ** np.arange(B)
        ref, _, _ = oracle.loglike_batch(src_id, P, s.plength, s.x, y, 1.0, T)
        for name, tol in (("strict", 1e-12), ("fast", 1e-11)):
            c = ctxs[name]
            c.set_spectrum(s.x, y)
            got, _, st = c.loglike_params_batch(model_id, Pn, pln, T, 1.0)
            assert (st == 0).all()
            err = np.max(np.abs(got - ref) / np.abs(ref))
            print("\nid %d vs oracle id %d (%s, do_amp %d): %.2e" % (model_id, src_id, name, do_amp, err))
            assert err < tol, (name, do_amp, err)


@pytest.mark.parametrize("model_id,lmax,do_amp", [(12, 1, 0), (12, 3, 1), (13, 1, 1), (13, 2, 0), (13, 3, 1), (14, 1, 0), (14, 2, 0), (14, 3, 1)])
def test_device_against_the_numpy_restatement(pkg, synth, ctxs, model_id, lmax, do_amp):
    """Random vectors that are not images of an inclination (asymmetric patterns, a zero height), offsets quirks included: STRICT model rows
    and logL, FAST logL, against hnlm_numpy.rows evaluated in the reference's per-bin order."""
    rng = np.random.default_rng(1000 * model_id + 10 * lmax + do_amp)
    vecs = [random_vector(synth, rng, model_id, lmax, do_amp) for _ in range(3)]
    for p, pl, _ in vecs:
        _white_noise_above_one(p, pl)
    x = vecs[0][2]
    refs = []
    for p, pl, _ in vecs:
        m, nz, nh = hnlm_numpy.rows(model_id, p, pl, x)
        refs.append(eval_table(m, nz, nh, x))
    y = refs[0] * np.random.default_rng(1).exponential(1.0, x.size)
    T = np.array([1.0, 1.5, 2.25])
    want = np.array([-float(np.sum(np.asarray(y / r + np.log(r), dtype=np.longdouble))) / t for r, t in zip(refs, T)])
    P, pl = np.stack([v[0] for v in vecs]), vecs[0][1]
    for name, tol in (("strict", 1e-12), ("fast", 1e-11)):
        c = ctxs[name]
        c.set_spectrum(x, y)
        got, model, st = c.loglike_params_batch(model_id, P, pl, T, 1.0, want_model=(name == "strict"))
        assert (st == 0).all()
        if name == "strict":
            assert np.max(np.abs(model - np.stack(refs)) / np.stack(refs)) < 1e-12
        err = np.max(np.abs(got - want) / np.abs(want))
        assert err < tol, (name, err)


@pytest.mark.parametrize("nx", [3, 64, 511, 512, 513, 1025, 4097])
def test_awkward_grids(pkg, synth, ctxs, nx):
    """The grids of test_random_tables_on_awkward_grids: windows clipped at both ends, grids shorter than a wave, either side of a tile."""
    for model_id in (12, 13, 14):
        rng = np.random.default_rng(nx + model_id)
        p, pl, x0 = random_vector(synth, rng, model_id, 3, 1)
        o_f0 = int(pl[0] + pl[1])
        fmid = p[o_f0 + 1]
        step = 0.05
        x = fmid - 0.4 * nx * step + step * np.arange(nx)
        p[-2] = 4.0  # trunc_c: narrow windows, most of them outside this grid
        st, m, nz, nh = pkg.build_mode_table(model_id, p, pl, x)
        ref_rows = hnlm_numpy.rows(model_id, p, pl, x)
        c = ctxs["strict"]
        y = np.full(nx, 1.0)
        c.set_spectrum(x, y)
        got, model, status = c.loglike_params_batch(model_id, p[None, :], pl, [1.0], 1.0, want_model=True)
        assert status[0] == st
        if st == 0:
            ref = eval_table(*ref_rows, x)
            assert np.max(np.abs(model[0] - ref) / ref) < 1e-12
            f = ctxs["fast"]
            f.set_spectrum(x, y)
            gf, _, _ = f.loglike_params_batch(model_id, p[None, :], pl, [1.0], 1.0)
            assert abs(gf[0] - got[0]) <= 1e-11 * abs(got[0])


def _numpy_logl(model_id, p, pl, x, y, T):
    m, nz, nh = hnlm_numpy.rows(model_id, p, pl, x)
    M = eval_table(m, nz, nh, x)
    terms = np.asarray(y / M + np.log(M), dtype=np.longdouble)
    return -float(np.sum(terms)) / T, float(np.sum(np.abs(terms))) / T


@pytest.mark.parametrize("model_id,do_amp", [(12, 0), (12, 1), (13, 0), (13, 1), (14, 0), (14, 1)])
def test_device_unpack_against_host_tables_and_numpy(pkg, synth, ctxs, model_id, do_amp):
    """Rows unpacked ON THE DEVICE (k_fd_unpack: shared_scalars_base, build_multiplet, component_heights in wg_unpack) for vectors that are
    not images of an inclination -- lmax = 3 with the offset quirks, asymmetric patterns, a zero height, do_amp on and off; ids 12, 13 at
    the headline size (56 multiplets, 1e5 bins), id 14 at the local-slice size -- on the UNMODIFIED noise levels of the generators.
    (1) the base-point logL that fd_gradient returns against loglike_params_batch of the same vectors (host-built tables, same tile) and
    against the numpy restatement; (2) the forward-difference gradient against the same difference of the numpy restatement.
    Bounds: the host builder forms nu_nlm and the heights in long double, the device in double (1-2 ulp apart, mode_tables_impl.h), so
    host and device tables are not bit-equal; the stated 1e-12 (STRICT) / 1e-11 (FAST), here relative to the sum of |terms| of logL (the
    scale of its rounding error; on these vectors the sum itself can cancel to a small fraction of that).  Gradient: the bound of
    test_windowed_fd_matches_full_fd against the oracle, 5e-14 Nx / h of cancellation noise + 1e-6 of the gradient's scale."""
    rng = np.random.default_rng(7000 + 10 * model_id + do_amp)
    big = model_id != 14
    vecs = [random_vector(synth, rng, model_id, 3, do_amp, nfreqs=14 if big else 5) for _ in range(2)]
    pl = vecs[0][1]
    x = synth.grid(100000, 1500.0, 0.02) if big else vecs[0][2]
    P = np.stack([v[0] for v in vecs])
    T = np.array([1.0, 1.6])
    m0, nz0, nh0 = hnlm_numpy.rows(model_id, P[0], pl, x)
    assert len(m0) == (56 if big else 10)
    y = eval_table(m0, nz0, nh0, x) * np.random.default_rng(2).exponential(1.0, x.size)
    ref = [_numpy_logl(model_id, P[b], pl, x, y, T[b]) for b in range(2)]
    want, scale = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
    lay = hnlm_numpy.layout(pl)
    o_f0, o_split, o_width, o_inc = lay[3], lay[4], lay[5], lay[7]
    hb = np.arange(lay[0]) if model_id == 14 else np.arange(o_inc, o_inc + pl[9])      # the block that holds the component heights
    idx = np.unique(np.r_[hb[:24], hb[-6:], 0, o_f0, o_f0 + pl[2], o_split, o_width]).astype(np.int32)
    h = 1e-6 * np.maximum(np.abs(P[0][idx]), 1e-2)
    for name, tol in (("strict", 1e-12), ("fast", 1e-11)):
        c = ctxs[name]
        c.set_spectrum(x, y)
        host, _, st = c.loglike_params_batch(model_id, P, pl, T, 1.0)
        assert (st == 0).all()
        l0, g = c.fd_gradient(model_id, P, pl, idx, h, T, 1.0)
        print("\nid %d do_amp %d %s: device unpack vs host tables %.2e, vs numpy %.2e (of the sum of |terms|)"
              % (model_id, do_amp, name, np.max(np.abs(l0 - host) / scale), np.max(np.abs(l0 - want) / scale)))
        assert np.all(np.abs(l0 - host) <= tol * scale), name
        assert np.all(np.abs(l0 - want) <= tol * scale), name
        assert np.all(np.abs(host - want) <= tol * scale), name
        g_ref = np.zeros(idx.size)
        for k, i in enumerate(idx):
            q = P[0].copy()
            q[i] = q[i] + h[k]
            g_ref[k] = (_numpy_logl(model_id, q, pl, x, y, T[0])[0] - want[0]) / (q[i] - P[0][i])
        bound = 5e-14 * x.size / h + 1e-6 * np.max(np.abs(g_ref))
        assert np.all(np.abs(g[0] - g_ref) <= bound), (name, np.max(np.abs(g[0] - g_ref) / bound))
        assert np.count_nonzero(g_ref) >= idx.size // 2
        assert np.all(g[0][g_ref == 0] == 0)             # slots the offset quirk never reads: no gradient on the device either


def _fd_star(synth, oracle, model_id):
    if model_id == 14:
        s = synth.make_hnlm_star(oracle.amplitude_ratio, nx=10000)
    else:
        s = synth.make_v2_star(oracle.amplitude_ratio, nx=40000, nmax=8, step=0.05, fmin=2000.0)
        if model_id == 13:   # model level only: the Classic star with a v3 height block, every height free
            c3 = synth.make_classic_star(nx=40000, nmax=8, step=0.05, fmin=2000.0)
            p13, pl13 = synth.classic_to_v3(c3.params, c3.plength, oracle.amplitude_ratio)
            o = int(c3.plength[:9].sum())
            relax = np.r_[c3.relax[:o], np.ones(pl13[9], dtype=np.int32), c3.relax[o + 1:]]
            s = synth.Star(13, p13, pl13, c3.x, relax, np.zeros((4, p13.size)), np.zeros(p13.size), None, 0)
    return s


@pytest.mark.parametrize("model_id", [12, 13, 14])
def test_windowed_gradient_matches_brute_force(pkg, oracle, synth, ctxs, model_id):
    """Windowed finite differences against the brute-force batch (both unpack on the device: what is compared is the delta-table path
    against whole evaluations; the rows themselves are checked in test_device_unpack_against_host_tables_and_numpy), at the tolerance of
    test_windowed_fd_matches_full_fd; a height parameter of ids 13 / 14 changes one row's heights only: its delta evaluation touches
    that multiplet's window, not the spectrum."""
    s = _fd_star(synth, oracle, model_id)
    st, m, nz, nh = pkg.build_mode_table(model_id, s.params, s.plength, s.x)
    assert st == 0
    y = s.set_spectrum_from_model(eval_table(m, nz, nh, s.x), 9)
    idx = s.index_to_relax
    h = 1e-6 * np.maximum(np.abs(s.params[idx]), 1e-2)
    T = np.array([1.0, 1.7])
    P = _perturbed(s.params, idx, 2, np.random.default_rng(5), 0.002)
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST, timing=True)
    c.set_spectrum(s.x, y)
    c.set_option(pkg.OPT_FD_WINDOWED, 0)
    l0_f, g_f = c.fd_gradient(model_id, P, s.plength, idx, h, T, 1.0)
    c.set_option(pkg.OPT_FD_WINDOWED, 1)
    c.reset_kernel_stats()
    l0_w, g_w = c.fd_gradient(model_id, P, s.plength, idx, h, T, 1.0)
    bins, evals = c.fd_stats()
    c.close()
    assert np.allclose(l0_w, l0_f, rtol=1e-12)
    scale = np.max(np.abs(g_f), axis=1, keepdims=True)
    tol = 5e-15 * s.x.size / h[None, :] + 1e-6 * scale
    assert np.all(np.abs(g_w - g_f) <= tol)
    assert evals == 2 * (idx.size + 1) and 0 < bins < 0.5 * evals * s.x.size, (bins, evals)


def _sampler_star(pkg, oracle, synth, model_id, nx=4000, seed=5):
    if model_id == 14:
        s = synth.make_hnlm_star(oracle.amplitude_ratio, nx=nx)
    elif model_id == 12:
        s = synth.make_v2_star(oracle.amplitude_ratio, nx=nx, nmax=5, lmax=2, step=0.2, fmin=2200.0)
    else:
        s = synth.make_classic_star(nx=nx, nmax=5, lmax=2, step=0.2, fmin=2200.0)
    st, m, nz, nh = pkg.build_mode_table(s.model_id, s.params, s.plength, s.x)
    assert st == 0
    s.set_spectrum_from_model(eval_table(m, nz, nh, s.x), seed)
    return s


@pytest.mark.parametrize("model_id", [12, 14])
@pytest.mark.parametrize("drift", [0, 1])
def test_device_engine_follows_host_engine(pkg, oracle, synth, model_id, drift):
    """Same Philox draws, same algorithm: one iteration and a short walk of the two engines coincide until a knife-edge decision
    (bounds of test_device_engine_follows_host_engine / test_device_langevin_engine_follows_the_host_engine)."""
    star = _sampler_star(pkg, oracle, synth, model_id)
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    ctx.set_spectrum(star.x, star.y)
    kw = dict(nchains=5, lambda_temp=1.5, seed=11, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,), dN_mixing=1, use_drift=drift)
    if drift:
        kw.update(Nt_learn=(20, 60), c0=3.0)
    h = pkg.Sampler(ctx, star, engine="host", **kw)
    d = pkg.Sampler(ctx, star, engine="device", **kw)
    a0, b0 = h.state(), d.state()
    assert np.allclose(a0["logL"], b0["logL"], rtol=1e-11) and np.allclose(a0["logPrior"], b0["logPrior"], rtol=1e-13)
    assert np.all(np.isfinite(a0["logPrior"]))
    n = 90
    sh, th = h.run(n, stats=True)
    sd1, td1 = d.run(50, stats=True)
    sd2, td2 = d.run(n - 50, stats=True)             # a second call continues the same chains
    sd, td = np.concatenate([sd1, sd2]), np.concatenate([td1, td2])
    if drift:
        dev = np.max(np.abs(sh - sd) / (np.abs(sh) + 1e-3), axis=(1, 2))
        same, need = dev < 1e-4, 40
    else:
        same, need = np.all(np.isclose(sh, sd, rtol=1e-9, atol=1e-12), axis=(1, 2)), 60
    first_div = n if same.all() else int(np.argmin(same))
    assert same[0] and first_div >= need, f"engines diverge at iteration {first_div}"
    assert np.allclose(th[:first_div], td[:first_div], rtol=1e-5 if drift else 1e-9, atol=1e-3 if drift else 1e-7)
    a, b = h.state(), d.state()
    assert a["iteration"] == b["iteration"] == n and a["swap_attempts"] == b["swap_attempts"] == n - 1
    assert abs(a["swaps"] - b["swaps"]) <= 6
    assert (sh[:, 0] != sh[0, 0]).any()
    h.close(); d.close(); ctx.close()


@pytest.mark.parametrize("model_id,nchains", [(12, 7), (14, 7), (12, 9)])
def test_fused_step_is_bitwise_the_lockstep_chain(pkg, oracle, synth, model_id, nchains):
    """Lockstep kernels, fused step, fused step with TAMCMC_OPT_QUICK_DECIDE = 1: the same chains bit for bit (the deferred-visibility
    paths of the fused step's helper wave included)."""
    star = _sampler_star(pkg, oracle, synth, model_id)
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    ctx.set_spectrum(star.x, star.y)
    kw = dict(nchains=nchains, lambda_temp=1.4, seed=23, Nt_learn=(40, 90), periods_learn=(2,), dN_mixing=1)
    out, infos = [], []
    fused = 0 if nchains < 8 else 3
    for scheme, forced in ((1, 0), (fused, 0), (fused, 1)):
        ctx.set_option(pkg.OPT_STEP_SCHEME, scheme)
        ctx.set_option(pkg.OPT_QUICK_DECIDE, forced)
        d = pkg.Sampler(ctx, star, engine="device", **kw)
        s1, t1 = d.run(200, stats=True)
        out.append((s1, t1, d.state()))
        infos.append(d.info())
        d.close()
    ctx.close()
    assert infos[0]["iter_fused"] == 0 and infos[1]["fused_available"] == 1 and infos[1]["iter_fused"] > 100
    assert infos[2]["quick_fallbacks"] > 0
    for k in (1, 2):
        assert np.array_equal(out[k][0], out[0][0]) and np.array_equal(out[k][1], out[0][1])
        for key in ("vars", "logL", "logPrior", "logPost", "Pmove", "sigma"):
            assert np.array_equal(out[k][2][key], out[0][2][key]), key
    assert (out[0][0][1:, 0] != out[0][0][:-1, 0]).any()


def test_packed_v2_and_classic_stars_side_by_side(pkg, oracle, synth):
    from tamcmc_c_amd import sampler as S
    stars = [_sampler_star(pkg, oracle, synth, 12, seed=5), _sampler_star(pkg, oracle, synth, 3, seed=5)]

    def build():
        cs, ss = [], []
        for k, st in enumerate(stars):
            c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
            c.set_spectrum(st.x, st.y)
            cs.append(c)
            ss.append(pkg.Sampler(c, st, engine="device", nchains=4 + 2 * k, lambda_temp=1.5, seed=40 + k, Nt_learn=(20, 160), periods_learn=(1,)))
        return cs, ss

    n = 240
    cs, ss = build()
    solo = [s.run(n, stats=True) for s in ss]
    for s in ss:
        s.close()
    for c in cs:
        c.close()
    cs, ss = build()
    smp, stt = S.run_packed(ss, n, stats=True)
    for k in range(2):
        assert np.array_equal(smp[k], solo[k][0]) and np.array_equal(stt[k], solo[k][1]), k
        assert (smp[k][1:, 0] != smp[k][:-1, 0]).any()
    for s in ss:
        s.close()
    for c in cs:
        c.close()


def test_posterior_of_the_ratios_covers_the_injected_inclination(pkg, oracle, synth):
    """Inject an inclination (the id-12 star is the image of a Classic star at i = truth), fit id 12 with the random-walk and the
    Langevin sampler: the posterior of every free ratio covers amplitude_ratio(l, i) -- the truth within 4 posterior sigma of the
    mean (one noise realisation moves the posterior by ~1 sigma) -- and the two samplers agree on every mean within 4.5 combined
    Monte-Carlo errors (mc_stats.compare_chains), in the style of test_langevin_and_random_walk_sample_the_same_posterior..."""
    import mc_stats
    star = _sampler_star(pkg, oracle, synth, 12, nx=9000, seed=3)
    o = int(star.plength[:9].sum())
    truth = star.params[o:o + 9].copy()
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    ctx.set_spectrum(star.x, star.y)
    cols = [int(np.flatnonzero(star.index_to_relax == o + k)[0]) for k in range(9) if star.relax[o + k]]
    res = {}
    for drift, n in ((0, 120000), (1, 30000)):
        s = pkg.Sampler(ctx, star, engine="device", use_drift=drift, nchains=4, lambda_temp=1.6, seed=91 + drift, Nt_learn=(100, 4100),
                        periods_learn=(1,), c0=5.0)
        s.run(4100, record=False)
        smp, _ = s.run(n)
        s.close()
        cold = smp[:, 0, :][:, cols]
        acc = np.mean(np.any(smp[1:, 0] != smp[:-1, 0], axis=1))
        assert 0.05 < acc < 0.9, (drift, acc)
        z = (cold.mean(0) - truth[[k for k in range(9) if star.relax[o + k]]]) / cold.std(0)
        print("\ndrift %d: acceptance %.2f, (mean - truth) / sigma of the ratios: %s" % (drift, acc, np.round(z, 2)))
        assert np.all(np.abs(z) < 4), z
        res[drift] = cold
    ctx.close()
    zm, zv, ea, eb = mc_stats.compare_chains(res[0], res[1])
    print("MH vs Langevin on the ratios: ESS min %.0f / %.0f, max |z_mean| %.2f" % (ea.min(), eb.min(), np.abs(zm).max()))
    assert ea.min() > 50 and eb.min() > 30, (ea.min(), eb.min())
    assert np.all(np.abs(zm) < 4.5), zm

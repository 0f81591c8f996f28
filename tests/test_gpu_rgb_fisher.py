"""Expected (Fisher) information of the red-giant models (ids 25 / 27) on the GPU: tamcmc_hip_fisher with TAMCMC_OPT_RGB_FISHER = 1
(csrc/fisher.hip: k_fisher_freeze_rgb, csrc/fisher_rgb_rule.h) and the proposal law seeded from it, against the numpy yardstick of
tests/rgb_fisher_numpy.py on the tables the device builder exports.  Every test here fails without the feature: the option does not exist.

One star for the file, the one tests/test_gpu_rgb_gradient.py builds (4000 bins, 4 radial orders, period spacing 200 s, 25 mixed modes, 35
free parameters), and its id-27 twin; geometries 64 x 8 and 256 x 4, FAST and FAST_DIRECT.

  yardstick     |F_dev - F_ref| <= 2 B elementwise, B = fisher_numpy.bound with h_applied the step of the form used (the derived bound of
                tests/test_gpu_fisher.py);
  forms         central at the star's own parameters, one-sided across a mode-count change, unfrozen for a step of the order of a
                mixed-mode spacing -- each with its counter;
  properties, failure contract, sampler seeding on both engines."""
import ctypes as C

import numpy as np
import pytest

import fisher_numpy as fn
import rgb_fisher_numpy as rf
from test_gpu_rgb_gradient import _small_star, _steps

pytestmark = pytest.mark.gpu

CONFIGS = [("fast", 64, 8), ("fast", 256, 4), ("fast_direct", 64, 8), ("fast_direct", 256, 4)]   # arithmetic, workgroup, bins per thread
KDP_BASE = 199.95987434979568 - 1e-5      # tests/test_gpu_rgb_gradient.py::test_perturbation_that_changes_the_mode_count
KDP_STEP = 2e-5


def _star(synth, oracle, cte):
    star, o = _small_star(synth, cte=cte)
    st, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    assert st == 0 and star.model_id == (27 if cte else 25)
    star.set_spectrum_from_model(m0, 4)
    return star, o


@pytest.fixture(scope="module")
def small(synth, oracle):
    return _star(synth, oracle, False)


@pytest.fixture(scope="module")
def twin27(synth, oracle):
    return _star(synth, oracle, True)


@pytest.fixture(scope="module")
def ctxs(pkg):
    """Timing on (the form counters), the option set."""
    c = {"fast": pkg.HipContext(0, precision=pkg.PRECISION_FAST, timing=True),
         "fast_direct": pkg.HipContext(0, precision=pkg.PRECISION_FAST_DIRECT, timing=True)}
    for v in c.values():
        v.set_option(pkg.OPT_RGB_FISHER, 1)
    yield c
    for v in c.values():
        v.close()


def _configured(pkg, ctxs, cfg, star):
    name, wg, K = cfg
    c = ctxs[name]
    c.set_option(pkg.OPT_WORKGROUP, wg)
    c.set_option(pkg.OPT_BINS_PER_THREAD, K)
    c.set_spectrum(star.x, star.y)
    return c


def _fisher_raw(pkg, c, star, P, idx, h, T=None, p=1.0):
    """tamcmc_hip_fisher as it is: (return code, F) whatever the code."""
    P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
    pl, idx, h = np.ascontiguousarray(star.plength, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(h, dtype=np.float64)
    T = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
    F = np.zeros((P.shape[0], idx.size, idx.size))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = pkg.lib().tamcmc_hip_fisher(c._h, star.model_id, P.shape[0], P.ctypes.data_as(dp), P.shape[1], pl.ctypes.data_as(ip), idx.ctypes.data_as(ip),
                                     idx.size, h.ctypes.data_as(dp), None if T is None else T.ctypes.data_as(dp), float(p), F.ctypes.data_as(dp))
    return rc, F


_REF = {}


def _reference(pkg, ctxs, star, params, idx, h, key, force=None):
    """(F, U, h_applied, forms) of the numpy yardstick on the exported tables, computed once per key (the builder does not depend on the
    arithmetic mode or the geometry: tests/test_gpu_rgb_adjoint.py)."""
    if key not in _REF:
        c = _configured(pkg, ctxs, CONFIGS[0], star)
        exported = rf.export(c, star, params, idx, h)
        _REF[key] = (exported, rf.fisher_rgb(star, params, idx, h, exported))
    if force is not None:
        return rf.fisher_rgb(star, params, idx, h, _REF[key][0], force)
    return _REF[key][1]


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_option_opens_the_red_giant_ids(pkg, small, twin27):
    """Fails without the feature: set_option(16, 1) raises TAMCMC_ERR_BAD_ARG."""
    star, _ = small
    idx = star.index_to_relax
    h = _steps(star.params, idx)
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    try:
        assert pkg.OPT_RGB_FISHER == 16
        c.set_option(pkg.OPT_RGB_FISHER, 1)
        for bad in (2, -1):
            with pytest.raises(pkg.TamcmcError) as e:
                c.set_option(pkg.OPT_RGB_FISHER, bad)
            assert e.value.code == pkg.ERR_BAD_ARG
        for name, wg, K in CONFIGS:                          # both arithmetic modes, both geometries
            c.set_option(pkg.OPT_PRECISION, pkg.PRECISION_FAST if name == "fast" else pkg.PRECISION_FAST_DIRECT)
            c.set_option(pkg.OPT_WORKGROUP, wg)
            c.set_option(pkg.OPT_BINS_PER_THREAD, K)
            for s, _ in (small, twin27):
                c.set_spectrum(s.x, s.y)
                F = c.fisher(s.model_id, np.tile(s.params, (2, 1)), s.plength, s.index_to_relax, _steps(s.params, s.index_to_relax), [1.0, 2.0])
                n = s.index_to_relax.size
                assert F.shape == (2, n, n) and np.all(np.isfinite(F)) and c.last_fisher_status == 0
                assert np.count_nonzero(np.diag(F[0])) >= n - 3
        c.set_option(pkg.OPT_PRECISION, pkg.PRECISION_FAST)
        c.set_spectrum(star.x, star.y)
        with pytest.raises(pkg.TamcmcError) as e:            # id 1 stays refused with the option at 1
            c.fisher(1, star.params, star.plength, idx, h)
        assert e.value.code == pkg.ERR_BAD_MODEL
        c.set_option(pkg.OPT_PRECISION, pkg.PRECISION_STRICT)
        c.set_spectrum(star.x, star.y)
        with pytest.raises(pkg.TamcmcError) as e:
            c.fisher(star.model_id, star.params, star.plength, idx, h)
        assert e.value.code == pkg.ERR_BAD_ARG
        c.set_option(pkg.OPT_PRECISION, pkg.PRECISION_FAST)
        c.set_spectrum(star.x, star.y)
        c.set_option(pkg.OPT_RGB_FISHER, 0)                  # back at 0: today's refusal, whatever the adjoint's option says
        for adj in (0, 1):
            c.set_option(pkg.OPT_RGB_ADJOINT, adj)
            for s, _ in (small, twin27):
                with pytest.raises(pkg.TamcmcError) as e:
                    c.fisher(s.model_id, s.params, s.plength, s.index_to_relax, _steps(s.params, s.index_to_relax))
                assert e.value.code == pkg.ERR_BAD_MODEL
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("which", ["id25", "id27"])
def test_fisher_within_the_row_tolerance_of_the_yardstick(pkg, small, twin27, ctxs, which):
    """Every free variable of the star, at its own parameters: all central.  The largest |F_dev - F_ref| / B of every configuration is
    printed; DESIGN section 9 records it (it has to stay below 0.5).

    Measured (one MI355X): 0.002 (id 25) and 0.001 (id 27) in all four configurations; every variable one-sided against central moves F
    by at most 4.0e-3 (id 25) / 2.5e-3 (id 27) of sqrt(F_jj F_kk) -- the figure include/tamcmc_hip.h states."""
    star, _ = small if which == "id25" else twin27
    idx = star.index_to_relax
    h = _steps(star.params, idx)
    F_ref, U, happ, forms = _reference(pkg, ctxs, star, star.params, idx, h, ("own", which))
    assert forms == [rf.CENTRAL] * idx.size
    B = fn.bound(U, happ, star.x.size)
    print("\n%s: Nv %d, bound at most %.2e, median %.2e of sqrt(F_jj F_kk)" % (which, idx.size, np.max(B / fn.scale(F_ref)), np.median(B / fn.scale(F_ref))))
    # the one-sided form's truncation error (include/tamcmc_hip.h states it by this measurement): here both forms exist for every variable
    for side in (rf.ONE_SIDED_PLUS, rf.ONE_SIDED_MINUS):
        F_os = _reference(pkg, ctxs, star, star.params, idx, h, ("own", which), force={k: side for k in range(idx.size)})[0]
        d = np.abs(F_os - F_ref) / fn.scale(F_ref)
        j, k = np.unravel_index(np.argmax(d), d.shape)
        print("%s: all variables %s against central, largest |dF| / sqrt(F_jj F_kk) = %.2e (variables %d, %d = parameters %d, %d)"
              % (which, side, d[j, k], j, k, idx[j], idx[k]))
    for cfg in CONFIGS:
        c = _configured(pkg, ctxs, cfg, star)
        F = c.fisher(star.model_id, star.params, star.plength, idx, h)[0]
        assert c.last_fisher_status == 0 and np.all(np.isfinite(F))
        assert c.rgb_fisher_stats() == (idx.size, 0, 0)
        ratio = np.max(np.abs(F - F_ref) / np.where(B > 0, B, 1.0))
        print("%s %s: largest |F_dev - F_ref| / B = %.3f" % (which, cfg, ratio))
        assert np.all(np.abs(F - F_ref) <= 2 * B), (cfg, np.argwhere(np.abs(F - F_ref) > 2 * B)[:4])


# ---------------------------------------------------------------------------------------------------------------- 3
def test_one_sided_form_across_a_mode_count_change(pkg, oracle, small, ctxs):
    """Period spacing 199.95987434979568 - 1e-5, step 2e-5: the oracle gives 26 and 25 modes across +h and keeps the base's set across -h,
    so the variable is one-sided on the - side; in the same batch the envelope rotation and an l=0 height are central.  Counter (2, 1, 0).
    Row and column of the variable within 2 B of the one-sided yardstick; and, since that yardstick is the central formula with the +
    slot's row replaced by M0 and the step x0 - x-, the device value is reproduced within B: the substituted side adds exactly zero.
    A device that kept the + table (26 modes) instead would be the unfrozen central difference, which is told apart."""
    star, o = small
    kdp = o[3] + 1
    p = star.params.copy()
    p[kdp] = KDP_BASE
    idx = np.array([kdp, o[6], 0], dtype=np.int32)
    h = np.concatenate([[KDP_STEP], _steps(p, idx[1:])])
    step = star.x[2] - star.x[1]
    vp, vm = p.copy(), p.copy()
    vp[kdp], vm[kdp] = p[kdp] + h[0], p[kdp] + (-h[0])
    m0, mp, mm = (oracle.rgb_modes(v, star.plength, step)[1]["fl1"] for v in (p, vp, vm))
    assert mp.size != m0.size and mm.size == m0.size and rf.modes_linearisable(m0, mm), (m0.size, mp.size, mm.size)
    F_ref, U, happ, forms = _reference(pkg, ctxs, star, p, idx, h, "one-sided")
    assert forms == [rf.ONE_SIDED_MINUS, rf.CENTRAL, rf.CENTRAL]
    assert happ[0] == p[kdp] - vm[kdp]
    B = fn.bound(U, happ, star.x.size)
    F_unf = _reference(pkg, ctxs, star, p, idx, h, "one-sided", force={0: rf.UNFROZEN})[0]
    assert abs(F_unf[0, 0] - F_ref[0, 0]) > 100 * B[0, 0]           # (the two forms are far apart here: the check below tells them apart)
    for cfg in CONFIGS:
        c = _configured(pkg, ctxs, cfg, star)
        F = c.fisher(star.model_id, p, star.plength, idx, h)[0]
        assert c.last_fisher_status == 0 and np.all(np.isfinite(F))
        assert c.rgb_fisher_stats() == (2, 1, 0), cfg
        ratio = np.max(np.abs(F - F_ref) / B)
        print("\n%s: one-sided variable, largest |F_dev - F_ref| / B = %.2e (F_00 = %.6e; unfrozen central would give %.6e)"
              % (cfg, ratio, F[0, 0], F_unf[0, 0]))
        assert np.all(np.abs(F - F_ref) <= 2 * B), (cfg, F, F_ref, B)
        assert np.all(np.abs(F - F_ref) <= B), (cfg, ratio)        # (the substituted side replaced by M0 reproduces the device value)
        assert np.array_equal(c.fisher(star.model_id, p, star.plength, idx, h)[0], F)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_unfrozen_form_for_a_step_of_a_mode_spacing(pkg, oracle, small, ctxs):
    """A step on the period spacing large enough that neither side is linearisable, found on the CPU with the oracle's mode lists and the
    numpy rule (nu dPi / Pi of the order of a mixed-mode spacing: a few seconds).  Counter (2, 0, 1) with two ordinary variables beside
    it; the elements within 2 B of the unfrozen numpy central difference."""
    star, o = small
    kdp = o[3] + 1
    p = star.params.copy()
    step = star.x[2] - star.x[1]
    m0 = oracle.rgb_modes(p, star.plength, step)[1]["fl1"]
    found = None
    for hh in np.arange(0.5, 8.01, 0.25):
        sides = []
        for s in (hh, -hh):
            v = p.copy()
            v[kdp] = p[kdp] + s
            rc, m = oracle.rgb_modes(v, star.plength, step)
            sides.append(rc == 0 and not rf.modes_linearisable(m0, m["fl1"]))
        if all(sides):
            found = hh
            break
    assert found is not None
    idx = np.array([kdp, o[6], 0], dtype=np.int32)
    h = np.concatenate([[found], _steps(p, idx[1:])])
    F_ref, U, happ, forms = _reference(pkg, ctxs, star, p, idx, h, "unfrozen")
    print("\nstep of %.2f s on the period spacing: forms %s" % (found, forms))
    assert forms == [rf.UNFROZEN, rf.CENTRAL, rf.CENTRAL]
    B = fn.bound(U, happ, star.x.size)
    for cfg in CONFIGS:
        c = _configured(pkg, ctxs, cfg, star)
        F = c.fisher(star.model_id, p, star.plength, idx, h)[0]
        assert c.last_fisher_status == 0 and np.all(np.isfinite(F))
        assert c.rgb_fisher_stats() == (2, 0, 1), cfg
        print("%s: unfrozen variable, largest |F_dev - F_ref| / B = %.2e" % (cfg, np.max(np.abs(F - F_ref) / B)))
        assert np.all(np.abs(F - F_ref) <= 2 * B), (cfg, F, F_ref, B)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_fisher_properties(pkg, small, ctxs):
    """As tests/test_gpu_fisher.py::test_fisher_properties: symmetry bit for bit, positive semi-definiteness, same bits twice, a chain's F
    the same bits alone / as one of three / one chain per pass (TAMCMC_OPT_FISHER_WORKSPACE_MB = 1: 2 240 000 B per chain),
    F(T, p) = F(1, 1) p / T within one spacing.  Chain 1 sits at the point of test 3, 1e-5 s from a change of the mode set: the period
    spacing and whichever other variables reach across it are one-sided there, so the independence holds across forms.  The counters
    are the numpy rule's on the exported tables."""
    star, o = small
    idx = star.index_to_relax
    h = _steps(star.params, idx)
    P = np.tile(star.params, (3, 1))
    P[2, idx] *= 1 + 0.002 * np.random.default_rng(12).standard_normal(idx.size)
    kdp = int(np.flatnonzero(idx == o[3] + 1)[0])
    P[1, idx[kdp]] = KDP_BASE
    hh = h.copy()
    hh[kdp] = KDP_STEP
    T = np.array([1.0, 3.5, 150.0])
    c = _configured(pkg, ctxs, CONFIGS[0], star)
    forms = []
    for ch in range(3):
        tabs, _, _ = rf.export(c, star, P[ch], idx, hh)
        forms += [rf.form_of(tabs[0], tabs[1 + k], tabs[1 + idx.size + k]) for k in range(idx.size)]
    counts = (forms.count(rf.CENTRAL), forms.count(rf.ONE_SIDED_PLUS) + forms.count(rf.ONE_SIDED_MINUS), forms.count(rf.UNFROZEN))
    print("\nforms of the three chains (central, one-sided, unfrozen): %s" % (counts,))
    assert forms[idx.size + kdp] == rf.ONE_SIDED_MINUS and forms[:idx.size] == [rf.CENTRAL] * idx.size and counts[1] >= 1
    for cfg in CONFIGS:
        c = _configured(pkg, ctxs, cfg, star)
        F = c.fisher(star.model_id, P, star.plength, idx, hh, T, 2.0)
        assert np.all(np.isfinite(F))
        assert c.rgb_fisher_stats() == counts, cfg
        assert np.array_equal(c.fisher(star.model_id, P, star.plength, idx, hh, T, 2.0), F)
        for ch in range(3):
            assert np.array_equal(F[ch], F[ch].T)
            assert np.all(np.diag(F[ch]) >= 0)
            assert np.linalg.eigvalsh(F[ch] / fn.scale(F[ch]))[0] >= -1e-12
            alone = c.fisher(star.model_id, P[ch], star.plength, idx, hh, T[ch:ch + 1], 2.0)[0]
            assert np.array_equal(alone, F[ch]), (cfg, ch)
            F11 = c.fisher(star.model_id, P[ch], star.plength, idx, hh)[0]
            want = F11 * 2.0 / T[ch]
            assert np.all(np.abs(F[ch] - want) <= np.spacing(np.abs(want))), (cfg, ch)
        assert not np.array_equal(F[0] * T[0], F[2] * T[2])      # (different points)
        c.set_option(pkg.OPT_FISHER_WORKSPACE_MB, 1)
        try:
            assert np.array_equal(c.fisher(star.model_id, P, star.plength, idx, hh, T, 2.0), F), cfg
            assert c.rgb_fisher_stats() == counts                        # (summed over the three passes)
        finally:
            c.set_option(pkg.OPT_FISHER_WORKSPACE_MB, 2048)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_failed_tables_mark_their_rows_and_nothing_else(pkg, small, ctxs):
    """A step of NaN on a parameter of the width law (a NaN width: TAMCMC_ERR_NAN_WINDOW at theta +- h e_k; no solver input is touched)
    makes the call return that status and row and column k NaN; every other element keeps its bits.  A chain whose base vector the
    pre-step refuses (the last radial mode pulled below the first: tests/test_gpu_rgb_gradient.py) is NaN throughout, and the chains
    beside it keep their bits.  Failed tables only."""
    star, o = small
    idx = star.index_to_relax
    h = _steps(star.params, idx)
    kW = int(np.flatnonzero((idx >= o[7]) & (idx < o[8]))[-1])     # (the depth of the width law's dip: it reaches widths only)
    P = np.tile(star.params, (3, 1))
    P[1:, idx] *= 1 + 0.002 * np.random.default_rng(12).standard_normal((2, idx.size))
    T = np.array([1.0, 3.5, 150.0])
    for cfg in CONFIGS:
        c = _configured(pkg, ctxs, cfg, star)
        good = c.fisher(star.model_id, P, star.plength, idx, h, T, 1.0)
        assert c.last_fisher_status == 0 and np.all(np.isfinite(good))
        hb = h.copy()
        hb[kW] = np.nan
        F = c.fisher(star.model_id, P, star.plength, idx, hb, T, 1.0)
        assert c.last_fisher_status == pkg.ERR_NAN_WINDOW
        assert c.rgb_fisher_stats() == (3 * (idx.size - 1), 0, 0)        # (the failed pairs are in no count)
        keep = np.ones(idx.size, dtype=bool)
        keep[kW] = False
        assert np.all(np.isnan(F[:, kW, :])) and np.all(np.isnan(F[:, :, kW]))
        assert np.array_equal(F[:, keep][:, :, keep], good[:, keep][:, :, keep])
        Pb = P.copy()
        Pb[1, o[3] - 1] -= 80.0
        rc, F = _fisher_raw(pkg, c, star, Pb, idx, h, T)
        assert rc == pkg.ERR_BAD_ARG
        assert np.all(np.isnan(F[1])) and np.array_equal(F[0], good[0]) and np.array_equal(F[2], good[2])


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("engine,which", [("host", "id25"), ("host", "id27"), ("device", "id25"), ("device", "id27"), ("device_langevin", "id25"),
                                          ("device_langevin", "id27")])
def test_sampler_seeds_its_proposal_law(pkg, small, twin27, engine, which):
    """Sigma_m = E (I + E F_m E)^-1 E from the returned F within max(1e-9, 1e-14 lambda_max(I + E F E)) e_j e_k (the second term is numpy's
    own inverse in double), symmetric, never wider than the default law, mu and sigma untouched, and the chains run on from it.  With
    the option at 0 the call returns TAMCMC_ERR_BAD_MODEL and the law is unchanged."""
    from tamcmc_c_amd.sampler import default_errors
    star, _ = small if which == "id25" else twin27
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    try:
        ctx.set_spectrum(star.x, star.y)
        kw = dict(nchains=4, lambda_temp=3.5, seed=21, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,), engine="host" if engine == "host" else "device")
        if engine == "device_langevin":
            ctx.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 1)
            kw["use_drift"] = 1
        s = pkg.Sampler(ctx, star, **kw)
        e = default_errors(star)
        mu0, cov0, sig0 = s.proposal_law()
        with pytest.raises(pkg.TamcmcError) as err:
            s.seed_proposal_fisher()
        assert err.value.code == pkg.ERR_BAD_MODEL
        mu1, cov1, sig1 = s.proposal_law()
        assert np.array_equal(mu1, mu0) and np.array_equal(cov1, cov0) and np.array_equal(sig1, sig0)
        ctx.set_option(pkg.OPT_RGB_FISHER, 1)
        F = s.seed_proposal_fisher()
        assert F.shape == (4, s.nvars, s.nvars) and np.all(np.isfinite(F))
        T = 3.5 ** np.arange(4)
        assert np.allclose(F[3] * T[3], F[0], rtol=1e-12)        # (all chains start at the same point: F_m = F_0 / T_m)
        mu1, cov1, sig1 = s.proposal_law()
        assert np.array_equal(mu1, mu0) and np.array_equal(sig1, sig0)
        ee = e[:, None] * e[None, :]
        for m in range(4):
            A = np.eye(s.nvars) + ee * F[m]
            ev = np.linalg.eigvalsh(A)
            assert ev[0] >= 1 - 1e-9
            tol = max(1e-9, 1e-14 * ev[-1])
            want = ee * np.linalg.inv(A)
            print("\n%s %s chain %d: lambda_max(I + E F E) = %.3e, largest |dSigma| / (e_j e_k) = %.2e (tolerance %.2e)"
                  % (engine, which, m, ev[-1], np.max(np.abs(cov1[m] - want) / np.where(ee > 0, ee, 1.0)), tol))
            assert np.all(np.abs(cov1[m] - want) <= tol * ee), (m, np.max(np.abs(cov1[m] - want) / np.where(ee > 0, ee, 1.0)))
            assert np.array_equal(cov1[m], cov1[m].T)
            assert np.all(np.diag(cov1[m]) <= e * e)
        assert np.min(np.diag(cov1[0])[e > 0] / (e * e)[e > 0]) < 0.5          # (the data do narrow the law somewhere)
        smp, stt = s.run(50, stats=True)
        assert np.all(np.isfinite(smp)) and np.all(np.isfinite(stt))
        s.close()
    finally:
        ctx.close()

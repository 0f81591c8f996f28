"""The adjoint gradient on the GPU (csrc/adjoint.hip: k_adj_rows, k_adj_noise, k_adj_fold, k_adj_contract) against the 50-digit
definition and the exact replay of tests/adjoint_reference.py, on the cases of tests/adjoint_cases.py.

  fields        tamcmc_hip_adjoint_table's G / Gn against table_adjoint_exact of THE DEVICE'S OWN base table (tamcmc_hip_fd_batch_tables,
                slot c (Nvars + 1)): |G_dev - G_ref| <= 1e-11 Gabs, the header's tolerance, with Gabs from the 50-digit sum; the
                reference differentiates in field space and shares no closed form with the kernel;
  contraction   every component of tamcmc_hip_fd_gradient under the option, inverted to the dS the contraction kernel left
                (dS_from_gradient), against the exact sum of G_dev . (T_e - T_0) over the batch's own exported tables, within the
                rounding bound of the kernel's own operation count (test_contraction_replayed_exactly);
  failures      a failed perturbed table and a failed base table, ids 3 .. 23;
  red giants    the same replay on the hybrid batch of test_gpu_rgb_adjoint.py.

Measured on one MI355X: fields at most 7.0e-14 of the absolute sum (256 x 4; 1.9e-14 at 64 x 8) against 1e-11;
contraction at most 0.114 of its rounding bound (rows64), 0.06 .. 0.09 elsewhere.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import adjoint_cases as ac
import adjoint_numpy as an
import adjoint_reference as ar

pytestmark = pytest.mark.gpu

CONFIGS = [("fast", 64, 8), ("fast", 256, 4), ("fast_direct", 64, 8), ("fast_direct", 256, 4)]   # as test_gpu_adjoint.py
# the geometries that have no DELTA kernel (the adjoint batch is allowed in any geometry, fd_route.h): on the smallest case of each test
NO_DELTA_CONFIGS = [(mode, wg, K) for mode in ("fast", "fast_direct") for wg, K in ((256, 1), (256, 2), (64, 16))]
SMALLEST_FIELD_CASE, SMALLEST_CASE = "corner", "id11"   # (16 rows on 4000 bins, the 50-digit reference shared; 6 rows on 4000 bins)
U = Fraction(1, 2 ** 53)
TOL_G = 1e-11


@pytest.fixture(scope="module")
def ctxs(pkg):
    c = {"fast": pkg.HipContext(0, precision=pkg.PRECISION_FAST), "fast_direct": pkg.HipContext(0, precision=pkg.PRECISION_FAST_DIRECT)}
    for v in c.values():
        v.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT)
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


@pytest.mark.parametrize("name", ac.FIELD_CASES)
def test_fields_against_the_50_digit_definition(pkg, synth, ctxs, name):
    """corner and corner_neg (asymmetry +15 / -15; 16 rows, windows of 50 .. 548 bins, l = 3 rows, rows clamped at the spectrum's edge, a
    Harvey term with tau = 0), three chains, all four configurations.  The reference is of the table the device built, so nothing but
    the three kernels' sums is compared.  The rules on zeros hold exactly."""
    c = ac.case(synth, name)
    s, y = c.star, ac.spectrum(pkg, c)
    E = c.idx.size + 1
    for cfg in CONFIGS + (NO_DELTA_CONFIGS if name == SMALLEST_FIELD_CASE else []):
        ctx = _configured(pkg, ctxs, cfg, s, y)
        tabs, noise, nh, nn, status = ctx.fd_batch_tables(s.model_id, c.P, s.plength, c.idx, c.h)
        assert (status == 0).all()
        G, Gn = ctx.adjoint_table(s.model_id, c.P, s.plength, ac.TEMPS, ac.P_EXP)
        worst = 0.0
        for ch in range(3):
            b = ch * E
            tab = tabs[b]
            assert tab.size == 16 and np.all(tab["asym"] == c.asym) and nn[b] == 7 and nh[b] == 2
            Gw, Ga, Gnw, Gna = ar.cached_table_adjoint(tab, noise[b, :nn[b]], nh[b], s.x, y)
            assert np.count_nonzero(Gw) >= 3 * tab.size and G.shape == (3, tab.size, 17)
            errG, errN = np.abs(G[ch] - Gw), np.abs(Gn[ch, :nn[b]] - Gnw)
            worst = max(worst, np.max(errG / np.where(Ga > 0, Ga, 1.0)), np.max(errN / np.where(Gna > 0, Gna, 1.0)))
            assert np.all(errG <= TOL_G * Ga), (cfg, ch, np.argwhere(errG > TOL_G * Ga)[:4])
            assert np.all(errN <= TOL_G * Gna), (cfg, ch, np.flatnonzero(errN > TOL_G * Gna))
            assert np.all((G[ch] == 0) == (Gw == 0)) and np.all((Gn[ch, :nn[b]] == 0) == (Gnw == 0))
        print("\n%s %s: worst field error %.2e of its 50-digit absolute sum (bound 1e-11)" % (name, cfg, worst))


def _replay(c_name, G, Gn, tabs, noise, nn, g, P, idx, h, T, p, E, nchains):
    """Every chain and component: the device's dS (from g) against the exact contraction of the device's G with the exported tables.
    Returns (worst ratio to the bound, fields seen, per component abs_sum > 0, per component dS of the device)."""
    worst, seen = 0.0, set()
    live = np.zeros((nchains, idx.size), dtype=bool)
    dev = [[None] * idx.size for _ in range(nchains)]
    for ch in range(nchains):
        b = ch * E
        rows = tabs[b].size
        D = 2 + 17 + math.ceil(rows / 64) + 6 + int(nn[b])
        for k in range(idx.size):
            e = b + 1 + k
            assert tabs[e].size == rows
            fields = set()
            dS, ab = ar.contract_exact(G[ch], Gn[ch], tabs[b], noise[b], tabs[e], noise[e], nn[b], fields)
            got = ar.dS_from_gradient(g[ch, k], P[ch, idx[k]], h[k], T[ch], p)
            bound = D * U * ab + 3 * U * abs(dS)
            err = abs(got - dS)
            if bound > 0:
                worst = max(worst, float(err / bound))
            assert err <= bound, (c_name, ch, k, float(got), float(dS), float(err / bound) if bound else math.inf, D)
            seen |= fields
            live[ch, k] = ab > 0
            dev[ch][k] = got
    return worst, seen, live, dev


@pytest.mark.parametrize("name", ac.NAMES)
def test_contraction_replayed_exactly(pkg, synth, ctxs, name):
    """k_adj_contract and the host's assemble_gradient, replayed without a tolerance of convenience.  FAST, 64 x 8, three chains
    (T = 1, 1.3, 2.2, p = 2), index_to_relax = the star's free parameters + the asymmetry + every noise parameter.  For every chain and
    component k

        |dS_from_gradient(g[c][k]) - sum G_dev . dT| <= D 2^-53 sum |G_dev . dT| + 3 x 2^-53 |dS|,   D = 2 + 17 + ceil(rows / 64) + 6 + nn

    with G_dev / Gn_dev from adjoint_table (the header: the bits the batch contracts with) and the tables from fd_batch_tables.  D is
    the roundings one term passes in k_adj_contract as written (the library is built with -ffp-contract=off, so `v += g[m] * (e - b)`
    is a rounded difference, a rounded product and a rounded sum): the difference and the product (2); the row's running sum v, at most
    7 + 7 + 1 + 2 = 17 additions; the lane's `s += v` once per row of the lane, ceil(rows / 64); the six steps of the wave's tree; lane
    0's nn additions of the noise entries.  The 3: assemble_gradient's division by T (long double, then rounded to double: one rounding
    and 2^-11 of one) and by h_applied.
    rows68 / rows132: the second and third pass of the lane loop (no other main-sequence test has more than 64 rows).  *_asym, corner*,
    id3, id11, id13: base asymmetry != 0 with the asymmetry free, so G[row][15] is contracted -- asserted.  rows64 / rows68 / rows132 /
    id12 / id14: base asymmetry 0, where the component's likelihood share is exactly 0 (the header's rule).  corner_neg: negative steps.
    rows68_asym: steps of 2e-3 relative, so that perturbed rows have another window than the base row -- asserted on the exported tables
    -- which the kernel must not read.  corner_negnoise: a negative Harvey height and a negative white noise in the vector.
    id11, the smallest case, also at 256 x 1, 256 x 2 and 64 x 16 in both FAST modes: the geometries whose base launch no other adjoint
    test runs."""
    for cfg in [CONFIGS[0]] + (NO_DELTA_CONFIGS if name == SMALLEST_CASE else []):
        _contraction_replayed_exactly(pkg, synth, ctxs, name, cfg)


def _contraction_replayed_exactly(pkg, synth, ctxs, name, cfg):
    c = ac.case(synth, name)
    s, y = c.star, ac.spectrum(pkg, c)
    ctx = _configured(pkg, ctxs, cfg, s, y)
    E = c.idx.size + 1
    G, Gn = ctx.adjoint_table(s.model_id, c.P, s.plength, ac.TEMPS, ac.P_EXP)
    tabs, noise, nh, nn, status = ctx.fd_batch_tables(s.model_id, c.P, s.plength, c.idx, c.h)
    assert (status == 0).all() and len(tabs) == 3 * E
    l0, g = ctx.fd_gradient(s.model_id, c.P, s.plength, c.idx, c.h, ac.TEMPS, ac.P_EXP)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(l0))
    if c.rows is not None:
        assert all(tabs[ch * E].size == c.rows for ch in range(3))
    worst, seen, live, dev = _replay(name, G, Gn, tabs, noise, nn, g, c.P, c.idx, c.h, ac.TEMPS, ac.P_EXP, E, 3)
    print("\n%s %s: %d rows, worst |dS_dev - dS_exact| at %.3f of the rounding bound; fields contracted %s" % (name, cfg, tabs[0].size, worst, sorted(seen)))
    # the comparison is not between zeros: a component without a term is the asymmetry at asym = 0, an entry of a Harvey term with tau = 0
    # or (ids 13, 14) a height the model never reads
    dead_ok = c.unread(pkg) if name in ("id13", "id14") else np.zeros((3, c.idx.size), dtype=bool)
    dead_ok[:, c.k_asym] |= c.asym == 0.0
    for t in range(len(c.noise_index) // 3):
        if s.params[c.noise_index[3 * t + 1]] == 0.0:
            dead_ok[:, [int(np.flatnonzero(c.idx == c.noise_index[3 * t + f])[0]) for f in range(3)]] = True
    assert np.all(live | dead_ok), np.argwhere(~(live | dead_ok))[:4]
    assert np.count_nonzero(live) >= 3 * c.idx.size // 2
    assert len(seen) >= 3 and 17 in seen and 14 in seen
    for ch in range(3):
        base, asy = tabs[ch * E], tabs[ch * E + 1 + c.k_asym]
        if c.asym != 0.0:    # G[row][15] is contracted, in every row, and by nothing else
            assert np.all(base["asym"] == c.asym) and np.all(asy["asym"] != base["asym"]) and 15 in seen and dev[ch][c.k_asym] != 0
            f15 = set()
            ar.contract_exact(G[ch], Gn[ch], base, noise[ch * E], asy, noise[ch * E + 1 + c.k_asym], nn[ch * E], f15)
            assert f15 == {15}
        else:                # no derivative at asym = 0: the share is 0 exactly although the perturbed table has an asymmetry
            assert np.all(base["asym"] == 0.0) and np.all(asy["asym"] != 0.0)
            assert dev[ch][c.k_asym] == 0 and g[ch, c.k_asym] == 0.0
    if c.step_kind == "large":
        moved = sum(int(np.any((tabs[1 + k]["i0"] != tabs[0]["i0"]) | (tabs[1 + k]["i1"] != tabs[0]["i1"]))) for k in range(c.idx.size))
        print("%s: %d of %d perturbed tables have a row whose window is not the base row's" % (name, moved, c.idx.size))
        assert moved >= 1
    if c.step_kind == "negative":
        assert np.all(c.h < 0)
    if name == "corner_negnoise":
        assert np.all(noise[0, :nn[0]] == np.abs(c.P[0][c.noise_index])) and np.sum(c.P[0][c.noise_index] < 0) == 2


def _adjoint_table_raw(pkg, ctx, model_id, P, plength):
    """tamcmc_hip_adjoint_table with its status RETURNED (HipContext.adjoint_table raises on a failed table and drops the outputs)."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    pl = np.ascontiguousarray(plength, dtype=np.int32)
    n = C.c_int(0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L = pkg.lib()
    st = L.tamcmc_hip_adjoint_table(ctx._h, int(model_id), 0, P.ctypes.data_as(dp), P.shape[1], pl.ctypes.data_as(ip), None, 1.0, None, None, C.byref(n))
    assert st == 0
    G = np.full((P.shape[0], n.value, 17), 7.0)     # (poisoned: zeros must be written)
    Gn = np.full((P.shape[0], max(int(pl[8]), 1)), 7.0)
    st = L.tamcmc_hip_adjoint_table(ctx._h, int(model_id), P.shape[0], P.ctypes.data_as(dp), P.shape[1], pl.ctypes.data_as(ip), None, 1.0,
                                    G.ctypes.data_as(dp), Gn.ctypes.data_as(dp), C.byref(n))
    return st, G, Gn


@pytest.mark.parametrize("name", ["id11", "corner"])
def test_failed_tables_mark_their_component_and_nothing_else(pkg, synth, ctxs, name):
    """The failure contract of the adjoint route, ids 3 .. 23.  A step of NaN on a width (TAMCMC_ERR_NAN_WINDOW at theta + h e_k):
    fd_gradient gives NaN in that component of every chain and the same bits everywhere else; fd_gradient_posterior gives a likelihood
    share of 0 there (the gradient is the prior's share) and the same bits everywhere else.  A base vector with a NaN width: adjoint_table
    returns the status, that chain's G and Gn are all 0 and the chains beside it keep their bits; fd_gradient gives that chain NaN
    throughout and the others their bits."""
    c = ac.case(synth, name)
    s, y = c.star, ac.spectrum(pkg, c)
    idx = s.index_to_relax
    h = an.steps(s.params, idx)
    kW = [k for k, i in enumerate(idx) if s.names[i].startswith("Width")][1]
    keep = np.arange(idx.size) != kW
    for cfg in (CONFIGS[0], CONFIGS[3]):
        ctx = _configured(pkg, ctxs, cfg, s, y)
        l0, g = ctx.fd_gradient(s.model_id, c.P, s.plength, idx, h, ac.TEMPS, ac.P_EXP)
        l0p, pr0, gp = ctx.fd_gradient_posterior(s, c.P, h, ac.TEMPS, ac.P_EXP)
        gprior = ctx.last_grad_prior.copy()
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(gp)) and np.all(g[:, kW] != 0)
        hb = h.copy()
        hb[kW] = np.nan
        l0b, gb = ctx.fd_gradient(s.model_id, c.P, s.plength, idx, hb, ac.TEMPS, ac.P_EXP)
        assert np.all(np.isnan(gb[:, kW])) and np.array_equal(gb[:, keep], g[:, keep]) and np.array_equal(l0b, l0)
        l0q, pr0q, gq = ctx.fd_gradient_posterior(s, c.P, hb, ac.TEMPS, ac.P_EXP)
        gprior_q = ctx.last_grad_prior.copy()
        assert np.array_equal(gq[:, kW], gprior_q[:, kW]) and np.all(np.isfinite(gq))            # likelihood share 0
        assert np.array_equal(gq[:, keep], gp[:, keep]) and np.array_equal(gprior_q[:, keep], gprior[:, keep])
        assert np.array_equal(l0q, l0p) and np.array_equal(pr0q, pr0)
        st, G, Gn = _adjoint_table_raw(pkg, ctx, s.model_id, c.P, s.plength)
        assert st == 0 and np.count_nonzero(G) > 0 and not np.any(G == 7.0)
        Pb = c.P.copy()
        Pb[1, idx[kW]] = np.nan
        stb, Gb, Gnb = _adjoint_table_raw(pkg, ctx, s.model_id, Pb, s.plength)
        assert stb == pkg.ERR_NAN_WINDOW
        assert not Gb[1].any() and not Gnb[1].any()
        assert np.array_equal(Gb[[0, 2]], G[[0, 2]]) and np.array_equal(Gnb[[0, 2]], Gn[[0, 2]])
        l0c, gc = ctx.fd_gradient(s.model_id, Pb, s.plength, idx, h, ac.TEMPS, ac.P_EXP)
        assert np.all(np.isnan(gc[1])) and np.isnan(l0c[1])
        assert np.array_equal(gc[[0, 2]], g[[0, 2]]) and np.array_equal(l0c[[0, 2]], l0[[0, 2]])


def test_red_giant_contraction_replayed_exactly(pkg, oracle):
    """The hybrid red-giant batch of test_gpu_rgb_adjoint.test_contraction_against_numpy_on_the_exported_tables (two chains, T = 1 and
    1.7, the second perturbed by 0.2 %), every slot linearised (rgb_adjoint_stats reports no fallback slot): the same exact replay, with
    rgb_batch_tables as the export and the rows of the base table (not the rows reserved) in the count D."""
    from tamcmc_c_amd import synth
    from test_gpu_rgb_gradient import _small_star, _steps
    star, _ = _small_star(synth)
    st, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    assert st == 0
    star.set_spectrum_from_model(m0, 4)
    idx = star.index_to_relax
    h = _steps(star.params, idx)
    P = np.tile(star.params, (2, 1))
    P[1, idx] *= 1 + 0.002 * np.random.default_rng(12).standard_normal(idx.size)
    T = np.array([1.0, 1.7])
    E = idx.size + 1
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST, timing=True)
    try:
        ctx.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT)
        ctx.set_option(pkg.OPT_RGB_ADJOINT, 1)
        ctx.set_option(pkg.OPT_WORKGROUP, 64)
        ctx.set_option(pkg.OPT_BINS_PER_THREAD, 8)
        ctx.set_spectrum(star.x, star.y)
        G, Gn = ctx.adjoint_table(star.model_id, P, star.plength)
        tabs, noise, nh, status = ctx.rgb_batch_tables(star.model_id, P, star.plength, idx, h)
        assert (status == 0).all()
        ctx.reset_kernel_stats()
        l0, g = ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T)
        assert ctx.rgb_adjoint_stats() == (2 * idx.size, 0)
    finally:
        ctx.close()
    nn = np.array([len(v) for v in noise])
    worst, seen, live, _ = _replay("red giant", G, Gn, tabs, noise, nn, g, P, idx, h, T, 1.0, E, 2)
    print("\nred giant: %d rows, worst |dS_dev - dS_exact| at %.3f of the rounding bound; fields contracted %s" % (tabs[0].size, worst, sorted(seen)))
    assert np.count_nonzero(live) >= 2 * (idx.size - 3) and len(seen) >= 3

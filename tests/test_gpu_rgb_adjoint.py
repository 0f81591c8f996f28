"""Adjoint gradient of the red-giant models (ids 25 / 27): the hybrid batch of csrc/fd_batch.hip under TAMCMC_OPT_GRADIENT =
TAMCMC_GRADIENT_ADJOINT with TAMCMC_OPT_RGB_ADJOINT = 1 -- the table-space adjoint (csrc/adjoint.hip) for the perturbed slots whose rows
correspond one to one with the base table's (csrc/adj_rgb_match.h), the windowed delta evaluation for the others.  FAST arithmetic, both
workgroup geometries.

The host cannot build a red-giant table, so the yardstick (tests/adjoint_numpy.py, tests/strict_numpy.py) works on the batch's own tables
as tamcmc_hip_rgb_batch_tables exports them; test 2 ties those to the oracle's model.  One star for the file, the one
tests/test_gpu_rgb_gradient.py builds: 4000 bins, 4 radial orders, period spacing 200 s, 25 mixed modes, 35 free parameters."""
import ctypes as C
import math

import numpy as np
import pytest

import adjoint_numpy as an
import strict_numpy
from test_gpu_rgb_gradient import _batch, _small_star, _steps

pytestmark = pytest.mark.gpu

GEOMS = [(64, 8), (256, 4)]           # workgroup, bins per thread
TOL_G = 1e-11                         # include/tamcmc_hip.h: each G / Gn entry within this of its absolute sum
TOL_LOGL = 1e-11                      # ... the FAST tolerance of a log-likelihood
LD = np.longdouble


@pytest.fixture(scope="module")
def small(synth, oracle):
    star, o = _small_star(synth)
    st, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    assert st == 0
    star.set_spectrum_from_model(m0, 4)
    return star, o


@pytest.fixture(scope="module")
def twin27(synth, oracle):
    star, o = _small_star(synth, cte=True)
    st, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    assert st == 0 and star.model_id == 27
    star.set_spectrum_from_model(m0, 4)
    return star, o


@pytest.fixture(scope="module")
def ctx(pkg, small):
    """FAST, timing on (the slot counters), both options set."""
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST, timing=True)
    c.set_spectrum(small[0].x, small[0].y)
    c.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT)
    c.set_option(pkg.OPT_RGB_ADJOINT, 1)
    yield c
    c.close()


def _geometry(pkg, c, geom, star=None):
    c.set_option(pkg.OPT_WORKGROUP, geom[0])
    c.set_option(pkg.OPT_BINS_PER_THREAD, geom[1])
    if star is not None:
        c.set_spectrum(star.x, star.y)


class _FdRoute:
    """The context on the finite-difference route (windowed unless windowed=0) for the length of a with block."""

    def __init__(self, pkg, c, windowed=1):
        self.pkg, self.c, self.windowed = pkg, c, windowed

    def __enter__(self):
        self.c.set_option(self.pkg.OPT_GRADIENT, self.pkg.GRADIENT_FD)
        self.c.set_option(self.pkg.OPT_FD_WINDOWED, self.windowed)

    def __exit__(self, *exc):
        self.c.set_option(self.pkg.OPT_GRADIENT, self.pkg.GRADIENT_ADJOINT)
        self.c.set_option(self.pkg.OPT_FD_WINDOWED, 1)


def _numpy_adjoint(tab, noise, nh, x, y):
    """adjoint_numpy.table_adjoint of an exported table: (G, Gabs, Gn, Gnabs)."""
    return an.table_adjoint(tab, noise, int(nh), x, y)


_REF = {}


def _reference(c, star, P, idx, h, key):
    """Exported tables of the batch (P, idx, h) and the numpy adjoint of each chain's base table, computed once per key."""
    if key not in _REF:
        tabs, noise, nh, status = c.rgb_batch_tables(star.model_id, P, star.plength, idx, h)
        assert (status == 0).all()
        E = idx.size + 1
        adj = [_numpy_adjoint(tabs[ch * E], noise[ch * E], nh[ch * E], star.x, star.y) for ch in range(np.atleast_2d(P).shape[0])]
        _REF[key] = (tabs, noise, nh, adj)
    return _REF[key]


def _contraction_and_bound(adj, tabs, noise, ch, E, k, T, happ, p=1.0):
    """Numpy gradient component k of chain ch from the exported tables, and the stated G tolerance carried through the contraction."""
    G, Ga, Gn, Gna = adj
    base, tab, n0, nz = tabs[ch * E], tabs[ch * E + 1 + k], noise[ch * E], noise[ch * E + 1 + k]
    assert tab.size == base.size
    want = float(-LD(p) * an.contract(G, Gn, base, n0, tab, nz) / LD(T) / LD(happ))
    s = LD(0)
    for j in range(base.size):
        nc = 2 * int(base["l"][j]) + 1
        s += np.sum((Ga[j, :nc] * np.abs(tab["nu"][j, :nc] - base["nu"][j, :nc])).astype(LD))
        s += np.sum((Ga[j, 7:7 + nc] * np.abs(tab["hv"][j, :nc] - base["hv"][j, :nc])).astype(LD))
        s += Ga[j, 14] * abs(tab["gamma"][j] - base["gamma"][j])
        if base["asym"][j] != 0.0:
            s += Ga[j, 15] * abs(tab["asym"][j] - base["asym"][j]) + Ga[j, 16] * abs(tab["fc"][j] - base["fc"][j])
    s += np.sum((Gna * np.abs(nz - n0)).astype(LD))
    return want, float((p / T) / abs(happ) * TOL_G * s)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_option_opens_the_red_giant_ids(pkg, small, twin27):
    """Fails without the feature: the option does not exist, set_option raises TAMCMC_ERR_BAD_ARG."""
    star, _ = small
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    try:
        c.set_option(pkg.OPT_RGB_ADJOINT, 1)
        with pytest.raises(pkg.TamcmcError) as e:
            c.set_option(pkg.OPT_RGB_ADJOINT, 2)
        assert e.value.code == pkg.ERR_BAD_ARG
        with pytest.raises(pkg.TamcmcError) as e:
            c.set_option(pkg.OPT_RGB_ADJOINT, -1)
        assert e.value.code == pkg.ERR_BAD_ARG
        c.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT)
        for s, _ in (small, twin27):
            c.set_spectrum(s.x, s.y)
            idx = s.index_to_relax
            h = _steps(s.params, idx)
            l0, g = c.fd_gradient(s.model_id, np.tile(s.params, (2, 1)), s.plength, idx, h, [1.0, 2.0])
            assert g.shape == (2, idx.size) and np.isfinite(l0).all() and np.isfinite(g).all() and np.count_nonzero(g) >= 2 * (idx.size - 3)
            l0p, pr0, gp = c.fd_gradient_posterior(s, s.params, h)
            assert np.isfinite(pr0).all() and np.isfinite(gp).all() and l0p[0] == l0[0]
            G, Gn = c.adjoint_table(s.model_id, s.params, s.plength)
            tabs, noise, nh, status = c.rgb_batch_tables(s.model_id, s.params, s.plength, idx, h)
            assert len(tabs) == idx.size + 1 and (status == 0).all() and G.shape[0] == 1 and G.shape[2] == 17
            assert G.shape[1] == s.plength[2] + s.plength[4] + s.plength[5] + 400 and tabs[0].size < G.shape[1] and np.count_nonzero(G) > 0
        with pytest.raises(pkg.TamcmcError) as e:          # a model that is no red giant has no such tables
            c.rgb_batch_tables(3, star.params, star.plength, star.index_to_relax, _steps(star.params, star.index_to_relax))
        assert e.value.code == pkg.ERR_BAD_MODEL
        c.set_option(pkg.OPT_PRECISION, pkg.PRECISION_STRICT)   # STRICT: TAMCMC_ERR_BAD_ARG, as for the other models
        with pytest.raises(pkg.TamcmcError) as e:
            c.fd_gradient(star.model_id, star.params, star.plength, star.index_to_relax, _steps(star.params, star.index_to_relax))
        assert e.value.code == pkg.ERR_BAD_ARG
        c.set_option(pkg.OPT_PRECISION, pkg.PRECISION_FAST)
        c.set_option(pkg.OPT_RGB_ADJOINT, 0)                     # back at 0: today's refusals
        c.set_spectrum(star.x, star.y)
        with pytest.raises(pkg.TamcmcError) as e:
            c.fd_gradient(star.model_id, star.params, star.plength, star.index_to_relax, _steps(star.params, star.index_to_relax))
        assert e.value.code == pkg.ERR_BAD_MODEL
        with pytest.raises(pkg.TamcmcError) as e:
            c.adjoint_table(star.model_id, star.params, star.plength)
        assert e.value.code == pkg.ERR_BAD_MODEL
        c.set_option(pkg.OPT_RGB_ADJOINT, 1)                     # the Fisher information keeps refusing the ids
        with pytest.raises(pkg.TamcmcError) as e:
            c.fisher(star.model_id, star.params, star.plength, star.index_to_relax, _steps(star.params, star.index_to_relax))
        assert e.value.code == pkg.ERR_BAD_MODEL
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- 2
def test_the_exported_tables_are_the_models(pkg, oracle, small, twin27, ctx):
    """strict_numpy.eval_table of the base slot's exported table against oracle.call_model, ||dM||_2 / ||M||_2 <= 1e-10 (the header's
    red-giant tolerance); the l=1 rows' frequencies are rgb_mixed_modes of the same vector to 1e-10 muHz."""
    for star, _ in (small, twin27):
        _geometry(pkg, ctx, GEOMS[0], star)
        idx = star.index_to_relax
        tabs, noise, nh, status = ctx.rgb_batch_tables(star.model_id, star.params, star.plength, idx[:2], _steps(star.params, idx[:2]))
        assert (status == 0).all() and len(tabs) == 3
        st, M = oracle.call_model(star.model_id, star.params, star.plength, star.x)
        assert st == 0
        got = strict_numpy.eval_table(tabs[0], noise[0], int(nh[0]), star.x)
        rel = np.linalg.norm(got - M) / np.linalg.norm(M)
        nu = ctx.rgb_mixed_modes(star.model_id, star.params, star.plength)[0]
        f1 = tabs[0]["fc"][tabs[0]["l"] == 1]
        print("\nid %d: exported base table against the oracle's model, ||dM|| / ||M|| = %.2e; %d mixed modes, max |d nu| %.2e muHz"
              % (star.model_id, rel, f1.size, np.max(np.abs(f1 - nu))))
        assert rel <= 1e-10
        assert f1.size == nu.size == 25 and np.all(np.abs(f1 - nu) <= 1e-10)
        assert list(tabs[0]["l"]) == sorted(tabs[0]["l"]) and np.all(np.diff(f1) > 0)       # l=0, the mixed modes in frequency order, l=2, l=3


# ---------------------------------------------------------------------------------------------------------------- 3
def _star_cases(small, twin27):
    star, _ = small
    idx = star.index_to_relax
    P2 = np.tile(star.params, (2, 1))
    P2[1, idx] *= 1 + 0.002 * np.random.default_rng(12).standard_normal(idx.size)
    return {"small": (star, np.atleast_2d(star.params)), "id27": (twin27[0], np.atleast_2d(twin27[0].params)), "two_chains": (star, P2)}


@pytest.mark.parametrize("name", ["small", "id27", "two_chains"])
def test_table_space_adjoint_field_by_field(pkg, small, twin27, ctx, name):
    """G and Gn of adjoint_table against adjoint_numpy.table_adjoint on the exported base table: each entry within 1e-11 of its absolute
    sum; entries of rows beyond the table's count exactly 0.  "two_chains": a chain perturbed by 0.2 % beside the star's own."""
    star, P = _star_cases(small, twin27)[name]
    none = np.zeros(0, dtype=np.int32)
    for geom in GEOMS:
        _geometry(pkg, ctx, geom, star)
        tabs, noise, nh, adj = _reference(ctx, star, P, none, np.zeros(0), ("fields", name))
        again = ctx.rgb_batch_tables(star.model_id, P, star.plength, none, np.zeros(0))
        assert all(np.array_equal(a, b) for a, b in zip(again[0], tabs))         # (the builder does not depend on the geometry)
        G, Gn = ctx.adjoint_table(star.model_id, P, star.plength)
        assert G.shape == (P.shape[0], star.plength[2] + star.plength[4] + star.plength[5] + 400, 17)
        for ch in range(P.shape[0]):
            Gw, Ga, Gnw, Gna = adj[ch]
            n = tabs[ch].size
            assert np.count_nonzero(Gw) >= 3 * n
            errG, errN = np.abs(G[ch, :n] - Gw), np.abs(Gn[ch, :Gnw.size] - Gnw)
            worst = max(np.max(errG / np.where(Ga > 0, Ga, 1.0)), np.max(errN / np.where(Gna > 0, Gna, 1.0)))
            print("\n%s %s chain %d: %d rows, worst field error %.2e of its absolute sum" % (name, geom, ch, n, worst))
            assert np.all(errG <= TOL_G * Ga), (geom, ch, np.argwhere(errG > TOL_G * Ga)[:4])
            assert np.all(errN <= TOL_G * Gna), (geom, ch)
            assert not G[ch, n:].any()
        G2, Gn2 = ctx.adjoint_table(star.model_id, P, star.plength)
        assert np.array_equal(G2, G) and np.array_equal(Gn2, Gn)
        if P.shape[0] == 2:                                 # alone = as row 1 of 2, and the two chains' tables do differ
            G1, Gn1 = ctx.adjoint_table(star.model_id, P[1], star.plength)
            assert np.array_equal(G1[0], G[1]) and np.array_equal(Gn1[0], Gn[1]) and not np.array_equal(G[0], G[1])


# ---------------------------------------------------------------------------------------------------------------- 4
def test_contraction_against_numpy_on_the_exported_tables(pkg, oracle, small, ctx):
    """The device gradient (no prior; T = 1 and T = 1.7, the second chain perturbed by 0.2 %) against adjoint_numpy.contract of the numpy
    G / Gn with the exported perturbed tables, per component within (p/T)/|h_applied| 1e-11 [sum A |dT| + sum An |d noise|].  logL0 is the
    windowed route's and the prior's share the finite-difference route's, bit for bit; two calls give the same bits; a chain's gradient
    is the same bits alone and in the batch; 35 linearised and 0 fallback slots per chain, which the oracle confirms for the star's own
    parameters (no step changes the mode set; the largest move of a mixed mode against the distance to its nearest neighbour)."""
    star, _ = small
    idx = star.index_to_relax
    h = _steps(star.params, idx)
    P = np.tile(star.params, (2, 1))
    P[1, idx] *= 1 + 0.002 * np.random.default_rng(12).standard_normal(idx.size)
    T = np.array([1.0, 1.7])
    E = idx.size + 1
    _, happ = _batch(P, idx, h)
    step = star.x[2] - star.x[1]
    V, _ = _batch(star.params, idx, h)
    rc, m0 = oracle.rgb_modes(V[0, 0], star.plength, step)
    assert rc == 0
    gap = np.minimum(np.diff(m0["fl1"], prepend=-np.inf), np.diff(m0["fl1"], append=np.inf))
    worst = 0.0
    for v in V[0, 1:]:
        rc, m = oracle.rgb_modes(v, star.plength, step)
        assert rc == 0 and m["fl1"].size == m0["fl1"].size == 25
        worst = max(worst, np.max(np.abs(m["fl1"] - m0["fl1"]) / np.abs(gap)))
    print("\noracle: no step changes the mode set; largest move of a mixed mode %.2e of the distance to its nearest neighbour" % worst)
    assert worst < 0.5
    for geom in GEOMS:
        _geometry(pkg, ctx, geom, star)
        tabs, noise, nh, adj = _reference(ctx, star, P, idx, h, "contraction")
        ctx.reset_kernel_stats()
        l0, g = ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T)
        assert ctx.rgb_adjoint_stats() == (2 * idx.size, 0)
        ratio = 0.0
        for ch in range(2):
            for k in range(idx.size):
                want, bound = _contraction_and_bound(adj[ch], tabs, noise, ch, E, k, T[ch], happ[ch, k])
                ratio = max(ratio, abs(g[ch, k] - want) / bound if bound > 0 else (0.0 if g[ch, k] == want else np.inf))
                assert abs(g[ch, k] - want) <= bound, (geom, ch, k, g[ch, k], want, bound)
        print("\n%s: device contraction against numpy on the exported tables, max |dgrad| / bound %.3e" % (geom, ratio))
        assert np.count_nonzero(g) >= 2 * (idx.size - 3)
        l0b, gb = ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T)
        assert np.array_equal(l0b, l0) and np.array_equal(gb, g)
        l01, g1 = ctx.fd_gradient(star.model_id, P[1], star.plength, idx, h, T[1:])
        assert l01[0] == l0[1] and np.array_equal(g1[0], g[1])
        l0p, pr0, gpost = ctx.fd_gradient_posterior(star, P, h, T)
        gprior = ctx.last_grad_prior.copy()
        assert np.array_equal(l0p, l0) and np.all(np.isfinite(gpost))
        with _FdRoute(pkg, ctx):
            l0w, pr0w, gw = ctx.fd_gradient_posterior(star, P, h, T)
            gprior_w = ctx.last_grad_prior.copy()
        assert np.array_equal(l0w, l0) and np.array_equal(pr0w, pr0) and np.array_equal(gprior_w, gprior)
        assert not np.array_equal(gw, gpost)               # (the two routes do differ: the option took effect)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_the_yardstick_against_the_frozen_central_difference(pkg, small, ctx):
    """No device likelihood, only exported tables.  The numpy adjoint gradient with the FORWARD table Jacobian must lie within 3 R + J of the
    frozen-window central difference: that difference from the exported tables at theta +- h with the base table's windows, rows by
    strict_numpy, sums in long double; R = max_k |g(h) - g(h/2)| its own uncertainty; J_k = |adjoint with the forward Jacobian - adjoint with
    the central Jacobian|, the curvature of the tables (a red giant's mixed-mode frequencies are curved in the period spacing, the
    coupling and the large separation) that the forward Jacobian carries and the reference does not."""
    star, _ = small
    _geometry(pkg, ctx, GEOMS[0], star)
    idx = star.index_to_relax
    h = _steps(star.params, idx)
    n = idx.size
    idx4, h4 = np.tile(idx, 4).astype(np.int32), np.concatenate([h, -h, 0.5 * h, -0.5 * h])
    tabs, noise, nh, status = ctx.rgb_batch_tables(star.model_id, star.params, star.plength, idx4, h4)
    assert (status == 0).all()
    base, nz0, nh0 = tabs[0], noise[0], int(nh[0])
    G, _, Gn, _ = _numpy_adjoint(base, nz0, nh0, star.x, star.y)
    V, happ4 = _batch(star.params, idx4, h4)
    happ4 = happ4[0]

    def S_frozen(slot):
        m = tabs[slot].copy()
        assert m.size == base.size
        m["i0"], m["i1"] = base["i0"], base["i1"]
        M = strict_numpy.eval_table(m, noise[slot], nh0, star.x)
        return np.sum((star.y / M).astype(LD)) + np.sum(np.log(M).astype(LD))

    def central(first):                                     # slots 1 + first + k (theta + s e_k) and 1 + first + n + k (theta - s e_k)
        g = np.zeros(n)
        for k in range(n):
            sp, sm = 1 + first + k, 1 + first + n + k
            g[k] = float(-(S_frozen(sp) - S_frozen(sm)) / (LD(happ4[sp - 1]) - LD(happ4[sm - 1])))
        return g

    g_ref, g_half = central(0), central(2 * n)
    R = float(np.max(np.abs(g_ref - g_half)))
    g_fwd, g_cen = np.zeros(n), np.zeros(n)
    for k in range(n):
        sp, sm = 1 + k, 1 + n + k
        g_fwd[k] = float(-an.contract(G, Gn, base, nz0, tabs[sp], noise[sp]) / LD(happ4[sp - 1]))
        g_cen[k] = float(-an.contract(G, Gn, tabs[sm], noise[sm], tabs[sp], noise[sp]) / (LD(happ4[sp - 1]) - LD(happ4[sm - 1])))
    J = np.abs(g_fwd - g_cen)
    d = np.abs(g_fwd - g_ref)
    scale = np.max(np.abs(g_ref))
    kJ = int(np.argmax(J))
    print("\nyardstick: gradient scale %.3e; R = %.3e (%.2e of scale); max J = %.3e (%.2e of scale, variable %d = parameter %d); "
          "max |adjoint(forward) - reference| = %.3e = %.2f of its 3R + J; max |adjoint(central) - reference| = %.2f R"
          % (scale, R, R / scale, J.max(), J.max() / scale, kJ, idx[kJ], d.max(), np.max(d / (3 * R + J)), np.max(np.abs(g_cen - g_ref)) / R))
    assert np.all(d <= 3 * R + J)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_fallback_slot_across_a_mode_count_change(pkg, oracle, small, ctx):
    """The point of tests/test_gpu_rgb_gradient.py::test_perturbation_that_changes_the_mode_count (period spacing 199.95987434979568 - 1e-5,
    h = 2e-5: the oracle gives 26 and 25 modes): one fallback slot.  Its component is the windowed route's bit for bit and meets that
    test's two bounds -- against brute force 5e-15 Nx / h + 1e-6 scale, against the oracle 2 1e-11 |logL| / h.  In the same batch a
    variable that moves every mixed mode without changing the set (the envelope rotation) and one that moves one row (an l=0 height)
    are contracted, within the bound of test 4."""
    star, o = small
    kdp = o[3] + 1
    p = star.params.copy()
    p[kdp] = 199.95987434979568 - 1e-5
    idx = np.array([kdp, o[6], 0], dtype=np.int32)
    h = np.concatenate([[2e-5], _steps(p, idx[1:])])
    V, happ = _batch(p, idx, h)
    step = star.x[2] - star.x[1]
    n_o = [len(oracle.rgb_modes(v, star.plength, step)[1]["fl1"]) for v in V[0]]
    assert n_o[0] != n_o[1] and n_o[2] == n_o[3] == n_o[0], n_o
    L, _, st = oracle.loglike_batch(star.model_id, V[0, :2], star.plength, star.x, star.y, 1.0, None)
    assert (st == 0).all()
    want_oracle = (L[1] - L[0]) / happ[0, 0]
    for geom in GEOMS:
        _geometry(pkg, ctx, geom, star)
        tabs, noise, nh, status = ctx.rgb_batch_tables(star.model_id, p, star.plength, idx, h)
        assert (status == 0).all() and [t.size - tabs[0].size for t in tabs] == [0, n_o[1] - n_o[0], 0, 0]
        ctx.reset_kernel_stats()
        l0, g = ctx.fd_gradient(star.model_id, p, star.plength, idx, h, [1.0])
        assert ctx.rgb_adjoint_stats() == (2, 1)
        with _FdRoute(pkg, ctx):
            l0w, gw = ctx.fd_gradient(star.model_id, p, star.plength, idx, h, [1.0])
        with _FdRoute(pkg, ctx, windowed=0):
            l0f, gf = ctx.fd_gradient(star.model_id, p, star.plength, idx, h, [1.0])
        scale = np.max(np.abs(gf))
        b_brute = 5e-15 * star.x.size / h[0] + 1e-6 * scale
        b_oracle = 2 * TOL_LOGL * abs(L[0]) / abs(happ[0, 0])
        print("\n%s: fallback component %.6e; |d| against brute force %.2e of its bound, against the oracle %.2e of its bound"
              % (geom, g[0, 0], abs(g[0, 0] - gf[0, 0]) / b_brute, abs(g[0, 0] - want_oracle) / b_oracle))
        assert l0[0] == l0w[0]
        assert g[0, 0] == gw[0, 0]                          # the windowed route's component, bit for bit
        assert abs(g[0, 0] - gf[0, 0]) <= b_brute and abs(g[0, 0] - want_oracle) <= b_oracle
        adj = _numpy_adjoint(tabs[0], noise[0], nh[0], star.x, star.y)
        for k in (1, 2):
            want, bound = _contraction_and_bound(adj, tabs, noise, 0, idx.size + 1, k, 1.0, happ[0, k])
            assert g[0, k] != 0.0 and abs(g[0, k] - want) <= bound, (geom, k, g[0, k], want, bound)
            assert g[0, k] != gw[0, k]                      # (contracted, not differenced)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_option_hygiene(pkg, oracle, synth, small, ctx):
    """With the new option on and TAMCMC_OPT_GRADIENT = FD the gradient has the bits of a context that never set it; ids 3 and 23 under the
    adjoint have the same bits with the option 0 and 1; a vector the pre-step refuses gives NaN in its component and the status, the other
    component unaffected (tests/test_gpu_rgb_gradient.py::test_failed_prestep_of_one_perturbed_vector)."""
    star, o = small
    idx = star.index_to_relax
    h = _steps(star.params, idx)
    fresh = pkg.HipContext(0, precision=pkg.PRECISION_FAST, workgroup=64, bins_per_thread=8)
    fresh.set_spectrum(star.x, star.y)
    want = fresh.fd_gradient_posterior(star, star.params, h, [1.3]) + (fresh.last_grad_prior.copy(),)
    fresh.close()
    _geometry(pkg, ctx, (64, 8), star)
    with _FdRoute(pkg, ctx):
        got = ctx.fd_gradient_posterior(star, star.params, h, [1.3]) + (ctx.last_grad_prior.copy(),)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    for ms in (synth.make_classic_star(nx=20000, nmax=6, step=0.05), synth.make_c3_star(nx=20000, step=0.1, nmax=8)):
        assert ms.model_id in (3, 23)
        y = an.spectrum(oracle, ms)
        c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
        try:
            c.set_spectrum(ms.x, y)
            c.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT)
            hm = an.steps(ms.params, ms.index_to_relax)
            res = []
            for flag in (0, 1):
                c.set_option(pkg.OPT_RGB_ADJOINT, flag)
                res.append(c.fd_gradient(ms.model_id, ms.params, ms.plength, ms.index_to_relax, hm, [1.3]) + c.adjoint_table(ms.model_id, ms.params, ms.plength))
            assert all(np.array_equal(a, b) for a, b in zip(*res)) and np.isfinite(res[0][1]).all()
        finally:
            c.close()
    bad = np.array([o[3] - 1, 0], dtype=np.int32)
    hb = np.array([-80.0, 1e-5])
    p = np.ascontiguousarray(star.params)
    pl = np.ascontiguousarray(star.plength, dtype=np.int32)
    l0, g = np.zeros(1), np.zeros((1, 2))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ctx.reset_kernel_stats()
    rc = pkg.lib().tamcmc_hip_fd_gradient(ctx._h, star.model_id, 1, p.ctypes.data_as(dp), p.size, pl.ctypes.data_as(ip), bad.ctypes.data_as(ip), 2,
                                          hb.ctypes.data_as(dp), None, 1.0, l0.ctypes.data_as(dp), g.ctypes.data_as(dp))
    assert rc == pkg.ERR_BAD_ARG and ctx.rgb_adjoint_stats() == (1, 0)      # (the failed slot is in neither count)
    _, g1 = ctx.fd_gradient(star.model_id, p, pl, bad[1:], hb[1:])
    assert np.isfinite(l0[0]) and np.isnan(g[0, 0]) and np.isfinite(g[0, 1]) and g[0, 1] == g1[0, 0]
    tabs, _, _, status = ctx.rgb_batch_tables(star.model_id, p, pl, bad, hb)
    assert list(status) == [0, pkg.ERR_BAD_ARG, 0] and tabs[1].size == 0 and tabs[2].size == tabs[0].size


# ---------------------------------------------------------------------------------------------------------------- 8
def test_host_engine_holds_the_hybrid_gradient(pkg, small, ctx):
    """tests/test_gpu_rgb_gradient.py::test_host_engine_langevin_sampler as it stands, on a context with both options: the gradient the
    engine holds equals the direct call's bits without swaps and lies within that test's re-tempering bound with swaps.  Then: the engine
    did take the hybrid route."""
    import test_gpu_rgb_gradient as rg
    star, _ = small
    _geometry(pkg, ctx, (256, 4), star)
    ctx.reset_kernel_stats()
    rg.test_host_engine_langevin_sampler(pkg, small, {"fast": ctx})
    lin, fall = ctx.rgb_adjoint_stats()
    print("\nhost engine: %d linearised and %d fallback slots" % (lin, fall))
    assert lin > 0
    s = pkg.Sampler(ctx, star, nchains=3, lambda_temp=1.6, use_drift=1, seed=5, engine="host", Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,),
                    dN_mixing=10**6)
    s.run(3)
    g, _, valid = s.gradient()
    held = np.tile(star.params, (3, 1))
    held[:, star.index_to_relax] = s.state()["vars"]
    hs = 1e-7 * np.maximum(np.abs(s.get_proposal(0)[0]), 1e-3)
    with _FdRoute(pkg, ctx):
        _, _, g_fd = ctx.fd_gradient_posterior(star, held, hs, np.array([math.pow(1.6, m) for m in range(3)]))
    v = np.flatnonzero(valid)
    assert v.size and not np.array_equal(g_fd[v], g[v])
    s.close()


def test_device_engine_follows_the_host_engine(pkg, small, ctx):
    """tests/test_gpu_rgb_device_langevin.py::test_one_iteration_at_a_time_against_the_host_engine as it stands (seed, widened Hfactor error,
    25 iterations, its bounds and its required events, proposals outside the prior's support among them), both engines on the hybrid route
    with TAMCMC_OPT_RGB_DEVICE_LANGEVIN = 1."""
    import test_gpu_rgb_device_langevin as dl
    star, _ = small
    _geometry(pkg, ctx, (64, 8), star)
    ctx.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 1)
    try:
        ctx.reset_kernel_stats()
        dl.test_one_iteration_at_a_time_against_the_host_engine(pkg, star, ctx)
        lin, fall = ctx.rgb_adjoint_stats()
        print("\nboth engines and the direct calls of the walk: %d linearised and %d fallback slots" % (lin, fall))
        assert lin > 0
        # the sampler continues across a change of route between two calls (tests/test_gpu_route_switch.py), and its held gradient is the
        # direct call's under the options of the moment
        d = pkg.Sampler(ctx, star, engine="device", **dl.KW)
        for hybrid in (True, False, True):
            ctx.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT if hybrid else pkg.GRADIENT_FD)
            _, stt = d.run(3, stats=True)
            g, gp, valid = d.gradient()
            g_direct, gp_direct, _ = dl._direct(ctx, star, d, d.state()["vars"])
            v = np.flatnonzero(valid)
            assert np.isfinite(stt).all() and v.size
            assert np.allclose(g[v], g_direct[v], rtol=1e-7, atol=1e-7 * np.abs(g_direct).max()), hybrid
        assert d.state()["iteration"] == 9
        d.close()
    finally:
        ctx.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT)
        ctx.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 0)


def test_a_geometry_without_the_delta_kernel_is_refused_and_leaves_nothing_behind(pkg, small, ctx):
    """The hybrid batch needs the DELTA variant of the likelihood kernel for its fallback slots (fd_batch.hip, layout): at 64 x 16, which
    has none, fd_gradient and fd_gradient_posterior return TAMCMC_ERR_BAD_ARG before anything is laid out.  The next calls at 64 x 8 give
    the bits of a context that never saw the refusal."""
    star, _ = small
    idx = star.index_to_relax
    h = _steps(star.params, idx)
    P = np.tile(star.params, (2, 1))
    P[1, idx] *= 1 + 0.002 * np.random.default_rng(12).standard_normal(idx.size)
    T = [1.0, 1.7]
    _geometry(pkg, ctx, (64, 16), star)
    try:
        with pytest.raises(pkg.TamcmcError) as e:
            ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T)
        assert e.value.code == pkg.ERR_BAD_ARG
        with pytest.raises(pkg.TamcmcError) as e:
            ctx.fd_gradient_posterior(star, P, h, T)
        assert e.value.code == pkg.ERR_BAD_ARG
    finally:
        _geometry(pkg, ctx, (64, 8), star)
    l0, g = ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T)
    l0p, pr0, gp = ctx.fd_gradient_posterior(star, P, h, T)
    fresh = pkg.HipContext(0, precision=pkg.PRECISION_FAST, timing=True)
    try:
        fresh.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT)
        fresh.set_option(pkg.OPT_RGB_ADJOINT, 1)
        _geometry(pkg, fresh, (64, 8), star)
        l0f, gf = fresh.fd_gradient(star.model_id, P, star.plength, idx, h, T)
        l0q, pr0q, gq = fresh.fd_gradient_posterior(star, P, h, T)
    finally:
        fresh.close()
    assert np.all(np.isfinite(g)) and np.count_nonzero(g) >= 2 * (idx.size - 3)
    for a, b in ((l0, l0f), (g, gf), (l0p, l0q), (pr0, pr0q), (gp, gq)):
        assert np.array_equal(a, b)

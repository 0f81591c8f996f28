"""Directed cases for the windowed finite-difference route against tests/delta_reference.py, as small as the paths allow.

A case is a star from tamcmc_c_amd.synth, a list of variables (parameter index, step, the path the variable is there for) and at most
three chains (T = 1, 1.3, 2.2; the other chains perturbed by 0.3 %).  Spectra are model x Exp(1) noise with a fixed seed, the model being
the longdouble twin's row of the host-built table at the star's own parameters (no oracle, no device).

Sizes.  An l = 0 window is 2 x 2.2 c = 220 muHz wide (set_imin_imax, c = 50, width <= 1 muHz) and must hold far tiles on both sides of its
near tiles at 512-bin tiles; the far gate rho <= 1/6 asks for about three tile widths of distance, so the window spans at least nine
tiles: 512 step <= 220 / 9, step <= 0.047 muHz.  Nx = 8192 + 307 = 8499 bins (no multiple of 256):
    ms      id 23, two radial orders x l <= 3 = 8 rows, 0.04 muHz from 1990 muHz (340 muHz): the second l = 0 window lies inside the grid;
    local   id 11, the C2 slice (6 rows, own height and width per mode, white noise only), 0.0317 muHz from 2900 muHz: the first l = 0 mode
            sits below the grid's first bin, its window is clamped at the lower edge; the second one's holds 13 tiles;
    wide    id 23, five radial orders (20 rows: a3 changes ten of them, twenty delta rows), 0.11 muHz from 1800 muHz, a1 = 3 muHz so that
            the l >= 2 windows reach the first tiles; at 256-bin tiles the first two lie in the far field of every row that covers them
            (rho <= 1/8 with the asymmetry on: eight half-widths of distance, which a 512-bin tile of 56 muHz does not have here).
Red giants (id 25): make_c5_star at nx = 4001, nmax = 4; its tables exist on the device only (rgb_batch_tables), so its classification
is checked by the GPU test.
    A second period-spacing step that changes the NUMBER of mixed modes: DP1 + 0.4 s (0.5 %) is in the case.  Found on the device
    (printed by the GPU test, recorded in DESIGN section 9): it takes chain 0 from 59 to 56 rows -- and the step of 1e-6 DP1 already
    changes the count (59 -> 58, 57 -> 58).  Full tables in FAST arithmetic, pairs with one-sided rows in FAST_DIRECT.
"""
from collections import namedtuple

import numpy as np

import delta_reference as dr

Case = namedtuple("Case", "name star idx h why P T y")
NX = 8192 + 307
T3 = np.array([1.0, 1.3, 2.2])


def _names(star, name):
    return [i for i, n in enumerate(star.names) if n == name]


def _small(star, idx):
    return 1e-6 * np.maximum(np.abs(star.params[np.asarray(idx)]), 1e-2)


def _chains(star, idx, n=3, seed=5):
    P = np.tile(star.params, (n, 1))
    u = np.unique(np.asarray(idx))
    P[1:, u] *= 1 + 0.003 * np.random.default_rng(seed).standard_normal((n - 1, u.size))
    return P


def host_table(pkg, star, params):
    st, rows, noise, nh = pkg.build_mode_table(star.model_id, params, star.plength, star.x)
    assert st == 0, st
    return dr.Table(rows, noise, nh, noise.size)


def spectrum(pkg, star, seed=1):
    t = host_table(pkg, star, star.params)
    m = dr.base_row(t, star.x).astype(np.float64)
    return m * np.random.default_rng(seed).exponential(1.0, m.size)


def host_tables(pkg, case):
    """The batch's tables in batch order, built on the host: slot c (Nvars + 1) + 1 + k is chain c with h[k] added to parameter idx[k]."""
    out = []
    for c in range(case.P.shape[0]):
        out.append(host_table(pkg, case.star, case.P[c]))
        for k, ip in enumerate(case.idx):
            p = case.P[c].copy()
            p[ip] = p[ip] + case.h[k]
            out.append(host_table(pkg, case.star, p))
    return out


def _ms(synth, asym):
    s = synth.make_c3_star(nx=NX, nmax=2, step=0.04, fmin=1990.0)
    o = s.plength[0] + s.plength[1] + s.plength[2:6].sum()
    s.params[o + 13] = asym
    return s, int(o)


def _case(pkg, name, star, vars_, chains=3, seed=5):
    idx = np.array([v[0] for v in vars_], dtype=np.int32)
    h = np.array([v[1] for v in vars_], dtype=np.float64)
    why = [v[2] for v in vars_]
    return Case(name, star, idx, h, why, _chains(star, idx, chains, seed), T3[:chains].copy(), spectrum(pkg, star))


def series(pkg, synth):
    """id 23, asymmetry on: heights, widths and one frequency of each degree at h = 1e-6 max(|theta|, 1e-2) and again at 1e-3 |theta|
    (frequencies: 1e-3 of the large separation's hundredth would still be a shift of many widths; they take 1e-6 |theta| x 30, a
    shift of 0.06 muHz), where |u| reaches 1e-3 .. 1e-2 and terms 3 to 5 of the series matter."""
    s, o = _ms(synth, 15.0)
    f = _names(s, "Frequency_l")
    ids = _names(s, "Height_l0") + _names(s, "Width_l0") + [f[0], f[2], f[4], f[6]]
    small = _small(s, ids)
    vars_ = [(i, hh, "series") for i, hh in zip(ids, small)]
    for i in ids:
        big = 3e-5 * abs(s.params[i]) if s.names[i] == "Frequency_l" else 1e-3 * abs(s.params[i])
        vars_.append((i, big, "series_high_order"))
    return _case(pkg, "series", s, vars_, seed=9)   # (a seed at which every far rule of the case keeps its 1e-3)


def closed_form(pkg, synth):
    """Height and width steps of 5 % on the strongest mode (|u| > 0.01 on its peak: the closed form), and a height step of 0.8 % that
    keeps max |u| between 0.005 and 0.01, just inside the series."""
    s, o = _ms(synth, 0.0)
    hs, ws = _names(s, "Height_l0"), _names(s, "Width_l0")
    k = int(np.argmax(s.params[hs]))
    vars_ = [(hs[k], 0.05 * s.params[hs[k]], "closed"), (ws[k], 0.05 * s.params[ws[k]], "closed"), (hs[k], 0.008 * s.params[hs[k]], "just_inside")]
    return _case(pkg, "closed_form", s, vars_)


def heights_only(pkg, synth):
    """Inclination and a visibility: many rows, each ONE row of height differences."""
    s, o = _ms(synth, 0.0)
    ids = _names(s, "Inclination") + _names(s, "Visibility_l1") + _names(s, "Visibility_l3")
    return _case(pkg, "heights_only", s, [(i, hh, "heights_only") for i, hh in zip(ids, _small(s, ids))])


def window_edge(pkg, synth):
    """Frequency steps of 1.25 bins on an l = 0 mode (seven rows follow it through the interpolated widths: a full table) and on an l = 1
    mode (a1 = 0.4 muHz here, so that its window of 2 x 100 muHz lies inside the grid: one pair, light), a width step of 3 % on the
    wider order (width > 1: the window grows with it): a row's i0 or i1 differs between the two tables."""
    s, o = _ms(synth, 0.0)
    s.params[o] = 0.4
    f, ws = _names(s, "Frequency_l"), _names(s, "Width_l0")
    k = int(np.argmax(s.params[ws]))
    vars_ = [(f[1], 0.05, "edge"), (f[2], 0.05, "edge"), (ws[k], 0.03 * s.params[ws[k]], "edge")]
    return _case(pkg, "window_edge", s, vars_)


def noise(pkg, synth):
    """Every parameter of the active Harvey term and the white level, beside a term with tau = 0 (chains 0 and 1; on chain 2 both terms
    are active).  The height and the exponent of the switched-off term are variables too: the noise row changes and the model does not."""
    s, o = _ms(synth, 0.0)
    n0 = int(s.plength[:8].sum())
    ids = [n0 + 3, n0 + 4, n0 + 5, n0 + 6, n0, n0 + 2]
    tau1 = s.params[n0 + 1]
    s.params[n0 + 1] = 0.0
    c = _case(pkg, "noise", s, [(i, hh, "noise") for i, hh in zip(ids, _small(s, ids))])
    c.P[2, n0 + 1] = tau1
    return c


def full_table(pkg, synth):
    """a1, a2 and the asymmetry move more rows than the table is long: full tables.  a3 moves the ten l >= 2 rows: twenty delta rows,
    pairs, not light -- its far-only tiles are delta_moment_shortcut's."""
    s = synth.make_c3_star(nx=NX, nmax=5, step=0.11, fmin=1800.0)
    o = int(s.plength[0] + s.plength[1] + s.plength[2:6].sum())
    s.params[o] = 3.0
    s.params[o + 1] = 0.02
    s.params[o + 13] = 12.0
    ids = [o, o + 2, o + 13, o + 4]
    why = ["full", "full", "full", "pairs_not_light"]
    return _case(pkg, "full_table", s, [(i, hh, w) for i, hh, w in zip(ids, _small(s, ids), why)])


def moments(pkg, synth):
    """The C2 slice: frequency (h = 1e-7 |theta|), height and width of the two l = 0 modes (one row each: light, k_fd_far takes their
    far-only tiles; the first mode's window is clamped at the spectrum's lower edge), and a height step of 3 % whose far tiles fail the
    moment gate and walk their bins."""
    s = synth.make_c2_star(nx=NX)
    ids = [6, 7, 0, 1, 19]
    small = _small(s, ids)
    small[:2] *= 0.1   # (frequencies: at 1e-6 |theta| the tiles next to the near field sit within a factor 2 of the moment gate)
    vars_ = [(i, hh, "light") for i, hh in zip(ids, small)]
    vars_.append((1, 0.03 * s.params[1], "gate_fails"))
    return _case(pkg, "moments", s, vars_)


MAKERS = {"series": series, "closed_form": closed_form, "heights_only": heights_only, "window_edge": window_edge, "noise": noise,
          "full_table": full_table, "moments": moments}
_CACHE = {}


def case(pkg, synth, name):
    if name not in _CACHE:
        _CACHE[name] = MAKERS[name](pkg, synth)
    return _CACHE[name]


def red_giant(synth):
    """id 25 at nx = 4001, nmax = 4: one l = 0 height, one parameter of the width law and the period spacing (every mixed mode moves), the
    latter also with a step of 0.5 % (see the module docstring).  One chain more at +0.3 %.  No spectrum here: the tables, and with them
    the model the spectrum is drawn from, exist on the device only."""
    s = synth.make_c5_star(nx=4001, nmax=4)
    hs, dp, al = _names(s, "Height_l0"), _names(s, "DP1")[0], _names(s, "alpha")[0]
    ids = [hs[1], al, dp]
    vars_ = [(i, hh, w) for i, hh, w in zip(ids, _small(s, ids), ["heights", "widths", "period_spacing"])]
    vars_.append((dp, 0.005 * s.params[dp], "mode_count"))
    idx = np.array([v[0] for v in vars_], dtype=np.int32)
    h = np.array([v[1] for v in vars_], dtype=np.float64)
    return Case("red_giant", s, idx, h, [v[2] for v in vars_], _chains(s, idx, 2, 6), T3[:2].copy(), None)


# ---------------------------------------------------------------- references, once per process ----------------------------------------------------------------
_REFS = {}


def references(key, case_, tables, y=None):
    """[[Reference per variable] per chain] of a case from its tables in batch order, computed once per process under `key`."""
    if key not in _REFS:
        E = case_.idx.size + 1
        y = case_.y if y is None else y
        out = []
        for c in range(case_.P.shape[0]):
            t0 = tables[c * E]
            M0 = dr.base_row(t0, case_.star.x)
            out.append([dr.slot_reference(t0, tables[c * E + 1 + k], case_.star.x, y, M0) for k in range(E - 1)])
        _REFS[key] = out
    return _REFS[key]

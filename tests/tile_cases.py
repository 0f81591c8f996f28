"""Directed inputs for the likelihood tile, each at an edge of one of its approximations (test_tile_reference.py checks the reference's
twin on them on the CPU, test_gpu_tile_reference.py runs them on the device).  A case is a regular grid, a batch of evaluations for
ONE launch of the table-level entry -- (rows, noise vector, nh, nn) each -- and what the far rule must say about its rows.

The geometry of a case follows the tile: cases(tile_bins) builds every case for tiles of that many bins, on x = 1000 + 0.05 i with two
full tiles and a ragged third of 3 bins; tile 1 is the tile under test (centre x_c, half-width h).  Heights and the white noise are
chosen so that the term under test is >= 0.9 of M there.  The background case has its own grid (x0 = 0, 62 tiles of 512 bins).
"""
import functools
import math

import numpy as np

import tile_reference as tr
import tile_series as ts

MULT_DTYPE = np.dtype([("l", "<i4"), ("i0", "<i4"), ("i1", "<i4"), ("flags", "<i4"), ("fc", "<f8"), ("gamma", "<f8"),
                       ("asym", "<f8"), ("nu", "<f8", (7,)), ("hv", "<f8", (7,))])
X0, STEP = 1000.0, 0.05
NOISE_STRIDE = 10


def row(l, i0, i1, gamma, nus, hvs, asym=0.0, fc=None):
    r = np.zeros(1, dtype=MULT_DTYPE)[0]
    r["l"], r["i0"], r["i1"], r["gamma"], r["asym"] = l, i0, i1, gamma, asym
    nus, hvs = list(nus), list(hvs)
    assert len(nus) == len(hvs) == 2 * l + 1
    r["nu"][:len(nus)] = nus
    r["hv"][:len(hvs)] = hvs
    r["fc"] = nus[l] if fc is None else fc
    return r


def table(rows):
    t = np.zeros(len(rows), dtype=MULT_DTYPE)
    for i, r in enumerate(rows):
        t[i] = r
    return t


class Case:
    def __init__(self, name, tile_bins, x0, step, nx):
        self.name, self.tile_bins, self.x0, self.step, self.nx = name, tile_bins, x0, step, nx
        self.x = x0 + step * np.arange(nx)
        self.evals = []        # (rows, noise, nh, nn)
        self.labels = []
        self.far_expect = []   # (evaluation, row, tile, far?)
        self.edge_tiles = []   # tiles whose every bin the CPU test takes to the 50-digit definition
        self.series_expect = []  # (evaluation, tile, series?)

    @property
    def ntiles(self):
        return (self.nx + self.tile_bins - 1) // self.tile_bins

    def geometry(self, tile):
        return tr.tile_geometry(tile, self.tile_bins, self.x0, self.step)

    def add(self, label, rows, noise=(1e-3,), nh=0, far=None):
        e = len(self.evals)
        noise = [float(v) for v in noise]
        assert len(noise) >= 3 * nh + 1 and len(noise) <= NOISE_STRIDE
        self.evals.append((table(rows), noise, nh, len(noise)))
        self.labels.append(label)
        for j, (tile, isfar) in (far or {}).items():
            self.far_expect.append((e, j, tile, isfar))
        return e

    # ---- what the entry point takes ----
    def launch_args(self):
        mults = np.concatenate([ev[0] for ev in self.evals]) if self.evals else np.zeros(0, dtype=MULT_DTYPE)
        offsets = np.cumsum([0] + [ev[0].size for ev in self.evals]).astype(np.int32)
        noise = np.zeros((len(self.evals), NOISE_STRIDE))
        for b, ev in enumerate(self.evals):
            noise[b, :ev[3]] = ev[1]
        return mults, offsets, noise, [ev[2] for ev in self.evals], [ev[3] for ev in self.evals]

    def temperatures(self):
        return 1.0 + 0.25 * (np.arange(len(self.evals)) % 5)


def _base(name, tb):
    return Case(name, tb, X0, STEP, 2 * tb + 3)


def _gate_row(c, A, q2, l=0, asym=0.0, side=1.0, i0=0, i1=None, hv_scale=1.0):
    """A row whose component nearest tile 1 has rho^2 = q2 and argument A there; the other 2l components lie 8 muHz apart, further out."""
    xc, h = c.geometry(1)
    beta = math.sqrt(q2 * (A * A + 1.0))
    gamma = 2.0 * h / beta
    nu0 = xc + side * A * gamma / 2.0
    nus = [nu0 + side * 8.0 * k for k in range(2 * l + 1)]
    if side < 0:
        nus = nus[::-1]
    hv = hv_scale * (A * A + 1.0)
    return row(l, i0, c.nx if i1 is None else i1, gamma, nus, [hv] * (2 * l + 1), asym)


def far_gate(tb):
    """1. One component 1e-3 inside / outside the far gate on tile 1, for l = 0 and for l = 3 (one component of seven at the gate), without
    and with asymmetry (its gate: 1/64), at A = 0, 1, 10, 1e3; a window one bin short of the tile."""
    c = _base("far_gate", tb)
    for l in (0, 3):
        for asym in (0.0, 30.0, -30.0):
            r2 = ts.RHO_MAX2_ASYM if asym else ts.RHO_MAX2
            for A in (0.0, 1.0, 10.0, 1e3):
                for isfar in (True, False):
                    q2 = r2 * (1.0 - 1e-3 if isfar else 1.0 + 1e-3)
                    c.add("l%d asym%+g A%g %s" % (l, asym, A, "far" if isfar else "near"), [_gate_row(c, A, q2, l, asym)], far={0: (1, isfar)})
    c.add("window one bin short", [_gate_row(c, 10.0, ts.RHO_MAX2 * 0.5, i1=2 * tb - 1)], far={0: (1, False)})
    c.add("same, full window", [_gate_row(c, 10.0, ts.RHO_MAX2 * 0.5)], far={0: (1, True)})
    c.edge_tiles = [2]
    return c


def early_stop(tb):
    """2. Every far component of tile 1 just below one threshold of the coefficient loop's early stop (the wave-uniform break is taken);
    one component above the first threshold among many below it (it is not); and components just under the top of each band."""
    c = _base("early_stop", tb)
    As = (0.0, 1.0, 10.0, 100.0, 1e3)
    for thr, n in ts.EARLY_STOP:
        rows = [_gate_row(c, A, thr * (1.0 - 1e-3), side=(1.0 if i % 2 else -1.0), hv_scale=0.2) for i, A in enumerate(As)]
        c.add("all below %g" % thr, rows, far={j: (1, True) for j in range(len(rows))})
    thr = ts.EARLY_STOP[0][0]
    rows = [_gate_row(c, A, thr * (1.0 - 1e-3), side=-1.0, hv_scale=0.15) for A in As] + [_gate_row(c, 10.0, thr * (1.0 + 1e-3), hv_scale=0.15)]
    c.add("one above %g" % thr, rows, far={j: (1, True) for j in range(len(rows))})
    tops = [ts.RHO_MAX2] + [t for t, _ in ts.EARLY_STOP]
    for top in tops:
        c.add("band top %g" % top, [_gate_row(c, 100.0, 0.9 * top)], far={0: (1, True)})
        c.add("band top %g, l = 2" % top, [_gate_row(c, 30.0, 0.9 * top, l=2)], far={0: (1, True)})
    c.edge_tiles = [2]
    return c


def wing(tb):
    """3. Tile 1 in the wing of one tall, broad mode (an F star: Gamma = 6 muHz) as close as the gate lets it be far, little background:
    the far term is >= 0.99 of M."""
    c = _base("wing", tb)
    xc, h = c.geometry(1)
    for gamma in (6.0, 3.0):
        beta = 2.0 * h / gamma
        for l in (0, 1):
            nu0 = xc + 0.5 * gamma * math.sqrt(36.0 * beta * beta - 1.0) * 1.0005
            nus = [nu0 + 1.0 * k for k in range(2 * l + 1)]
            c.add("Gamma %g l%d" % (gamma, l), [row(l, 0, c.nx, gamma, nus, [1e4] * (2 * l + 1))], far={0: (1, True)})
    c.edge_tiles = [2]
    return c


def narrow(tb):
    """5. Narrow modes (gamma = 0.01 -- the narrowest mixed mode the header names -- and 0.1 muHz) centred on a bin, half a bin off, at the
    tile's last bin, and in the next tile with a window crossing the boundary."""
    c = _base("narrow", tb)
    x = c.x
    for gamma in (0.01, 0.1):
        for l in (0, 1):
            def m(nu0, i0, i1):
                nus = [nu0 + 0.3 * (k - l) for k in range(2 * l + 1)]
                return row(l, i0, i1, gamma, nus, [100.0 / (1 + abs(k - l)) for k in range(2 * l + 1)])
            rows = [m(x[tb + 100], tb + 60, tb + 140), m(x[tb + 180] + 0.5 * STEP, tb + 150, tb + 215),
                    m(x[2 * tb - 1], 2 * tb - 40, 2 * tb + 3), m(x[2 * tb + 1], 2 * tb - 30, c.nx)]
            c.add("gamma %g l%d" % (gamma, l), rows, noise=(1.0,))
            c.add("gamma %g l%d, first tile" % (gamma, l), [m(x[tb - 1], tb - 35, tb + 20), m(x[3] + 0.5 * STEP, 0, 40)], noise=(1.0,))
    c.edge_tiles = [1, 2]
    return c


def common_denominator(tb):
    """6. The common-denominator sum of fast_mult: heights over twelve decades, heights exactly 0, coincident components, and widths so
    small that the product of the denominators would overflow (F_SAFE is not set: the plain-sum branch)."""
    c = _base("common_denominator", tb)
    x = c.x
    ctr = x[tb + tb // 2]
    spl = [ctr + 0.4 * (k - 3) for k in range(7)]
    rows = [
        row(3, tb + 5, 2 * tb - 7, 1.0, spl, [1e-8, 1e-6, 1e-4, 1e-2, 1.0, 1e2, 1e4]),
        row(3, tb + 5, 2 * tb - 7, 1.0, spl, [0.0, 3.0, 0.0, 5.0, 1.0, 2.0, 4.0]),
        row(3, tb + 5, 2 * tb - 7, 1.0, [ctr + 0.01] * 7, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]),
        row(3, tb + 5, 2 * tb - 7, 0.7, spl, [4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], asym=12.0),
    ]
    for j, r in enumerate(rows):
        c.add("row %d" % j, [r], noise=(3.0,))
    c.add("all four", rows, noise=(3.0,))
    off = x[tb + 50] + 0.25 * STEP   # a quarter of a bin off every bin: the components are ~1e-40 everywhere, the row adds nothing
    for gamma in (1e-19, 1e-25):
        tiny = row(3, tb + 10, tb + 90, gamma, [off + 0.4 * k for k in range(7)], [1.0] * 7)
        c.add("gamma %g alone" % gamma, [tiny], noise=(1.0,))
        c.add("gamma %g beside a mode" % gamma, [rows[1], tiny, row(1, 0, c.nx, gamma, [off, off + 1.0, off + 2.0], [2.0, 3.0, 2.0])], noise=(1.0,))
    c.edge_tiles = [1, 2]
    return c


def windows(tb):
    """7. Windows one bin wide, ending exactly at a tile boundary, starting at the last bin (of a tile, of the grid); an evaluation with
    no rows; and 70 rows on one tile -- a second staging chunk -- with far and near rows alternating in table order."""
    c = _base("windows", tb)
    x, nx = c.x, c.nx

    def m(i_nu, i0, i1, l=1, gamma=0.5):
        return row(l, i0, i1, gamma, [x[i_nu] + 0.2 * (k - l) for k in range(2 * l + 1)], [50.0] * (2 * l + 1))
    c.add("one bin", [m(tb + 7, tb + 7, tb + 8)], noise=(0.5,))
    c.add("ends at a tile boundary", [m(tb - 5, tb - 30, tb), m(2 * tb - 3, tb + 1, 2 * tb)], noise=(0.5,))
    c.add("starts at the last bin", [m(nx - 1, nx - 1, nx), m(2 * tb - 1, 2 * tb - 1, 2 * tb + 2), m(tb - 1, tb - 1, tb)], noise=(0.5,))
    c.add("no rows", [], noise=(0.5,))
    c.add("no rows, a Harvey term", [], noise=(3.0, 1.2, 2.0, 0.5), nh=1)
    xc, h = c.geometry(1)
    rows, far = [], {}
    for j in range(70):
        if j % 2 == 0:
            g = h / 12.0
            l = (j // 2) % 4
            nu0 = xc + (10.0 + 0.1 * j) * h
            A = 2.0 * (nu0 - xc) / g
            rows.append(row(l, 0, nx, g, [nu0 + 0.3 * k for k in range(2 * l + 1)], [0.05 * A * A] * (2 * l + 1)))
            far[j] = (1, True)
        else:
            i_nu = tb + (j * tb) // 80
            rows.append(m(i_nu, max(i_nu - 30, 0), min(i_nu + 31, nx), l=j % 4, gamma=0.3))
            far[j] = (1, False)
    c.add("70 rows, far and near interleaved", rows, noise=(0.5,), far=far)
    c.add("the same, far rows last", rows[1::2] + rows[0::2], noise=(0.5,))
    c.edge_tiles = [1, 2]
    return c


BG_TILE_BINS = 512
BG_NTILES = 62
BG_P = (1.0, 2.0, 3.5, 4.0, 6.0, 8.0)
BG_AXC = (1.0, 5.0, 50.0)


def background(tb=BG_TILE_BINS):
    """4. The background series.  x0 = 0 and tiles of 512 bins: eps = h / x_c = 256 / (512 t + 255.5) on tile t whatever the step, so the
    tiles run through eps = 0.02 (between tiles 24 and 25) and through the gate of every exponent (p = 2: tile 25 .. p = 8: tile 58).
    One term per evaluation for p x (a x_c at the gate tile), Harvey-dominated (the term is ~1 at its gate, white noise 1e-2); two and
    three terms of different exponents; a term with tau = 0.  The first tile has x_c > 0 and h / x_c ~ 1, and its first bin is x = 0."""
    assert tb == BG_TILE_BINS
    c = Case("background", tb, 0.0, STEP, BG_NTILES * tb + 3)

    def gate_tile(p):
        e = ts.eps_at_gate(p)
        return next(t for t in range(c.ntiles) if 256.0 / (512.0 * t + 255.5) <= e)

    def term(p, axc):
        xc, _ = c.geometry(gate_tile(p))
        return [1.0 + axc ** p, axc / (1e-3 * xc), p]

    def add(label, terms):
        noise = [v for t in terms for v in t] + [1e-2]
        e = c.add(label, [], noise=noise, nh=len(terms))
        for t in range(c.ntiles):
            xc, h = c.geometry(t)
            c.series_expect.append((e, t, tr.series_gate(noise, len(terms), xc, h)))
        return e
    for p in BG_P:
        for axc in BG_AXC:
            add("p %g, a x_c %g" % (p, axc), [term(p, axc)])
        c.edge_tiles += [gate_tile(p) - 1, gate_tile(p)]
    add("two terms", [term(2.0, 5.0), term(4.0, 1.0)])
    add("three terms", [term(1.0, 1.0), term(3.5, 5.0), term(8.0, 5.0)])
    add("tau = 0 beside a steep term", [[5.0, 0.0, 8.0], term(2.0, 5.0)])
    add("tau = 0 alone", [[5.0, 0.0, 4.0]])
    c.edge_tiles = sorted(set(c.edge_tiles + [0, 24, 25, c.ntiles - 1]))
    return c


BUILDERS = (far_gate, early_stop, wing, narrow, common_denominator, windows)


@functools.lru_cache(maxsize=None)
def cases(tile_bins):
    out = [b(tile_bins) for b in BUILDERS]
    if tile_bins == BG_TILE_BINS:
        out.append(background())
    return out


class Reference:
    """The twin's answers for one case, computed once: model rows, the far sums, y (drawn around evaluation 0's row) and logL."""

    def __init__(self, case, seed=5):
        c = self.case = case
        self.M = [tr.model_row_ld(ev[0], ev[1], ev[2], ev[3], c.x) for ev in c.evals]
        FF = [tr.far_abs_sum(ev[0], c.x, c.tile_bins, c.x0, c.step) if ev[0].size else (np.zeros(c.nx, tr.LD),) * 2 for ev in c.evals]
        self.F = [f[0] for f in FF]
        self.Fa = [f[1] for f in FF]
        pick = max(range(len(c.evals)), key=lambda b: c.evals[b][0].size)   # the spectrum is drawn around the busiest evaluation
        self.y = (self.M[pick] * np.random.default_rng(seed).exponential(1.0, c.nx)).astype(np.float64)
        self.T = c.temperatures()
        self.logL = {p: [tr.loglike_ld(self.M[b], self.y, self.T[b], p) for b in range(len(c.evals))] for p in (1, 2)}


@functools.lru_cache(maxsize=None)
def reference(tile_bins, name):
    return Reference(next(c for c in cases(tile_bins) if c.name == name))

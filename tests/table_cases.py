"""Parameter vectors for the table parity tests (tests/table_reference.py), small enough that every GPU test takes seconds.

A GROUP is one layout (model id, plength) on one grid with several parameter vectors: the shape of a device batch (a gradient batch, the
chains of a sampler).  Directed groups place one property per vector; random groups add vectors drawn per id and lmax.  The reference
table of every vector is computed once (`reference`, `twin`) and shared by the CPU and the GPU modules.

Grids have 3 to 4097 bins and at most 17 radial orders.  Directed grids have a dyadic step and start, so that the decisions the cases
place ON a decision point (the `>=` of the upper clip rule) are exact in double as in the reference: those edges are listed in
`Group.exact_edges` and are not knife edges (nothing is rounded on the way to them).
"""
import math

import numpy as np

import table_reference as tr

AJ, CLASSIC, LOCAL, V2, V3, HNLM = tr.AJ, tr.CLASSIC, tr.LOCAL, tr.V2, tr.V3, tr.HNLM
IDS = tr.IDS
GLOBAL = (AJ, CLASSIC, V2, V3)
DEG = 180.0 / math.pi
INCLINATIONS = [0.0, 1e-8, 30.0, 90.0 - 1e-8, 90.0, math.acos(math.sqrt(1.0 / 3.0)) * DEG, math.acos(math.sqrt(3.0 / 5.0)) * DEG,
                math.acos(math.sqrt(1.0 / 5.0)) * DEG]   # the last three: zeros of l = 2 m = 0, l = 3 m = 0, l = 3 |m| = 1


class Group:
    def __init__(self, name, model_id, plength, x, directed):
        self.name, self.model_id, self.plength, self.x, self.directed = name, model_id, np.asarray(plength, dtype=np.int32), x, directed
        self.names, self.vectors, self.exact_edges = [], [], set()
        self.grid = tr.Grid(x)
        self._ref, self._twin = {}, {}

    def add(self, vname, p):
        assert p.size == int(self.plength.sum()), (vname, p.size, self.plength)
        self.names.append(vname)
        self.vectors.append(np.array(p, dtype=np.float64))
        return len(self.vectors) - 1

    @property
    def params(self):
        return np.stack(self.vectors)

    @property
    def per(self):
        return tr.count_rows(self.model_id, self.plength)

    def reference(self, i):
        if i not in self._ref:
            self._ref[i] = tr.build(self.model_id, self.vectors[i], self.plength, self.grid)
        return self._ref[i]

    def twin(self, i):
        if i not in self._twin:
            self._twin[i] = tr.build(self.model_id, self.vectors[i], self.plength, self.grid, twin=True)
        return self._twin[i]

    def __repr__(self):
        return self.name


def dyadic_grid(nx, x0, step):
    return x0 + step * np.arange(nx, dtype=np.float64)


class Maker:
    """One layout; `vector(**knobs)` fills it.  Offsets as the model functions decode them (models.cpp:1207-1219)."""

    def __init__(self, model_id, lmax, nfl0, nnoise=7, f0=40.0, dnu=8.0):
        self.id, self.lmax, self.n, self.nnoise, self.f0, self.dnu = model_id, lmax, nfl0, nnoise, f0, dnu
        self.nfl = [nfl0] + [nfl0 if l <= lmax else 0 for l in (1, 2, 3)]
        nf = sum(self.nfl)
        if model_id in GLOBAL:
            self.nmax, self.nvis, self.nwidth = nfl0, lmax, nfl0
        elif model_id == LOCAL:
            self.nmax, self.nvis, self.nwidth = nf, 0, nf
        else:
            self.nmax, self.nvis, self.nwidth = sum((l + 1) * self.nfl[l] for l in range(4)), 0, nf
        self.nsplit = 14 if model_id == AJ else 6
        self.ninc = {AJ: 1, CLASSIC: 1, LOCAL: 1, HNLM: 1, V2: 9, V3: max(1, (min(lmax, 3) + 1) * nfl0)}[model_id]
        self.plength = np.array([self.nmax, self.nvis] + self.nfl + [self.nsplit, self.nwidth, nnoise, self.ninc, 2], dtype=np.int32)
        self.o_vis = self.nmax
        self.o_f = [self.nmax + self.nvis + sum(self.nfl[:l]) for l in range(4)]
        self.o_split = self.nmax + self.nvis + nf
        self.o_width = self.o_split + self.nsplit
        self.o_noise = self.o_width + self.nwidth
        self.o_inc = self.o_noise + nnoise
        self.o_cfg = self.o_inc + self.ninc
        self.size = self.o_cfg + 2

    def span(self):
        return self.f0 - self.dnu, self.f0 + self.dnu * (self.n + 1)

    def vector(self, rng, inc=40.0, do_amp=0, trunc_c=2.5, a1=0.8, a3=0.02, asym=5.0, eta=1.0, wlo=0.4, whi=2.5, neg=False, slopes=True):
        p = np.zeros(self.size)
        n, dnu, f0 = self.n, self.dnu, self.f0
        p[:self.nmax] = rng.uniform(1.0, 10.0, self.nmax)
        if self.nvis:
            p[self.o_vis:self.o_vis + self.nvis] = [1.5, 0.5, 0.08][:self.nvis]
        # l = 0 knots; l = 1 inside segment n (the last one above the top knot); l = 2 just below its knot (the first one below the
        # bottom knot); l = 3 inside segment n again
        p[self.o_f[0]:self.o_f[0] + n] = f0 + dnu * np.arange(n) + rng.uniform(-0.2, 0.2, n)
        for l, shift in ((1, 0.5), (2, -0.12), (3, 0.3)):
            if self.nfl[l]:
                p[self.o_f[l]:self.o_f[l] + n] = f0 + dnu * (np.arange(n) + shift) + rng.uniform(-0.2, 0.2, n)
        sp = self.o_split
        if self.id == AJ:
            consts = [a1, 0.05, a3, 0.004, 0.002, 0.001]
            for j in range(6):
                p[sp + 2 * j] = consts[j] * (1.0 if j in (0, 2) else rng.uniform(0.5, 1.5))
                p[sp + 2 * j + 1] = rng.uniform(-0.3, 0.3) * consts[j] if slopes else 0.0
            p[sp + 12], p[sp + 13] = eta, asym
        elif self.id == LOCAL:
            r = math.sqrt(a1)
            p[sp:sp + 6] = [0.0, 5e7 * eta, a3, r * math.cos(inc / DEG), r * math.sin(inc / DEG), asym]
        elif self.id == HNLM:
            p[sp:sp + 6] = [a1, 5e7 * eta, a3, 0.0, 0.0, asym]
        else:
            p[sp:sp + 6] = [a1, 0.0, a3, 0.0, 0.0, asym]
        p[self.o_width:self.o_width + self.nwidth] = rng.uniform(wlo, whi, self.nwidth)
        p[self.o_noise:self.o_noise + self.nnoise] = rng.uniform(0.5, 2.0, self.nnoise)
        if self.id in (AJ, CLASSIC):
            p[self.o_inc] = inc
        elif self.id in (V2, V3):
            p[self.o_inc:self.o_inc + self.ninc] = rng.uniform(0.1, 0.6, self.ninc)
        p[self.o_cfg], p[self.o_cfg + 1] = trunc_c, do_amp
        if neg:  # the builders take |.| of heights, visibilities, widths, noise, ratios, a1 (ids 3, 12..14)
            for lo, cnt in ((0, self.nmax), (self.o_vis, self.nvis), (self.o_width, self.nwidth), (self.o_noise, self.nnoise)):
                p[lo:lo + cnt:2] *= -1.0
            if self.id in (V2, V3):
                p[self.o_inc:self.o_inc + self.ninc:3] *= -1.0
            if self.id in (CLASSIC, V2, V3, HNLM):
                p[sp] *= -1.0
        return p

    def set_local_inc(self, p, a1, p3=None, p4=None, inc=None):
        if inc is not None:
            p3, p4 = math.sqrt(a1) * math.cos(inc / DEG), math.sqrt(a1) * math.sin(inc / DEG)
        p[self.o_split + 3], p[self.o_split + 4] = p3, p4


def _l0_half_width(mk, p, n):
    """Half width of the window of the l = 0 mode n as a double (c 2.2 max(|W|, 1)): directed edges are placed 1e-6 of a bin from an
    integer, ten orders of magnitude above what this double's rounding moves them."""
    w = abs(p[mk.o_width + n])
    return p[mk.o_cfg] * 2.2 * max(w, 1.0)


def directed_groups(model_id):
    """The directed cases of one model id."""
    rng = np.random.default_rng(1000 + model_id)
    out = []
    step = 0.0625
    # ---- one group per (lmax, Nfl0): the register scan's sizes (2, 3, 16 | 17), every degree count
    for lmax, nfl0, nnoise in ((0, 2, 1), (1, 3, 4), (2, 16, 7), (3, 17, 10), (3, 16, 7)):
        mk = Maker(model_id, lmax, nfl0, nnoise=nnoise)
        lo, hi = mk.span()
        nx = min(4097, int((hi - lo) / step) + 1)
        g = Group(f"id{model_id}-lmax{lmax}-n{nfl0}", model_id, mk.plength, dyadic_grid(nx, lo, step), True)
        g.add("plain", mk.vector(rng))
        g.add("amp", mk.vector(rng, do_amp=1))
        g.add("negative", mk.vector(rng, neg=True))
        g.add("negative-amp", mk.vector(rng, neg=True, do_amp=1, asym=-30.0))
        p = mk.vector(rng)
        p[0] = 0.0                                                  # a zero height
        g.add("zero-height", p)
        for tag, a1 in (("below", 0.4), ("at", 1.0), ("above", 2.75)):
            g.add(f"a1-{tag}-1", mk.vector(rng, a1=a1, a3=-0.03, slopes=False))
        if model_id == AJ:
            # a1(nu) = a1_0 + a1_1 nu[mHz] crossing 1 inside the table: slope 10 per mHz = 0.08 per order
            p = mk.vector(rng, a1=1.0 - 10.0 * (mk.f0 + mk.dnu * 1.5) * 1e-3)
            p[mk.o_split + 1] = 10.0
            g.add("a1-slope-through-1", p)
            g.add("eta-off", mk.vector(rng, eta=0.0, asym=0.0))
        g.add("widths-below-1", mk.vector(rng, wlo=0.2, whi=0.9))
        p = mk.vector(rng, wlo=1.0, whi=1.0)
        g.add("widths-at-1", p)
        g.add("widths-above-1", mk.vector(rng, wlo=1.5, whi=4.0))
        g.add("trunc-small", mk.vector(rng, trunc_c=0.03))
        g.add("trunc-large", mk.vector(rng, trunc_c=200.0))
        if model_id in (AJ, CLASSIC):
            for inc in INCLINATIONS:
                g.add(f"inc-{inc!r}", mk.vector(rng, inc=inc, do_amp=int(inc == 30.0)))
        if model_id == LOCAL:
            for inc in INCLINATIONS:
                g.add(f"inc-{inc!r}", mk.vector(rng, inc=inc, a1=0.9))
            for tag, p3, p4 in (("p3-zero", 0.0, 0.8), ("p4-zero", 0.9, 0.0), ("p3-negative", -0.6, 0.7), ("p4-negative", 0.6, -0.7),
                                ("both-negative", -0.5, -0.4), ("a1-above-1", 1.2, 0.9), ("a1-exactly-1", 1.0, 0.0)):
                p = mk.vector(rng)
                mk.set_local_inc(p, None, p3=p3, p4=p4)
                g.add(tag, p)
        if lmax >= 2 and nfl0 >= 3:
            p = mk.vector(rng)
            p[mk.o_f[2] + 1] = p[mk.o_f[0] + 1]                       # an l = 2 frequency exactly on a knot
            p[mk.o_f[1] + 0] = p[mk.o_f[0] + nfl0 - 1]                # and an l = 1 frequency on the last one
            g.add("on-knots", p)
        # ---- a failing vector between two good ones
        g.add("good-before", mk.vector(rng))
        p = mk.vector(rng)
        p[mk.o_width + (1 if nfl0 > 1 else 0)] = float("nan")
        g.add("nan-width", p)
        g.add("good-between", mk.vector(rng, do_amp=1))
        g.add("empty-window", mk.vector(rng, trunc_c=-0.5))           # lo > hi: no bin whatever the rounding
        g.add("good-after", mk.vector(rng))
        # ---- directed window edges: the l = 0 mode `n` 1e-6 of a bin either side of an integer quotient
        nmid = nfl0 // 2
        for edge in ("i0", "i1"):
            for tag, delta in (("below", -1e-6), ("above", 1e-6)):
                p = mk.vector(rng, trunc_c=1.0)
                h = _l0_half_width(mk, p, nmid)
                k = round((p[mk.o_f[0] + nmid] - g.grid.x_first) / step)
                target = g.grid.x_first + step * (k + delta)
                p[mk.o_f[0] + nmid] = target + h if edge == "i0" else target - h
                g.add(f"edge-{edge}-{tag}", p)
        out.append(g)
    # ---- window placements on grids of their own (lmax 2, three orders)
    mk = Maker(model_id, 2, 3, nnoise=4, f0=64.0, dnu=8.0)
    for tag, x0, nx in (("grid-above-modes", 75.0, 257), ("grid-below-modes", 30.0, 600), ("x-first-0", 0.0, 1200), ("three-bins", 71.5, 3),
                        ("4097-bins", 0.0, 4097)):
        st = 0.03125 if tag == "4097-bins" else step
        g = Group(f"id{model_id}-{tag}", model_id, mk.plength, dyadic_grid(nx, x0, st), True)
        for c in (0.51, 4.03, 30.02):       # (not a multiple of the step: a clipped edge x_first + c is no integer quotient)
            g.add(f"c-{c}", mk.vector(rng, trunc_c=c))
            g.add(f"c-{c}-wide", mk.vector(rng, trunc_c=c, wlo=1.5, whi=3.0, a1=2.5))
        out.append(g)
    # ---- one-bin windows: every window narrower than a bin, modes half-way between bins
    mk = Maker(model_id, 1, 3, nnoise=1, f0=64.0, dnu=8.0)
    g = Group(f"id{model_id}-one-bin", model_id, mk.plength, dyadic_grid(513, 56.0, step), True)
    p = mk.vector(rng, trunc_c=0.004, wlo=0.3, whi=0.9, a1=0.5, a3=0.0)
    for l in range(2):
        f = p[mk.o_f[l]:mk.o_f[l] + 3]
        p[mk.o_f[l]:mk.o_f[l] + 3] = g.grid.x_first + step * (np.round((f - g.grid.x_first) / step) + 0.5)
    g.add("half-way", p)
    out.append(g)
    # ---- lo + step == x_last exactly: l = 1, width < 1, splitting < 1, c = 1/2 -> half width c (l + 1) = 1 exactly; the last l = 1
    # frequency is x_last + 1 - step, every operand dyadic.  `>=` moves lo to x_last - c (i0 = Nx - 1 - c / step = Nx - 9), `>` would
    # leave it at x_last - step (i0 = Nx - 2).
    mk = Maker(model_id, 1, 3, nnoise=1, f0=64.0, dnu=8.0)
    g = Group(f"id{model_id}-clip-on-x-last", model_id, mk.plength, dyadic_grid(513, 56.0, step), True)
    p = mk.vector(rng, trunc_c=0.5, wlo=0.5, whi=0.5, a1=0.5, a3=0.0, slopes=False)  # (equal widths: interpolated exactly)
    if model_id == LOCAL:
        mk.set_local_inc(p, None, p3=0.5, p4=0.5)
    p[mk.o_f[1] + 2] = g.grid.x_last + 1.0 - step
    i = g.add("lo-plus-step-on-x-last", p)
    row = (2 * 2 + 1) if model_id in (CLASSIC, V2, V3) else 3 + 2
    g.exact_edges |= {(i, row, "clip_lo"), (i, row, "i0")}       # (x_last - c is on the grid too: quotient Nx - 9 exactly)
    out.append(g)
    return out


def random_groups(model_id, seeds=(0, 1, 2)):
    """Random vectors per id and lmax: four vectors per group, Nfl0 cycling through 2, 3, 16, 17."""
    out = []
    for lmax in range(4):
        for s in seeds:
            rng = np.random.default_rng(50000 + 1000 * model_id + 10 * lmax + s)
            nfl0 = (2, 3, 16, 17)[(lmax + s) % 4]
            mk = Maker(model_id, lmax, nfl0, nnoise=(1, 4, 7, 10)[(lmax + 2 * s) % 4], f0=rng.uniform(30.0, 300.0), dnu=rng.uniform(4.0, 9.0))
            lo, hi = mk.span()
            step = rng.uniform(0.04, 0.09)
            nx = min(4097, int((hi - lo) / step) + 1)
            g = Group(f"id{model_id}-random-lmax{lmax}-s{s}", model_id, mk.plength, lo + step * np.arange(nx, dtype=np.float64), False)
            for v in range(4):
                g.add(f"v{v}", mk.vector(rng, inc=rng.uniform(0.0, 90.0), do_amp=int(rng.integers(0, 2)), trunc_c=rng.uniform(0.5, 20.0),
                                         a1=rng.uniform(0.2, 3.0), a3=rng.uniform(-0.05, 0.05), asym=rng.uniform(-50.0, 50.0),
                                         eta=float(rng.integers(0, 2)), neg=bool(rng.integers(0, 2))))
            out.append(g)
    return out


_GROUPS = {}


def groups(model_id):
    if model_id not in _GROUPS:
        _GROUPS[model_id] = directed_groups(model_id) + random_groups(model_id)
    return _GROUPS[model_id]


def all_groups():
    return [g for m in IDS for g in groups(m)]

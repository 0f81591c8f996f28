"""Small directed cases for the red-giant pre-step (ids 25 / 27), shared by tests/test_rgb_reference.py (CPU) and
tests/test_gpu_rgb_reference.py (MI355X).  A case is a parameter vector, its layout, a frequency grid and what it is there for; where a
case names a branch, `expect` says what the reference must report (tests/test_rgb_reference.py asserts it from the reference alone).

Default grid: 3400 bins of 0.05 muHz from 110 muHz, six radial orders, 20 to 60 mixed modes; a case leaves it only where it IS another grid.
References are computed once per process and shared (`reference`, `twin`, `finished`)."""
import functools

import numpy as np

import rgb_reference as rr

DEFAULT_X = 110.0 + 0.05 * np.arange(3400)


def make_params(rng, nmax=6, dnu=20.0, epsilon=0.2, n_first=6, delta0l=-0.6, DPl=80.0, alpha_g=0.0, q=0.15, nferr=4, bias_type=0, model_type=0,
                rot_env=0.1, rot_core=0.6, inclination=55.0, trunc_c=20.0, ferr_scale=0.05, cte_width=False, Wfactor=0.9, Hfactor=0.9, jitter=0.01,
                fref=None, do_amp=0.0, fl0=None, eta_switch=1.0):
    """A parameter vector of model_RGB_asympt_aj_AppWidth_HarveyLike_v4 / _CteWidth_ in the layout of models.cpp:4716-4733."""
    n = np.arange(nmax)
    if fl0 is None:
        fl0 = (n_first + n + epsilon) * dnu + rng.uniform(-jitter, jitter, nmax) * dnu
    fl0 = np.asarray(fl0, dtype=np.float64)
    numax = fl0.mean()
    heights = 40.0 * np.exp(-0.5 * ((fl0 - numax) / (1.2 * dnu)) ** 2) + 2.0
    if fref is None:
        fref = (n_first + 1 + np.arange(nferr) * max((nmax - 2) / max(nferr - 1, 1), 1) + epsilon + 0.5) * dnu
    ferr = rng.uniform(-ferr_scale, ferr_scale, nferr) if bias_type != 0 else np.zeros(nferr)
    l1 = np.concatenate([[delta0l, DPl, alpha_g, q, 0.0, 0.0, Wfactor, Hfactor], fref, ferr])
    fl2, fl3 = fl0[1:] - 0.12 * dnu, fl0[:-1] + 0.21 * dnu
    split = np.array([rot_env, rot_core, 0.0, 0.0, 0.01, 0.0, 0.0, 0.0, eta_switch, 0.0])
    width = np.array([0.14]) if cte_width else np.array([numax, numax, 1.5, 0.15, 0.8 * numax, 2.5])
    noise = np.array([30.0, 40.0, 2.0, 10.0, 8.0, 2.0, 0.4])
    cfg = np.array([trunc_c, do_amp, 0.0, float(model_type), float(bias_type), float(nferr)])
    params = np.concatenate([heights, [1.5, 0.53, 0.08], fl0, l1, fl2, fl3, split, width, noise, [inclination], cfg])
    plength = np.array([nmax, 3, nmax, l1.size, fl2.size, fl3.size, 10, width.size, 7, 1, 6], dtype=np.int32)
    assert params.size == plength.sum()
    return params, plength


class Case:
    def __init__(self, name, model_id, params, plength, x=None, expect=None, product_limit=False):
        self.name, self.model_id, self.params, self.plength = name, model_id, np.asarray(params, dtype=np.float64), np.asarray(plength, dtype=np.int32)
        self.x = DEFAULT_X if x is None else x
        self.expect = expect or {}
        self.product_limit = product_limit      # refused because of a stated limit of the product (MAXP): the reference model has no such limit

    def __repr__(self):
        return self.name


def _grid_for(params, plength, step, margin=1.3):
    o = np.cumsum([0] + list(plength))
    fl0 = params[o[2]:o[3]]
    dnu = (fl0.max() - fl0.min()) / (fl0.size - 1)
    lo = fl0.min() - margin * dnu
    return lo + step * np.arange(int((fl0.max() - fl0.min() + 2 * margin * dnu) / step))


BASE_VARIANTS = [(0, 0, False), (1, 0, False), (2, 1, False), (0, 1, False), (1, 0, True), (0, 1, True)]


@functools.lru_cache(maxsize=None)
def _cases():
    out = []

    def add(name, cte=False, x=None, expect=None, product_limit=False, seed=5, mutate=None, **kw):
        p, pl = make_params(np.random.default_rng(seed), cte_width=cte, **kw)
        if mutate:
            p, pl = mutate(p, pl)
        out.append(Case(name, rr.ID_CTE if cte else rr.ID_APP, p, pl, x=x, expect=expect, product_limit=product_limit))
    for bt, mt, cte in BASE_VARIANTS:
        add(f"base-b{bt}-m{mt}-{'cte' if cte else 'app'}", cte=cte, bias_type=bt, model_type=mt, expect={"modes": (20, 60)})
    add("weak-coupling-q1e-3", q=1e-3, bias_type=1, expect={"lost": True})
    add("strong-coupling-q0.6", q=0.6, bias_type=0)
    # Ratio-test pairs, found by bisection on the period spacing in the reference: in each pair ONE candidate (p mode, kind of
    # lin_interpol branch, frequency) is just accepted in the first vector and just rejected in the second; the margin to the gate is at
    # least 1e-6 of the ratio on both sides and for both local grids.  Coarse steps and strong coupling: only there does a candidate's
    # ratio come near the LOWER gate (an extrapolation from the window's first two points).
    for gate, q, step, mt, ip, kind, prop, (d_in, d_out) in (
            ("0.999", 0.8164674713957979, 0.1, 0, 0, "below", 109.8827, (76.21605172061646, 76.21605953311646)),
            ("1.001", 0.7764249450324676, 0.2, 1, 2, "above", 160.8073, (150.22923527213982, 150.22873527213983))):
        xg = 110.0 + step * np.arange(int(170 / step))
        for side, d in (("accepted", d_in), ("rejected", d_out)):
            add(f"ratio-gate-{gate}-{side}", DPl=d, q=q, model_type=mt, x=xg,
                expect={"gate": dict(gate=gate, ip=ip, kind=kind, prop=prop, accepted=side == "accepted")})
    # A mode whose sign-change cell is the SECOND above a pole's cell, with the pole just below the refinement window (found by a scan in
    # the reference): the first cell of a pole-free stretch of the structured scan.
    add("root-two-cells-above-a-pole", DPl=113.8988397592393, q=0.5104570966371511, x=110.0 + 0.2 * np.arange(850),
        expect={"above_pole": dict(ip=1, cell=188)})
    # fewer than six g modes in range: the wide zones; model_type 0: numin < 0, the grid starts at 0
    # (not 1500: the ends of the zeta grid would then be 1e6/(2 DPl) and 1e6/(6 DPl) and its point count an exact integer, 28032)
    add("few-g-m0", DPl=1530.0, model_type=0, expect={"few_g": True, "numin_negative": True})
    add("few-g-m1", DPl=1530.0, model_type=1, expect={"few_g": True})
    add("no-g-mode", DPl=1e9, expect={"no_modes": True})
    # low-frequency giants on a grid of 0.02 muHz: both overrides of the local grid's factor
    for name, n_first, fact in (("low-frequency-fact0.01", 30, "0.01"), ("low-frequency-fact0.005", 10, "0.005")):
        p, pl = make_params(np.random.default_rng(8), dnu=4.0, n_first=n_first, DPl=150.0 if n_first == 10 else 300.0, delta0l=-0.1)
        out.append(Case(name, rr.ID_APP, p, pl, x=_grid_for(p, pl, 0.02), expect={"fact": fact}))
    # Hfactor = Wfactor = 1: hr = sqrt(1 - zeta) is smallest where zeta is largest.  Without a bias a mode is a zero of p - g and its zeta stays
    # below the 4-year grid's maximum (tests/test_rgb_reference.py, test_zeta_of_an_unbiased_mode_stays_below_the_grid_maximum): no clip here.
    add("hfactor-1", Hfactor=1.0, Wfactor=1.0, bias_type=1, expect={"hr_below": 0.2})
    # The clip.  zeta is evaluated at root + bias, and zeta's sum is exactly Lp Lg at a pole of tan X -- at least the 4-year grid's maximum.
    # The second bias node value is tuned (bisection in the reference) so that the spline carries mode 0 onto the pole at 119.617225 muHz:
    # z = 1 + 4.5e-8 before the clip (the clip also holds 4e-5 muHz to either side), then hr = sqrt(1 - 1) = 0 is lifted to 1e-10.

    def onto_pole(p, pl):
        p = p.copy()
        p[int(pl[0] + pl[1] + pl[2]) + 8 + 4 + 1] = -0.08285799259726292
        return p, pl
    add("clip-on-a-pole", Hfactor=1.0, Wfactor=1.0, bias_type=1, mutate=onto_pole, expect={"clip": (0,)})
    # bias splines whose nodes cover the middle of the spectrum only: modes below the first node and above the last
    add("spline-extrapolation-cubic-3", bias_type=1, nferr=3, fref=np.array([160.0, 175.0, 190.0]), expect={"branches": {"left", "in", "right"}})
    add("spline-extrapolation-hermite-16", bias_type=2, nferr=16, fref=150.0 + 3.0 * np.arange(16), model_type=1,
        expect={"branches": {"left", "in", "right"}})
    # runs of roots chained within the unique tolerance: a spectrum step of 0.3 muHz
    add("unique-runs", DPl=19.0, q=0.6, alpha_g=0.5, x=110.0 + 0.3 * np.arange(506), expect={"runs": True})
    # Near the row cap.  On the default grid the solver itself cannot deliver 380 modes: with g modes this dense most roots share their
    # 0.05 muHz cell with a pole of tan X, the two sign changes cancel and the root is never seen (at most ~150 survive for any period
    # spacing and coupling).  The case therefore IS another grid: 0.01 muHz over the same range, strong coupling.
    fine = 110.0 + 0.01 * np.arange(17000)
    add("near-row-cap", DPl=9.5, q=0.6, x=fine, expect={"modes": (380, 400)})
    add("over-row-cap", DPl=8.3, q=0.6, x=fine, expect={"status": rr.ERR_BAD_ARG, "over_cap": True})
    irregular = (6 + np.arange(6) + 0.2) * 20.0 + np.array([0.0, 1.1, -0.94, 0.7, -1.25, 0.4])
    add("irregular-ladder-m1", model_type=1, bias_type=2, fl0=irregular, expect={"irregular": True})
    # refusals
    add("refuse-nferr17", bias_type=1, nferr=17, expect={"status": rr.ERR_BAD_ARG}, product_limit=True)

    def reverse(p, pl):
        o = np.cumsum([0] + list(pl))
        p = p.copy()
        p[o[2]:o[3]] = p[o[2]:o[3]][::-1]
        return p, pl
    add("refuse-decreasing-ladder", mutate=reverse, expect={"status": rr.ERR_BAD_ARG})
    add("refuse-fmin-below-dnu", n_first=0, epsilon=0.5, nmax=4, expect={"status": rr.ERR_BAD_ARG})
    add("refuse-m1-33-p-modes", model_type=1, nmax=32, dnu=5.0, n_first=20, expect={"status": rr.ERR_BAD_ARG}, product_limit=True)
    add("refuse-m1-no-p-mode", model_type=1, delta0l=-500.0, expect={"status": rr.ERR_BAD_ARG})

    def one_width(p, pl):
        o = np.cumsum([0] + list(pl))
        pl = pl.copy()
        pl[7] = 1
        return np.concatenate([p[:o[7] + 1], p[o[8]:]]), pl
    add("refuse-width-block-length", mutate=one_width, expect={"status": rr.ERR_BAD_ARG})
    # random vectors at fixed seeds
    for k in range(20):
        rng = np.random.default_rng(1000 + k)
        dnu = float(rng.uniform(8.0, 22.0))
        kw = dict(dnu=dnu, epsilon=float(rng.uniform(0.05, 0.95)), delta0l=float(rng.uniform(-0.9, 0.3)), DPl=float(rng.uniform(60.0, 320.0)),
                  alpha_g=float(rng.uniform(0.0, 0.9)), q=float(rng.uniform(0.03, 0.7)), Wfactor=float(rng.uniform(0.3, 1.0)),
                  Hfactor=float(rng.uniform(0.3, 1.0)), inclination=float(rng.uniform(2.0, 88.0)), rot_env=float(rng.uniform(0.0, 0.4)),
                  rot_core=float(rng.uniform(0.1, 1.5)), model_type=k % 2, bias_type=k % 3, nmax=int(rng.integers(4, 9)), n_first=int(rng.integers(5, 12)),
                  do_amp=float(k % 4 == 3))
        cte = k % 5 == 4
        p, pl = make_params(rng, cte_width=cte, **kw)
        out.append(Case(f"random-{k}", rr.ID_CTE if cte else rr.ID_APP, p, pl, x=_grid_for(p, pl, 0.05 if k % 3 else 0.031)))
    return out


def all_cases():
    return list(_cases())


_EXTRA = {}
# the cases that also run as gradient batches with six perturbed slots (each slot needs a reference of its own: not every case)
BATCHED = ("base-b1-m0-app", "base-b2-m1-app", "base-b0-m1-cte", "few-g-m0", "low-frequency-fact0.005", "spline-extrapolation-hermite-16",
           "unique-runs", "random-4", "random-9", "ratio-gate-0.999-accepted", "ratio-gate-1.001-rejected", "hfactor-1", "clip-on-a-pole",
           "irregular-ladder-m1")


def by_name(name):
    return _EXTRA[name] if name in _EXTRA else {c.name: c for c in _cases()}[name]


def adhoc(name, model_id, params, plength, x):
    """A case made on the spot (a vector an engine stored), registered so that its references are shared like the others'."""
    if name not in _EXTRA:
        _EXTRA[name] = Case(name, model_id, params, plength, x=x)
    return _EXTRA[name]


def perturbed(case):
    """The six perturbed slots of a gradient batch on `case`: (index_to_relax, hstep, cases) -- period spacing, coupling, delta0l, one
    radial frequency, inclination, Hfactor; slot k's vector is the base with hstep[k] added to parameter index_to_relax[k] in double."""
    L = rr.Layout(case.plength)
    idx = np.array([L.o1 + 1, L.o1 + 3, L.o1, L.o0 + 2, L.oi, L.o1 + 7], dtype=np.int32)
    h = np.array([0.013, 0.004, 0.01, 0.03, 1.5, -0.02])
    out = []
    for k, (i, d) in enumerate(zip(idx, h)):
        p = case.params.copy()
        p[i] = p[i] + d
        name = f"{case.name}+slot{k + 1}"
        if name not in _EXTRA:
            _EXTRA[name] = Case(name, case.model_id, p, case.plength, x=case.x)
        out.append(_EXTRA[name])
    return idx, h, out


@functools.lru_cache(maxsize=None)
def _reference(name, twin):
    c = by_name(name)
    return rr.build(c.model_id, c.params, c.plength, c.x, twin=twin)


def reference(case):
    return _reference(case.name, False)


def twin(case):
    return _reference(case.name, True)


@functools.lru_cache(maxsize=None)
def _finished(name, choice):
    return rr.finish(_reference(name, False), list(choice) if choice is not None else None)


def finished(case, choice=None):
    """Stages (c)-(e) of the definition at a choice of local grids per root (None: the full grid everywhere)."""
    return _finished(case.name, tuple(choice) if choice is not None else None)

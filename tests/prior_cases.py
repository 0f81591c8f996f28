"""Stars and parameter vectors for the log-prior parity tests (test_priors.py on the CPU, test_gpu_priors.py on the device).

synth.py keeps its defaults: the prior tables of the stars it makes are overwritten HERE so that every primitive id the product
implements (1, 2, 4, 5, 6, 7, 8, 10) and every hard constraint of the five prior classes is met by some vector.  All stars carry
nx = 2000 bins: the spectrum only has to exist.

zoo(synth) -> {name: Zoo}.  A Zoo holds the star and a list of Case(label, kind, params, expect):
    kind "inside"  the start vector and seeded jitters of it (the recipe of test_priors.py at 5e-4 relative) that the reference finds
                   inside every support;
    kind "edge"    one parameter moved onto / just outside an edge of its primitive prior, into a Gaussian tail (0.1, 3, 30 sigma) or to
                   a negative value (the _abs ids) -- the first and the last parameter carrying each id;
    kind "fail"    breaks exactly one hard constraint, named in `expect` (the start of the reference's name for it);
    kind "pass"    the twin of a "fail" case just on the passing side.
A constraint decided by a computed quantity (a ratio, a ratio sum, the width bound) is placed a factor 1 +- 1e-6 from its threshold; one
decided by a stored double sits on the exact edge and its np.nextafter neighbour.
"""
import copy

import numpy as np

NX = 2000
EPS = 1e-6


class Case:
    def __init__(self, label, kind, params, expect=None):
        self.label, self.kind, self.params, self.expect = label, kind, np.array(params, dtype=np.float64), expect


class Zoo:
    def __init__(self, name, star):
        self.name, self.star, self.cases = name, star, []
        self.spectrum_of = None  # a star of another model id whose model serves as this star's spectrum (ids the oracle has no model for)

    def add(self, label, kind, params, expect=None):
        self.cases.append(Case(label, kind, params, expect))

    @property
    def P(self):
        return np.array([c.params for c in self.cases])

    def fd_step(self):
        """The forward-difference steps of test_device_priors_match_host, from the star's own start vector."""
        return 1e-7 * np.maximum(np.abs(self.star.params[self.star.index_to_relax]), 1e-3)


def _own_tables(star):
    s = copy.copy(star)
    s.params, s.priors, s.priors_switch = star.params.copy(), star.priors.copy(), star.priors_switch.copy()
    s.relax, s.extra_priors = star.relax.copy(), star.extra_priors.copy()
    return s


def _set(star, i, kind, *vals):
    star.priors_switch[i] = kind
    star.priors[:, i] = -9999.0
    star.priors[:len(vals), i] = vals


def _offsets(star):
    return np.concatenate([[0], np.cumsum(star.plength)]).astype(int)


def _below(v):
    return np.nextafter(v, -np.inf)


def _above(v):
    return np.nextafter(v, np.inf)


NEG0 = _below(0.0)  # the largest negative double


# ---------------------------------------------------------------- stars ----------------------------------------------------------------
def _dress_global(star):
    """ids 5-10 on an aj-family (or Classic) global star; Gaussian priors where a hard constraint must be breakable alone."""
    o = _offsets(star)
    p = star.params
    nmax = int(star.plength[0])
    for n in range(0, nmax, 3):
        _set(star, n, 10, 1.0, 1.0e4)                                        # some heights: Jeffreys on |h|
    for i in range(o[1], o[2]):
        _set(star, i, 7, 0.95 * p[i], 1.05 * p[i], 0.03 * p[i], 0.01 * p[i])  # visibilities: Gaussian-Uniform-Gaussian
    for i in range(o[2], o[6], 3):
        _set(star, i, 6, p[i] - 8.0, p[i] + 8.0, 0.1)                        # some frequencies: Gaussian-Uniform
    for i in range(o[7], o[8], 2):
        _set(star, i, 5, 0.1, 10.0, 1.0)                                     # some widths: Uniform-Gaussian
    on = o[8]
    for i in (on + 3, on + 4, on + 6):
        _set(star, i, 2, p[i], 0.2 * p[i])                                   # second Harvey H, tc and the white noise: Gaussian
    _set(star, o[9], 2, p[o[9]], 10.0)                                       # first slot after the noise (inclination / first ratio)
    return o


def make_zoo_global(synth, nmax=14, lmax=3, step=1.0):
    star = _own_tables(synth.make_c3_star(nx=NX, step=step, nmax=nmax, lmax=lmax))
    o = _dress_global(star)
    a1 = star.params[o[6]]
    star.params[o[6] + 4], star.params[o[6] + 8] = 0.01 * a1, 0.004 * a1     # a3, a5 non-zero
    _set(star, o[6], 8, 0.0, 8.0)                                            # a1_0: Uniform on |a1|
    _set(star, o[6] + 9, 2, 0.0, 1.0)                                        # a5_1 (fixed): its id switches the third noise check on
    return star


def make_zoo_local(synth):
    """model_MS_local_basic in the sqrt(a1) cos i, sin i form (the a1 slot is 0)."""
    star = _own_tables(synth.make_c2_star(nx=NX))
    p, o = star.params, _offsets(star)
    _set(star, 0, 10, 1.0, 1.0e4)
    _set(star, 1, 5, 1.0, 30.0, 5.0)
    _set(star, o[2], 6, p[o[2]] - 5.0, p[o[2]] + 5.0, 0.1)
    _set(star, o[2] + 1, 7, p[o[2] + 1] - 5.0, p[o[2] + 1] + 5.0, 0.1, 0.2)
    _set(star, o[6] + 3, 8, 0.0, 2.5)                                        # sqrt(a1) cos i: Uniform on the absolute value
    _set(star, o[6] + 4, 8, 0.1, 2.5)
    _set(star, o[7], 5, 0.1, 10.0, 1.0)
    _set(star, o[7] + 1, 10, 0.05, 40.0)
    return star


def make_zoo_local_a1(synth):
    """The same star with a value in the a1 slot (priors_local then takes a3 / a1 from it) and a free inclination slot."""
    star = make_zoo_local(synth)
    o = _offsets(star)
    star.params[o[6]] = 1.2
    star.params[o[9]] = 40.0
    star.relax[o[9]] = 1
    _set(star, o[9], 2, 40.0, 10.0)
    return star


def make_zoo_hnlm(synth):
    star = _own_tables(synth.make_hnlm_star(nx=NX))
    p, o = star.params, _offsets(star)
    _set(star, 0, 10, 1.0e-3, 1.0e4)
    _set(star, 2, 5, 1.0e-3, 50.0, 5.0)
    _set(star, 3, 7, 1.0e-3, 50.0, 1.0e-4, 5.0)
    _set(star, o[2], 6, p[o[2]] - 5.0, p[o[2]] + 5.0, 0.1)
    _set(star, o[6], 8, 0.0, 6.0)                                            # Splitting_a1
    _set(star, o[7], 5, 0.1, 10.0, 1.0)
    return star


def make_zoo_v2(synth):
    star = _own_tables(synth.make_v2_star(nx=NX, step=1.0))
    o = _dress_global(star)
    star.params[o[9]:o[9] + 9] *= 0.9        # the ratio sums at 0.9: the start vector is not 1e-10 under the bound 1 + 1e-10
    for i in (o[9], o[9] + 1, o[9] + 2, o[9] + 5):  # Gaussian: the noise checks read the first three (the block after the seven noise
        _set(star, i, 2, star.params[i], 0.1)        # parameters), the fourth takes the l = 3 sum under 0
    return star


def make_zoo_rgb(synth):
    star = _own_tables(synth.make_c5_star(nx=NX, nmax=7))
    p, o = star.params, _offsets(star)
    _set(star, 0, 10, 0.1, 1.0e4)
    _set(star, 1, 5, 0.1, 100.0, 10.0)
    _set(star, o[2], 6, p[o[2]] - 0.9, p[o[2]] + 0.9, 0.05)
    _set(star, o[2] + 1, 7, p[o[2] + 1] - 0.9, p[o[2] + 1] + 0.9, 0.05, 0.1)
    _set(star, o[3] + 6, 2, p[o[3] + 6], 0.2)                                # Wfactor, Hfactor: Gaussian
    _set(star, o[3] + 7, 2, p[o[3] + 7], 0.2)
    _set(star, o[6], 8, 0.0, 1.0)                                            # rot_env
    on = o[8]
    _set(star, on + 3, 2, p[on + 3], 0.2 * p[on + 3])
    _set(star, on + 6, 2, p[on + 6], 0.2 * p[on + 6])
    _set(star, o[9], 2, p[o[9]], 10.0)
    _set(star, o[6] + 9, 2, 0.0, 1.0)                                        # asymmetry slot (fixed): switches the third noise check on
    return star


def make_zoo_env(synth, model_id):
    star = _own_tables(synth.make_envelope_star(model_id, nx=NX))
    p = star.params
    if model_id == 1:
        _set(star, 1, 5, 5.0, 500.0, 50.0)
        _set(star, 4, 6, 0.0, 100.0, 5.0)
        _set(star, 6, 8, 0.0, 10.0 * p[6])
        _set(star, 7, 10, 0.1 * p[7], 100.0 * p[7])
        _set(star, 8, 7, 0.6 * p[8], 1.4 * p[8], 0.5, 3.0)
        _set(star, 9, 1, 1.0, 3.0 * p[9])                                    # Gauss_sigma: the Stello bound lies inside the support
    else:
        _set(star, 5, 2, p[5], 0.3 * p[5])                                   # a1, a2: Gaussian
        _set(star, 6, 2, p[6], 0.3 * p[6])
        _set(star, 13, 8, 0.0, 10.0 * p[13])
        _set(star, 14, 10, 0.1 * p[14], 100.0 * p[14])
        _set(star, 15, 7, 0.6 * p[15], 1.4 * p[15], 0.5, 3.0)
        _set(star, 16, 5, 0.3 * p[16], 3.0 * p[16], 4.0)
    return star


# --------------------------------------------------------------- vectors ---------------------------------------------------------------
def _inside(zoo, ref, n=20, seed=4, rel=5e-4):
    star = zoo.star
    idx = star.index_to_relax
    rng = np.random.default_rng(seed)
    zoo.add("start", "inside", star.params)
    k = tries = 0
    while k < n and tries < 20 * n:
        tries += 1
        p = star.params.copy()
        p[idx] *= 1.0 + rel * rng.standard_normal(idx.size)
        if ref.star_log_prior(star, p).failed is None:
            zoo.add("jitter %d" % k, "inside", p)
            k += 1
    assert k == n, (zoo.name, k)


def _edge_values(kind, b):
    lo, hi, s1, s2 = b
    if kind == 1:
        return [("b_min", lo), ("b_max", hi), ("below b_min", _below(lo)), ("above b_max", _above(hi))]
    if kind == 8:
        v = [("|x| = b_max", hi), ("x = -b_max", -hi), ("|x| above b_max", _above(hi)), ("x below -b_max", -_above(hi)),
             ("negative inside", -0.5 * (lo + hi)), ("|x| = b_min", lo)]
        if lo > 0:
            v += [("x = -b_min", -lo), ("|x| below b_min", _below(lo)), ("x above -b_min", -_below(lo))]
        return v
    if kind == 4:
        return [("h = 0", 0.0), ("h = hmax", hi), ("h just above 0", _above(0.0)), ("h just below hmax", _below(hi)), ("h negative", -1.0)]
    if kind == 10:
        return [("h = 0", 0.0), ("|h| = hmax", hi), ("h = -hmax", -hi), ("h just below hmax", _below(hi)), ("h just above -hmax", -_below(hi)),
                ("negative inside", -0.25 * hi)]
    tails = (0.1, 3.0, 30.0)
    if kind == 5:
        return ([("b_min", lo), ("b_max", hi), ("below b_min", _below(lo))] + [("b_max + %g sigma" % t, hi + t * s1) for t in tails])
    if kind == 6:
        return ([("b_min", lo), ("b_max", hi), ("above b_max", _above(hi))] + [("b_min - %g sigma" % t, lo - t * s1) for t in tails])
    if kind == 7:
        return ([("b_min", lo), ("b_max", hi)] + [("b_min - %g sigma1" % t, lo - t * s1) for t in tails] +
                [("b_max + %g sigma2" % t, hi + t * s2) for t in tails])
    if kind == 2:
        return [("mean + 30 sigma", lo + 30.0 * hi)]
    return []


def _edges(zoo):
    star = zoo.star
    for kind in (1, 2, 4, 5, 6, 7, 8, 10):
        where = np.flatnonzero(star.priors_switch == kind)
        for i in sorted(set(where[[0, -1]])) if where.size else ():
            for what, v in _edge_values(kind, star.priors[:, i]):
                p = star.params.copy()
                p[i] = v
                zoo.add("id %d on parameter %d (%s): %s" % (kind, i, star.names[i], what), "edge", p)


def _pair(zoo, what, expect, i, v_fail, v_pass, base=None):
    for kind, v in (("fail", v_fail), ("pass", v_pass)):
        p = (zoo.star.params if base is None else base).copy()
        p[i] = v
        zoo.add("%s: %s" % (what, kind), kind, p, expect)


def _noise_constraints(zoo, on, o_sw3_ok):
    names = zoo.star.names
    for k in (3, 4, 5):
        _pair(zoo, "noise check 1, parameter %d (%s) negative" % (on + k, names[on + k]), "noise check 1", on + k, NEG0, 0.0)
    for k in (6, 7, 8):
        _pair(zoo, "noise check 2, parameter %d (%s) negative" % (on + k, names[on + k]), "noise check 2", on + k, NEG0, 0.0)
    if o_sw3_ok:
        _pair(zoo, "noise check 3, parameter %d (%s) negative" % (on + 9, names[on + 9]), "noise check 3", on + 9, NEG0, 0.0)


def _aj_vector(star, o, j, i_target, factor, slope_sign):
    """a_j(nu) = c0 + c1 (1e-3 nu) with |a_j / a1| = limit_j * factor at the mode whose frequency is parameter i_target, and a slope that
    makes the ratio grow (slope_sign = +1) or fall (-1) with frequency by 2 % of the limit per mHz; every other a_j a thousand times
    under its limit."""
    p = star.params.copy()
    a1 = p[o[6]]
    assert p[o[6] + 1] == 0.0 and a1 > 0
    lim = star.extra_priors[2 + j]
    for jj in range(1, 6):
        p[o[6] + 2 * jj], p[o[6] + 2 * jj + 1] = 1e-3 * star.extra_priors[2 + jj] * a1, 0.0
    c1 = slope_sign * 0.02 * lim * a1
    x = p[i_target] * 1e-3
    p[o[6] + 2 * j], p[o[6] + 2 * j + 1] = lim * factor * a1 - c1 * x, c1
    return p


def _aj_constraints(zoo, o):
    """|a_j / a1| >= limit_j (model_index 9).  The ratio is monotone in frequency, so one (degree, order) pair alone can break the limit
    only at the highest (slope +) or lowest (slope -) frequency of the degrees >= 1: those two pairs get every j = 1..5, failing and
    passing twin.  The first and last order of EVERY degree are met too (j = 2): there the pairs beyond the target in frequency fail
    with it, and the twin is the vector with the same slope whose extreme pair sits just under the limit."""
    star = zoo.star
    lmax = int(star.plength[1])
    first = {l: o[2] + int(star.plength[2:2 + l].sum()) for l in range(1, lmax + 1)}
    last = {l: first[l] + int(star.plength[2 + l]) - 1 for l in range(1, lmax + 1)}
    ends = [first[l] for l in first] + [last[l] for l in last]
    i_hi = max(ends, key=lambda i: star.params[i])
    i_lo = min(ends, key=lambda i: star.params[i])
    for j in range(1, 6):
        for i, sgn, which in ((i_hi, +1, "highest"), (i_lo, -1, "lowest")):
            for kind, f in (("fail", 1 + EPS), ("pass", 1 - EPS)):
                zoo.add("a%d/a1 at the %s l>=1 mode (parameter %d) x (1 %+g): %s" % (j + 1, which, i, f - 1, kind), kind,
                        _aj_vector(star, o, j, i, f, sgn), "|a%d/a1| over its limit" % (j + 1))
    for l in range(1, lmax + 1):
        for i, sgn, which in ((first[l], -1, "first"), (last[l], +1, "last")):
            zoo.add("a3/a1 over the limit from the %s order of l=%d on (parameter %d): fail" % (which, l, i), "fail",
                    _aj_vector(star, o, 2, i, 1 + EPS, sgn), "|a3/a1| over its limit")
    # a1 < 0 with small ratios: only the sign check rejects (|x| prior on a1_0); twin: the same vector with a1 > 0
    p = _aj_vector(star, o, 1, i_hi, 1e-3, +1)
    q = p.copy()
    p[o[6]] = -p[o[6]]
    zoo.add("a1 < 0, ratios a thousand times under their limits: fail", "fail", p, "a1 < 0")
    zoo.add("a1 < 0, ratios a thousand times under their limits: pass", "pass", q, "a1 < 0")


def _fill_global(zoo, ref, aj):
    star = zoo.star
    o = _offsets(star)
    _inside(zoo, ref)
    _edges(zoo)
    for i in range(o[1], o[2]):
        _pair(zoo, "negative visibility, parameter %d" % i, "negative visibility", i, NEG0, 0.0)
    _noise_constraints(zoo, o[8], star.priors_switch[o[6] + 9] != 0)
    if aj:
        _aj_constraints(zoo, o)


def _fill_v2(zoo, ref):
    star = zoo.star
    o = _offsets(star)
    _fill_global(zoo, ref, aj=False)
    q = o[9]
    blocks = {1: (q, [q + 1]), 2: (q + 2, [q + 3, q + 4]), 3: (q + 5, [q + 6, q + 7, q + 8])}
    for l, (i0, rest) in blocks.items():
        twice = 2 * star.params[rest].sum()
        for kind, f in (("fail", 1 + EPS), ("pass", 1 - EPS)):
            p = star.params.copy()
            p[i0] = (1. + 1e-10) * f - twice
            zoo.add("ratio sum l=%d at (1 + 1e-10) x (1 %+g): %s" % (l, f - 1, kind), kind, p, "ratio sum l=%d" % l)
    # lower bound 0 of the l = 3 sum (its m = 0 ratio carries a Gaussian prior: a negative value is inside it, and no noise check reads it)
    twice = 2 * star.params[q + 6:q + 9].sum()
    for kind, s in (("fail", -EPS), ("pass", +EPS)):
        p = star.params.copy()
        p[q + 5] = s - twice
        zoo.add("ratio sum l=3 at %+g: %s" % (s, kind), kind, p, "ratio sum l=3")


def _fill_local(zoo, ref, form):
    star = zoo.star
    o = _offsets(star)
    _inside(zoo, ref)
    _edges(zoo)
    lim = star.extra_priors[2]
    a1 = star.params[o[6]] if form == "a1" else star.params[o[6] + 3] ** 2 + star.params[o[6] + 4] ** 2
    what = "a1 fitted" if form == "a1" else "sqrt(a1) cos i, sin i"
    for sgn in (+1, -1):
        _pair(zoo, "a3/a1 (%s) at %+d x limit x (1 +- 1e-6)" % (what, sgn), "|a3/a1| over its limit (%s)" % what, o[6] + 2,
              sgn * lim * a1 * (1 + EPS), sgn * lim * a1 * (1 - EPS))
    if form != "a1":
        # neither branch: a1 slot 0 and sqrt(a1) cos i = 0 -- no limit on a3 at all
        p = star.params.copy()
        p[o[6] + 3], p[o[6] + 2] = 0.0, 50.0
        zoo.add("no a1 at all (cos slot 0), a3 = 50: no constraint", "pass", p, "|a3/a1|")
    oi = o[9]
    if star.priors_switch[oi] != 0:
        _pair(zoo, "negative inclination slot", "negative inclination", oi, NEG0, 0.0)


def _fill_rgb(zoo, ref):
    star = zoo.star
    o = _offsets(star)
    _inside(zoo, ref)
    _edges(zoo)
    for i in range(o[1], o[2]):
        _pair(zoo, "negative visibility, parameter %d" % i, "negative visibility", i, NEG0, 0.0)
    lim, rot = star.extra_priors[2], abs(star.params[o[6]])
    for sgn in (+1, -1):
        _pair(zoo, "a3/rot_env at %+d x limit x (1 +- 1e-6)" % sgn, "|a3/rot_env| over its limit", o[6] + 4, sgn * lim * rot * (1 + EPS),
              sgn * lim * rot * (1 - EPS))
    base = star.params.copy()
    base[o[6]] = -base[o[6]]   # rot_env enters through its absolute value
    _pair(zoo, "a3/|rot_env|, rot_env negative", "|a3/rot_env| over its limit", o[6] + 4, lim * rot * (1 + EPS), lim * rot * (1 - EPS), base)
    _noise_constraints(zoo, o[8], star.priors_switch[o[6] + 9] != 0)
    for i in range(o[7], o[8]):
        if star.priors_switch[i] == 2:
            _pair(zoo, "width-law parameter %d (%s) negative" % (i, star.names[i]), "negative width-law parameter", i, NEG0, 0.0)
    _pair(zoo, "negative Wfactor", "negative Wfactor", o[3] + 6, NEG0, 0.0)
    _pair(zoo, "negative Hfactor", "negative Hfactor", o[3] + 7, NEG0, 0.0)


def _fill_env(zoo, ref):
    star = zoo.star
    _inside(zoo, ref)
    _edges(zoo)
    i_numax, i_sig = (8, 9) if star.prior_class == 1 else (15, 16)
    from decimal import Decimal, localcontext
    with localcontext() as c:
        c.prec = 50
        half = float(Decimal(0.263) * Decimal(float(star.params[i_numax])) ** Decimal(0.77) / 2)
    _pair(zoo, "Gaussian width at the Stello bound x (1 -+ 1e-6)", "Gaussian width under the Stello bound", i_sig, half * (1 - EPS), half * (1 + EPS))
    if star.prior_class == 0:
        _pair(zoo, "a1 negative", "negative a1 or a2", 5, NEG0, 0.0)
        _pair(zoo, "a2 negative", "negative a1 or a2", 6, NEG0, 0.0)
        numax = star.params[15]
        _pair(zoo, "numax + mu_numax just under 0", "numax + mu_numax < 0", 17, -_above(numax), -numax)


_CACHE = {}
ZOO_NAMES = ("zoo_global", "zoo_small", "zoo_small2", "zoo_large", "zoo_local", "zoo_local_a1", "zoo_hnlm", "zoo_v2", "zoo_rgb", "zoo_env0",
             "zoo_env1")


def zoo(synth):
    """All the stars with their cases; built once per process (the reference is evaluated to pick the inside vectors)."""
    if "zoo" in _CACHE:
        return _CACHE["zoo"]
    import prior_reference as ref
    out = {}

    def new(name, star):
        out[name] = Zoo(name, star)
        return out[name]

    _fill_global(new("zoo_global", make_zoo_global(synth)), ref, aj=True)
    _fill_global(new("zoo_small", make_zoo_global(synth, nmax=3, lmax=1)), ref, aj=True)
    _fill_global(new("zoo_small2", make_zoo_global(synth, nmax=3, lmax=2)), ref, aj=True)
    _fill_global(new("zoo_large", make_zoo_global(synth, nmax=24, lmax=3, step=1.75)), ref, aj=True)
    _fill_local(new("zoo_local", make_zoo_local(synth)), ref, "sqrt")
    _fill_local(new("zoo_local_a1", make_zoo_local_a1(synth)), ref, "a1")
    _fill_local(new("zoo_hnlm", make_zoo_hnlm(synth)), ref, "a1")
    out["zoo_hnlm"].spectrum_of = synth.make_c2_star(nx=NX)                    # (the local star the Hnlm one was converted from)
    _fill_v2(new("zoo_v2", make_zoo_v2(synth)), ref)
    out["zoo_v2"].spectrum_of = synth.make_classic_star(nx=NX, step=1.0)       # (the Classic star the v2 one was converted from)
    _fill_rgb(new("zoo_rgb", make_zoo_rgb(synth)), ref)
    _fill_env(new("zoo_env0", make_zoo_env(synth, 0)), ref)
    _fill_env(new("zoo_env1", make_zoo_env(synth, 1)), ref)
    assert tuple(out) == ZOO_NAMES
    _CACHE["zoo"] = out
    return out


def references(synth):
    """{name: [Result per case]} of the exact reference, and the same of its float64 restatement; computed once per process and shared."""
    if "ref" not in _CACHE:
        import prior_reference as ref
        z = zoo(synth)
        _CACHE["ref"] = {n: [ref.star_log_prior(v.star, c.params) for c in v.cases] for n, v in z.items()}
        _CACHE["f64"] = {n: [ref.star_log_prior(v.star, c.params, exact=False) for c in v.cases] for n, v in z.items()}
    return _CACHE["ref"], _CACHE["f64"]


def measured_r(synth):
    """Largest |float64 restatement - reference| / (2^-52 scale) over every case with a finite prior."""
    ex, f64 = references(synth)
    r = 0.0
    for n in ex:
        for a, b in zip(ex[n], f64[n]):
            if a.failed is None:
                r = max(r, float(abs(_dec(b.value) - a.value) / (_dec(2.0 ** -52) * a.scale)))
    return r


def _dec(v):
    from decimal import Decimal
    return Decimal(float(v))


def device_K(synth):
    """K of tol_prior = K 2^-52 scale: four times the measured cost of double arithmetic on these cases, and at least 4 (a different
    summation order; device log / sqrt at 1-2 ulp where libm is at 0.5)."""
    if "K" not in _CACHE:
        _CACHE["r"] = measured_r(synth)
        _CACHE["K"] = max(4.0, 4.0 * _CACHE["r"])
    return _CACHE["K"]


def tol_prior(result, K):
    return K * 2.0 ** -52 * float(result.scale)


def bracket(result, tol):
    """The doubles a value within `tol` (a Decimal) of the reference can round to: [lo, hi], both ends correctly rounded."""
    return float(result.value - tol), float(result.value + tol)


def existing_gpu_test_vectors(synth):
    """The six vectors of tests/test_gpu_c1_real_data.py::test_device_priors_match_host (the prior does not depend on the grid)."""
    star = synth.make_c3_star(nx=NX, step=1.0)
    rng = np.random.default_rng(8)
    idx = star.index_to_relax
    P = np.tile(star.params, (6, 1))
    P[1:, idx] *= 1 + 0.01 * rng.standard_normal((5, idx.size))
    P[5, idx[3]] = -5.0
    return star, P

"""Small cases for the exact checks of the adjoint gradient (test_adjoint_exact.py on the CPU, test_gpu_adjoint_exact.py on the GPU).

A case is a star (4700 bins at most), three chains (T = 1, 1.3, 2.2, p = 2; rows 1 and 2 perturbed by 0.3 % in the star's own free
parameters), an index_to_relax -- the star's own free parameters PLUS the asymmetry parameter and every noise parameter, so that G[row][15]
and every Gn[j] is contracted -- and one set of steps.  check(pkg) asserts, from the host table builder alone, the properties the case is
there for (row count, windows, asymmetry on / off, ...).

  corner / corner_neg     adjoint_numpy.corner_star (16 rows, windows of 50 .. 548 bins, l = 3 rows, a Harvey term with tau = 0), asymmetry
                          +15 / -15; corner_neg with NEGATIVE steps
  corner_negnoise         corner with a negative Harvey height and a negative white-noise parameter in the vector (the builders store |.|)
  rows64 / rows68 / rows132 (+ _asym)   make_c3_star tables of 64, 68 and 132 rows: one full lane pass of k_adj_contract, one pass and four
                          rows, two passes and four rows; asymmetry 0 (the asymmetry component's likelihood share must be exactly 0: the
                          header's rule "no derivative at asym = 0") and 15.  rows68_asym with LARGE steps (2e-3 relative): perturbed rows
                          whose window [i0, i1) is not the base row's, which the contraction must not read
  id3 / id11 / id12 / id13 / id14   one star per further table id with a device builder
"""
import numpy as np

import adjoint_numpy as an

TEMPS = np.array([1.0, 1.3, 2.2])
P_EXP = 2.0
ASYM_NAME = "Lorentzian_asymetry"


class Case:
    def __init__(self, name, star, asym_index, noise_index, steps="usual", rows=None, windows=None):
        self.name, self.star, self.asym_index, self.noise_index, self.step_kind = name, star, int(asym_index), list(noise_index), steps
        self.rows, self.windows = rows, windows
        self.idx = np.array(sorted(set(star.index_to_relax.tolist()) | {self.asym_index} | set(self.noise_index)), dtype=np.int32)
        self.k_asym = int(np.flatnonzero(self.idx == self.asym_index)[0])
        self.P = np.tile(star.params, (3, 1))
        own = star.index_to_relax
        self.P[1:, own] *= 1 + 0.003 * np.random.default_rng(5).standard_normal((2, own.size))
        rel = {"usual": 1e-6, "negative": -1e-6, "large": 2e-3}[steps]
        self.h = rel * np.maximum(np.abs(star.params[self.idx]), 1e-2)
        self.asym = float(star.params[self.asym_index])

    def check(self, pkg):
        """The case's own properties, from the host builder (every chain's base table)."""
        s = self.star
        for ch in range(3):
            st, m, nz, nh = pkg.build_mode_table(s.model_id, self.P[ch], s.plength, s.x)
            assert st == 0, (self.name, ch, st)
            assert self.rows is None or m.size == self.rows, (self.name, m.size)
            n = np.minimum(m["i1"], s.x.size) - np.maximum(m["i0"], 0)
            if ch == 0 and self.windows is not None:
                assert (n.min(), n.max()) == self.windows, (self.name, n.min(), n.max())
            assert np.all(m["asym"] == self.asym), self.name
            assert np.all(nz >= 0) and nz.size == int(s.plength[8])
            assert np.array_equal(nz, np.abs(self.P[ch][self.noise_index]))
        assert s.x.size <= 4700 and self.idx.size > s.index_to_relax.size
        return m

    def unread(self, pkg):
        """[3 x Nvars] bool: components whose parameter the model never reads -- the host builder's table at theta + h e_k is the base
        table, byte for byte (ids 13 and 14 count every degree's height offset from the start of the block, include/tamcmc_hip.h, which
        leaves some heights unread)."""
        s = self.star
        out = np.zeros((3, self.idx.size), dtype=bool)
        for ch in range(3):
            _, m0, nz0, _ = pkg.build_mode_table(s.model_id, self.P[ch], s.plength, s.x)
            for k, ip in enumerate(self.idx):
                v = self.P[ch].copy()
                v[ip] += self.h[k]
                st, m, nz, _ = pkg.build_mode_table(s.model_id, v, s.plength, s.x)
                out[ch, k] = st == 0 and m.tobytes() == m0.tobytes() and nz.tobytes() == nz0.tobytes()
        return out


def _indices(star, names=None):
    names = star.names if names is None else names
    return names.index(ASYM_NAME), [i for i, nm in enumerate(names) if nm.startswith("Harvey-Noise") or nm == "White_Noise_N0"]


def _with_asym(star, value, names=None):
    ia, noise = _indices(star, names)
    star.params[ia] = value
    return star, ia, noise


def _c3(synth, nmax, nx, fmin):
    return synth.make_c3_star(nx=nx, step=1.0, nmax=nmax, fmin=fmin)


def _id13(synth):
    """The small Classic star with a Classic_v3 height block, every height free (as test_gpu_hnlm._fd_star; likelihood only: no priors)."""
    c3 = synth.make_classic_star(nx=4000, step=1.0, nmax=4, fmin=2300.0)
    ia, noise = _indices(c3)                       # (both lie in front of the inclination: the same places in the v3 vector)
    c3.params[ia] = 15.0
    p13, pl13 = synth.classic_to_v3(c3.params, c3.plength)
    o = int(c3.plength[:9].sum())
    relax = np.r_[c3.relax[:o], np.ones(pl13[9], dtype=np.int32), c3.relax[o + 1:]]
    return synth.Star(13, p13, pl13, c3.x, relax, np.zeros((4, p13.size)), np.zeros(p13.size), None, 0), ia, noise


def _negnoise(synth):
    s, ia, noise = _with_asym(an.corner_star(synth), 15.0)
    s.params[noise[0]] *= -1.0      # first Harvey height
    s.params[noise[-1]] *= -1.0     # white noise
    assert s.params[noise[0]] < 0 and s.params[noise[-1]] < 0
    return s, ia, noise


# nmax, nx, fmin -> rows, (shortest, longest window) of the star's own table: 17 .. 1408 bins over the three
ROWS = {"rows64": (16, 2600, 1000.0, 64, (41, 477)), "rows68": (17, 2600, 1000.0, 68, (17, 718)), "rows132": (33, 4700, 400.0, 132, (23, 1408))}

NAMES = ["corner", "corner_neg", "corner_negnoise", "rows64", "rows64_asym", "rows68", "rows68_asym", "rows132", "rows132_asym",
         "id3", "id11", "id12", "id13", "id14"]
FIELD_CASES = ["corner", "corner_neg"]

_CACHE = {}


def case(synth, name):
    """The case `name`, built once per process."""
    if name in _CACHE:
        return _CACHE[name]
    kw = {}
    if name == "corner":
        args = _with_asym(an.corner_star(synth), 15.0)
        kw = dict(rows=16, windows=(50, 548))
    elif name == "corner_neg":
        args = _with_asym(an.corner_star(synth), -15.0)
        kw = dict(rows=16, windows=(50, 548), steps="negative")
    elif name == "corner_negnoise":
        args = _negnoise(synth)
        kw = dict(rows=16)
    elif name.split("_")[0] in ROWS:
        nmax, nx, fmin, rows, win = ROWS[name.split("_")[0]]
        args = _with_asym(_c3(synth, nmax, nx, fmin), 15.0 if name.endswith("_asym") else 0.0)
        kw = dict(rows=rows, windows=win, steps="large" if name == "rows68_asym" else "usual")
    elif name == "id3":
        args = _with_asym(synth.make_classic_star(nx=4000, step=1.0, nmax=4, fmin=2300.0), 15.0)
    elif name == "id11":
        args = _with_asym(synth.make_c2_star(nx=4000), 15.0)
    elif name == "id12":
        args = _with_asym(synth.make_v2_star(nx=4000, step=1.0, nmax=4, fmin=2300.0), 0.0)
    elif name == "id13":
        args = _id13(synth)
    elif name == "id14":
        args = _with_asym(synth.make_hnlm_star(nx=4000), 0.0)
    else:
        raise KeyError(name)
    _CACHE[name] = Case(name, *args, **kw)
    return _CACHE[name]


_SPEC = {}


def spectrum(pkg, c):
    """y of the case: the host table's model row (strict_numpy.eval_table) times Exp(1) noise, once per process."""
    import strict_numpy
    if c.name not in _SPEC:
        s = c.star
        st, m, nz, nh = pkg.build_mode_table(s.model_id, s.params, s.plength, s.x)
        assert st == 0
        _SPEC[c.name] = np.array(s.set_spectrum_from_model(strict_numpy.eval_table(m, nz, nh, s.x), 1))
    return _SPEC[c.name]

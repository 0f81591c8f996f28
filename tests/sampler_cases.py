"""Stars, sizes and directed proposal laws of tests/test_gpu_sampler_reference.py, and the exact factors they share.

Sizes -- each a boundary of the sampler's kernels (dev_iterate_impl.h::adapt_chain_as, dev_mala_impl.h::k_mala_test):
    3            fewer columns than one panel of the blocked factorisation (8)
    8 / 9        one panel exactly / a remainder of one
    21           two panels and a remainder of five; every free variable of the local slice
    63 / 64 / 65 the second register row of the one-wave triangular solve (lane i holds rows i and i + 64)
    93           the headline shape's count
    128 / 129    the last size of the one-wave solve / the column-loop solve with the adaptation's work matrix still in LDS
    153          work matrix in device memory: column-by-column factorisation, no panels
Stars: up to 21 free variables the local slice (C2 family), the larger ones the global fit with 24 radial orders (153 free); variables
beyond the wanted count are frozen (prior switch 0 = Fix), as tests/test_gpu_sampler.py::test_learning_factor_at_every_panel_remainder
does.  The grids are as short as the models allow: the algebra under test does not depend on them.

Laws -- Sigma = D R D with D the star's default errors, one of them shrunk to 3e-5 (eps2 = 1e-12 is then 1e-3 of that variance: a wrong
or missing eps2 term is 1e-3 of a pivot, of a drift component and of a density), and R
    "identity"   the identity
    "ar1"        AR(1), rho = 0.9: every element of the factor is populated
    "pairs"      the identity except rho = 0.999 between variables 7|8 and, where they exist, 63|64 and 127|128: the pairs straddle the
                 panel edge and the register rows of the solve, and the second pivot of each is 2e-3 of its variance
"""
import numpy as np

import sampler_reference as R

SIZES = (3, 8, 9, 21, 63, 64, 65, 93, 128, 129, 153)
NCH, LAM, EPS2 = 3, 1.5, 1e-12
LAWS = ("identity", "ar1", "pairs")
SMALL_ERROR = 3e-5
# test_langevin_test: sigma_m = SIGMA_FACTOR x the sampler's initial value.  With the default errors and the short spectra of these stars
# the initial steps are small against the posterior: ln r ~ +-0.01 with either sign, and half of the moves have r = 1.  At 20 x sigma
# two thirds of them have 1e-6 < r < 1 (measured on the host engine: 12-17 of 18 chain-iterations per case at Nv >= 63).
SIGMA_FACTOR = 20.0


def build_star(oracle, synth, nv):
    if nv <= 21:
        star = synth.make_c2_star(nx=1500)
    else:
        star = synth.make_c3_star(seed=7, nx=6000, nmax=24, lmax=3, step=0.6, fmin=15 * 135.1 - 80.0)
    _, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    star.set_spectrum_from_model(m0, 1000 + nv)
    for i in star.index_to_relax[nv:]:
        star.relax[i] = 0
        star.priors_switch[i] = 0
        star.priors[:, i] = -9999.0
    assert star.nvars == nv
    return star


def small_index(nv):
    """The variable whose error is shrunk: a member of the 7|8 pair where there is one."""
    return 8 if nv > 8 else nv - 1


def law(name, errors):
    nv = errors.size
    D = np.array(errors, dtype=np.float64, copy=True)
    D[small_index(nv)] = SMALL_ERROR
    if name == "identity":
        Rm = np.eye(nv)
    elif name == "ar1":
        k = np.arange(nv)
        Rm = 0.9 ** np.abs(k[:, None] - k[None, :])
    elif name == "pairs":
        Rm = np.eye(nv)
        for a in (7, 63, 127):
            if a + 1 < nv:
                Rm[a, a + 1] = Rm[a + 1, a] = 0.999
    else:
        raise KeyError(name)
    cov = Rm * np.outer(D, D)
    return (cov + cov.T) / 2


_factors = {}


def exact_factor(A):
    """(L, L rounded to double, |L^-1|) of the double matrix A, or None: computed once per matrix and shared by the tests."""
    key = A.tobytes()
    if key not in _factors:
        L = R.cholesky(A)
        if L is None:
            _factors[key] = None
        else:
            Lf = R.factor_float(L)
            _factors[key] = (L, Lf, R.abs_inverse(Lf))
    return _factors[key]


_normals = {}


def normals(seed, chain, iteration, nv):
    key = (seed, chain, iteration, nv)
    if key not in _normals:
        _normals[key] = R.normals(seed, chain, iteration, nv)
    return _normals[key]

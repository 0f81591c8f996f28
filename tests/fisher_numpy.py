"""numpy yardstick of the expected (Fisher) information (test helper; uses no device code).

  F_jk = sum_i (d_j M_i)(d_k M_i) / M0_i^2   (T = 1, p = 1)

with the derivative of tamcmc_hip_fisher: the central difference of the model rows at theta +- h_k e_k, both perturbed tables keeping the
BASE table's windows [i0, i1) (frozen window).  Tables come from the host builder (adjoint_numpy.tables), model rows from
strict_numpy.eval_table; U_k,i = (M+_k,i - M-_k,i) / (h_applied,k M0_i), F = U U^T with the products summed in long double.
"""
import numpy as np

import adjoint_numpy as an
import strict_numpy

LD = np.longdouble


def frozen_rows(pkg, star, params, base=None):
    """(model row, table) of `params` with the windows of table `base` (None: its own)."""
    m, nz, nh = an.tables(pkg, star.model_id, params, star.plength, star.x)
    if base is not None:
        assert m.size == base.size
        m["i0"], m["i1"] = base["i0"], base["i1"]
    return strict_numpy.eval_table(m, nz, nh, star.x), m


def fisher_central(pkg, star, h, params=None):
    """(F [Nv x Nv], U [Nv x Nx], h_applied [Nv]) at `params` (default: the star's own vector) with steps h."""
    P0 = np.array(star.params if params is None else params, dtype=np.float64)
    idx = np.asarray(star.index_to_relax)
    M0, base = frozen_rows(pkg, star, P0)
    U, happ = np.zeros((idx.size, star.x.size)), np.zeros(idx.size)
    for k, ip in enumerate(idx):
        Pp, Pm = P0.copy(), P0.copy()
        Pp[ip] = P0[ip] + h[k]
        Pm[ip] = P0[ip] + (-h[k])
        happ[k] = Pp[ip] - Pm[ip]          # the difference of the two perturbed doubles as stored
        Mp, _ = frozen_rows(pkg, star, Pp, base)
        Mm, _ = frozen_rows(pkg, star, Pm, base)
        U[k] = (Mp - Mm) / (happ[k] * M0)
    UL = U.astype(LD)
    F = np.array([[float(np.sum(UL[j] * UL[k])) for k in range(idx.size)] for j in range(idx.size)])
    return F, U, happ


def bound(U, h_applied, Nx):
    """B_jk = eps_k ||U_j||_1 + eps_j ||U_k||_1 + Nx eps_j eps_k, eps_k = 2e-12 / |h_applied,k|: the FAST tolerance of a model row
    (|dM| / M <= 1e-12 per bin, include/tamcmc_hip.h) carried through the difference of two rows (2e-12 M0 / (|h| M0) per element of U) and
    the product U_j U_k."""
    eps = 2e-12 / np.abs(h_applied)
    n1 = np.sum(np.abs(U), axis=1)
    return eps[None, :] * n1[:, None] + eps[:, None] * n1[None, :] + Nx * eps[:, None] * eps[None, :]


def scale(F):
    """sqrt(F_jj F_kk), 1 where a variable carries no information."""
    d = np.sqrt(np.diag(F))
    d = np.where(d > 0, d, 1.0)
    return d[:, None] * d[None, :]


_CACHE = {}


def cached(pkg, oracle, synth, name):
    """(star, y, F, U, h_applied, h) of the named star at its own parameters and h = adjoint_numpy.steps, computed once per process."""
    if name not in _CACHE:
        star = an.corner_star(synth) if name == "corner" else an.stars(synth)[name]
        y = an.spectrum(oracle, star)
        h = an.steps(star.params, star.index_to_relax)
        F, U, happ = fisher_central(pkg, star, h)
        _CACHE[name] = (star, y, F, U, happ, h)
    return _CACHE[name]

"""The yardstick of the adjoint gradient, on the CPU (tests/adjoint_numpy.py; no code under test beyond the host table builder, whose
tables are the oracle's bit for bit): the numpy adjoint -- table-space sums contracted with the forward table Jacobian -- against the
central difference with frozen windows, within 3 R of it, R = max_k |g(h) - g(h/2)| that reference's own uncertainty.

Measured (of the gradient's scale): R 5.1e-7 / 7.5e-7 / 9.9e-6, distance 6.8e-7 / 1.0e-6 / 1.3e-5 for the C2, C3-with-asymmetry and Classic
stars: 1.33 R each -- g(h) - g(h/2) is 3/4 of the central difference's own O(h^2) term, so the distance IS that term -- whatever the
Jacobian's step (1e-6, 5e-7, 1e-7)."""
import numpy as np
import pytest

import adjoint_numpy as an


@pytest.mark.parametrize("name", ["c2", "c3_asym", "classic"])
def test_numpy_adjoint_matches_the_frozen_central_difference(pkg, oracle, synth, name):
    star, y, g_ref, R = an.cached_reference(pkg, oracle, synth, name)
    idx = star.index_to_relax
    scale = np.max(np.abs(g_ref))
    assert R < 1e-4 * scale
    for rel in (1e-6, 1e-7):
        g = an.adjoint_gradient(pkg, star.model_id, star.params, star.plength, idx, an.steps(star.params, idx, rel), star.x, y)
        d = np.max(np.abs(g - g_ref))
        print("\n%s: R %.2e, distance %.2e of scale (%.2f R) at Jacobian step %.0e" % (name, R / scale, d / scale, d / R, rel))
        assert d <= 3 * R


def test_corner_table_has_the_corners(pkg, synth):
    s = an.corner_star(synth)
    m, nz, nh = an.tables(pkg, s.model_id, s.params, s.plength, s.x)
    n = m["i1"] - m["i0"]
    assert n.min() < 256 < n.max() and (m["i0"] == 0).sum() >= 2 and (m["l"] == 3).sum() == 4 and np.all(m["asym"] != 0)
    assert nh == 2 and nz[4] == 0.0 and nz[1] != 0.0 and s.x.size % 512 != 0
    # a clamped row: its window starts at the first bin although its lowest component lies below the spectrum's edge or within reach of it
    assert np.any((m["i0"] == 0) & (m["nu"][:, 0] - s.x[0] < 0.5 * n))

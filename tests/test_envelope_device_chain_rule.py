"""The chain rule the device-resident Langevin step of the Gaussian-envelope fits runs (ids 0, 1; TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN;
k_env_mala_chain, csrc/dev_mala_impl.h), without a GPU.

env_grad_rows, env_row_jacobian and env_chain_contract of csrc/envelope_row.h are one text for two arithmetics: long double on the host
(the gradient entries; tests/test_envelope_gradient.py and the bitwise GPU tests hold that instantiation) and DOUBLE on the device.  Here
the double instantiation is compiled with g++ (tests/envelope_chain_rule_driver.cpp through tests/envelope_chain_rule.py) and fed the folded sums the kernels leave -- formed
in long double from the pieces of tests/envelope_grad_numpy.py in the layout of csrc/envelope_row.h and rounded to double, which is what
k_env_grad_fold hands on.  The gradient it assembles is held to the 50-digit derivative of S (tests/envelope_grad_reference.py) by the
header's gate, |d dS/dtheta_j| <= B_j (include/tamcmc_hip.h), at Nx = 2, 700, 1100 for both ids on the three vectors of
tests/test_gpu_envelope_gradient.py (the star's, a perturbed one, one with signs flipped; id 0 with mu_numax != 0), and on the vectors
with switched-off Harvey terms and zero exponents.  A parameter the model does not read gives exactly 0; the tc of a switched-off term
has no finite component.  The worst ratio per case is printed.

Fails on a tree without the feature: envelope_row.h has no double instantiation (the driver does not compile)."""
import mpmath as mp
import numpy as np
import pytest

import envelope_chain_rule as cr
import envelope_grad_numpy as gn
import envelope_grad_reference as gr
from test_gpu_envelope_gradient import _star, _vectors

LD = np.longdouble


def folded_sums(model_id, params, x, y):
    """(h, tile sums [16], xi sums [12]) as doubles, in the layout of csrc/envelope_row.h:
    tile  [sum r G, sum r G d, sum r G d^2, sum r, sum r L_q (NQ), sum r D_q (NQ), sum r D_q u_q (NQ); id 0: sum r L_k^2 (3)]
    xi    (id 0) [sum w L_k, sum w D_k, sum w D_k u_k, sum w L_k^2] (3 each)."""
    p, xl, yl = gn._ld(params), gn._ld(x), gn._ld(y)
    M, dM, _ = gn.row_derivatives(model_id, params, x)
    r = LD(1) / M - yl / (M * M)
    with np.errstate(divide="ignore"):
        lx = np.log(xl)
    raw, kraw = np.zeros(16, dtype=LD), np.zeros(12, dtype=LD)
    nu = p[8] if model_id == 1 else np.abs(p[15])
    d = xl - nu
    G = dM[0]                                   # g (id 1) / eta^2 g (id 0)
    raw[0], raw[1], raw[2], raw[3] = np.sum(r * G), np.sum(r * G * d), np.sum(r * G * d * d), np.sum(r)
    if model_id == 1:
        for q in range(2):
            tc, pw = np.abs(p[3 * q + 1]), np.abs(p[3 * q + 2])
            if tc == 0:
                continue
            u = np.log(LD(1e-3) * tc) + lx
            L, D = gn._logistic(pw, u)
            D0, Du = gn._guard(D, u)
            raw[4 + q], raw[6 + q], raw[8 + q] = np.sum(r * L), np.sum(r * D0), np.sum(r * Du)
    else:
        w = np.ones(xl.size, dtype=LD)
        w[0] = w[-1] = LD(0.5)
        nm = np.abs(p[15]) + p[17]
        for k, (i, j, ic) in enumerate(((2, 3, 4), (7, 8, 9), (10, 11, 12))):
            u = lx - (np.log(np.abs(p[i])) + p[j] * np.log(np.abs(nm)))
            L, D = gn._logistic(np.abs(p[ic]), u)
            D0, Du = gn._guard(D, u)
            raw[4 + k], raw[7 + k], raw[10 + k], raw[13 + k] = np.sum(r * L), np.sum(r * D0), np.sum(r * Du), np.sum(r * L * L)
            kraw[k], kraw[3 + k], kraw[6 + k], kraw[9 + k] = np.sum(w * L), np.sum(w * D0), np.sum(w * Du), np.sum(w * L * L)
    return float(x[1] - x[0]), raw.astype(np.float64), kraw.astype(np.float64)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = cr.build(tmp_path_factory.mktemp("envchain"))

    def run(model_id, P, x, y):
        """dS/dtheta [C x Np] (float64; not finite where the chain rule has no finite value) of the double chain rule."""
        sums = [folded_sums(model_id, p, x, y) for p in P]
        G, _, _ = cr.run(exe, "d", model_id, P, sums[0][0], [s[1] for s in sums], [s[2] for s in sums])
        return G.astype(np.float64)

    return run


def _gate(tag, model_id, P, x, y, got, undefined=()):
    worst = 0.0
    S = gr.EnvelopeS(model_id, x, y)
    for c, p in enumerate(P):
        ref = S.gradient(p)
        _, B, _ = gn.gradient_and_budget(model_id, p, x, y)
        for j, want in enumerate(ref):
            if want is None or (c, j) in undefined:
                assert not np.isfinite(got[c, j]), (tag, c, j, got[c, j])
                continue
            if B[j] == 0:
                assert got[c, j] == 0.0 and not np.signbit(got[c, j]), (tag, c, j, got[c, j])    # not read by the model: exactly +0
                continue
            ratio = float(abs(mp.mpf(float(got[c, j])) - want) / mp.mpf(float(B[j])))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (tag, c, j, got[c, j], float(want), ratio)
    print("\n%s: double chain rule, worst |d dS/dtheta_j| / B_j = %.3e" % (tag, worst))
    return worst


@pytest.mark.parametrize("model_id", [0, 1])
@pytest.mark.parametrize("nx", [2, 700, 1100])
def test_double_chain_rule_within_budget_of_the_50_digit_derivative(synth, driver, model_id, nx):
    star = _star(synth, model_id, nx, seed=70 + model_id)
    P = _vectors(star, seed=nx)
    assert np.any(P[2] < 0) and (model_id == 1 or P[1, 17] != 0)
    got = driver(model_id, P, star.x, star.y)
    assert got.shape == (3, 10 if model_id == 1 else 19)
    if model_id == 0:
        assert np.all(got[:, 18] == 0.0)
    _gate("id %d nx %d" % (model_id, nx), model_id, P, star.x, star.y, got)


def test_inactive_harvey_terms_and_zero_exponents(synth, driver):
    """The vectors of tests/test_gpu_envelope_gradient.py's test of the same name: a switched-off term leaves exactly 0 for its H and its
    exponent, and nothing finite for its tc (0 x 1/0; the Langevin step maps it to 0, as mala_gradient does with every such value)."""
    star = _star(synth, 1, 700, seed=21)
    P = np.tile(star.params, (3, 1))
    P[0, 4] = 0.0
    P[1, 1] = 0.0
    P[2, [2, 5]] = 0.0
    got = driver(1, P, star.x, star.y)
    assert got[0, 3] == 0.0 and got[0, 5] == 0.0 and got[1, 0] == 0.0 and got[1, 2] == 0.0
    _gate("id 1 inactive terms, zero exponents", 1, P, star.x, star.y, got, undefined={(0, 4), (1, 1)})

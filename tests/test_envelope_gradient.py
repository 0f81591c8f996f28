"""The analytic gradient of the Gaussian-envelope fits (ids 0, 1; TAMCMC_OPT_ENVELOPE_GRADIENT), without a GPU.

1. env_row_jacobian (csrc/envelope_row.h, the host's chain rule from row quantities to parameters) through a plain C++ driver
   (tests/envelope_jacobian_driver.cpp, g++ and libm, long double) against the 50-digit Jacobian of the row quantities
   (tests/envelope_grad_reference.py): the vectors of tests/test_envelope_row.py (synthetic stars, perturbed, negated, tc = 0, zero
   exponents) and mu_numax != 0.  Tolerance K 2^-64 |ref| with K = 8: the worst entry, d a_0^2/d p1 = p0^2 nu^(2 p1) 2 ln nu, passes a
   powl and a logl (1 ulp each) and four products (1/2 ulp each), 4 ulps of the 64-bit significand; K doubles that.  The measured
   ratio is printed.  An entry the reference has as exactly 0 must be exactly 0; the tc of a switched-off term is not finite.
2. The long-double numpy yardstick (tests/envelope_grad_numpy.py) against the 50-digit derivative of S itself at Nx = 2, 700, 1100 for both
   ids: every component within 1e-3 of its budget B_j, so that the yardstick's own error does not count where it judges the device
   (long double carries 2^-64 against the 1e-12 the budget is made of; the ratio is printed).
3. The option number and the audit entry in the header and in the package.
These fail on a tree without the feature."""
import os
import re
import subprocess

import mpmath as mp
import numpy as np
import pytest

import envelope_grad_numpy as gn
import envelope_grad_reference as gr
import envelope_numpy as en
from test_envelope_row import _vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8.0
YARDSTICK = 1e-3   # share of B_j the yardstick may use: it judges the device above Nx = 1100, so its own error must not count there


def _mp_from_hex(word):
    """A C99 hex float (as printf %La writes it) as an exact mpf; inf / nan as floats."""
    w = word.strip().lower()
    if "inf" in w or "nan" in w:
        return float(w)
    m = re.fullmatch(r"([+-]?)0x([0-9a-f]+)(?:\.([0-9a-f]*))?p([+-]?\d+)", w)
    assert m, word
    sign, whole, frac, e = m.group(1), m.group(2), m.group(3) or "", int(m.group(4))
    v = mp.mpf(int(whole + frac, 16)) * mp.mpf(2) ** (e - 4 * len(frac))
    return -v if sign == "-" else v


def _jacobian_vectors(synth):
    out = _vectors(synth)
    p = synth.make_envelope_star(0, nx=64, seed=3).params
    for mu in (3.5, -7.25):
        q = p.copy()
        q[17] = mu
        out.append((0, q))
        out.append((0, -q * np.where(np.arange(q.size) == 17, -1.0, 1.0)))   # every sign flipped but mu's (numax + mu stays positive)
    return out


@pytest.fixture(scope="module")
def printed(synth, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("envjac") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "envelope_jacobian_driver.cpp")], check=True, capture_output=True, timeout=300)
    vec = _jacobian_vectors(synth)
    text = "".join("%d %d %s\n" % (mid, p.size, " ".join(float(v).hex() for v in p)) for mid, p in vec)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert out[0].startswith("C ") and len(out) == len(vec) + 1
    return [int(w) for w in out[0].split()[1:]], vec, [line.split()[1:] for line in out[1:]]


def test_layout_constants(printed):
    consts, _, _ = printed
    assert consts == [13, 9, 16, 10, 15]   # row quantities, xi sums, tile sums of id 0 / id 1, the option


def test_host_jacobian_matches_the_50_digit_jacobian(printed):
    _, vec, rows = printed
    worst, eps = 0.0, mp.mpf(2) ** -64
    seen = {"negated": False, "tc0": False, "pw0": False, "mu": False}
    for (mid, p), words in zip(vec, rows):
        n = p.size
        assert len(words) == 13 * n
        J = gr.row_jacobian(mid, p)
        seen["negated"] |= bool(p[0] < 0)
        seen["tc0"] |= mid == 1 and (p[1] == 0 or p[4] == 0)
        seen["pw0"] |= mid == 1 and p[2] == 0
        seen["mu"] |= mid == 0 and p[17] != 0
        for q in range(13):
            for j in range(n):
                got, want = _mp_from_hex(words[q * n + j]), J[q][j]
                if want is None:
                    assert isinstance(got, float) and not np.isfinite(got), (mid, q, j, got)
                elif want == 0:
                    assert got == 0, (mid, q, j, got)
                else:
                    ratio = float(abs(got - want) / (eps * abs(want)))
                    worst = max(worst, ratio)
                    assert ratio <= K, (mid, q, j, got, want, ratio)
    assert all(seen.values()), seen
    print("\nworst host Jacobian entry: %.2f x 2^-64 |ref| (K = %.0f)" % (worst, K))


def _case(synth, model_id, nx, seed):
    star = synth.make_envelope_star(model_id, nx=nx, seed=seed)
    rng = np.random.default_rng(seed + 1)
    p = star.params * (1.0 + 0.03 * rng.standard_normal(star.params.size))
    if model_id == 0:
        p[17] = 1.5
    star.set_spectrum_from_model(np.asarray(en.model(model_id, p, star.x), dtype=np.float64), seed=seed + 2)
    return p, star.x, star.y


@pytest.mark.parametrize("model_id", [0, 1])
@pytest.mark.parametrize("nx", [2, 700, 1100])
def test_yardstick_within_budget_of_the_50_digit_derivative(synth, model_id, nx):
    p, x, y = _case(synth, model_id, nx, seed=40 + nx % 7)
    flips = np.ones(p.size)
    flips[[0, 2, 7]] = -1.0 if model_id == 1 else 1.0     # id 1: H1, p1, Amax negative
    if model_id == 0:
        flips[[4, 13, 14, 16]] = -1.0                      # id 0: c_gran, N0, Amax, sigma negative
    worst = 0.0
    for q in (p, p * flips):
        ref = gr.EnvelopeS(model_id, x, y).gradient(q)
        grad, B, _ = gn.gradient_and_budget(model_id, q, x, y)
        for j, want in enumerate(ref):
            if model_id == 0 and j == 18:
                assert grad[j] == 0
                continue
            hi = float(grad[j])
            got = mp.mpf(hi) + mp.mpf(float(grad[j] - np.longdouble(hi)))
            ratio = float(abs(got - want) / mp.mpf(float(B[j])))
            worst = max(worst, ratio)
            assert ratio <= YARDSTICK, (model_id, nx, j, float(got), float(want), ratio)
    print("\nid %d nx %d: yardstick at %.2e of B_j" % (model_id, nx, worst))


def test_public_surface(pkg):
    hip_h = open(os.path.join(ROOT, "include", "tamcmc_hip.h")).read()
    assert re.search(r"#define\s+TAMCMC_OPT_ENVELOPE_GRADIENT\s+15\b", hip_h)
    assert pkg.OPT_ENVELOPE_GRADIENT == 15
    others = {int(m.group(1)) for m in re.finditer(r"#define\s+TAMCMC_OPT_(?!ENVELOPE_GRADIENT)\w+\s+(\d+)\b", hip_h)}
    assert 15 not in others
    assert re.search(r"#define\s+TAMCMC_ENVELOPE_GRAD_N\s+13\b", hip_h) and re.search(r"#define\s+TAMCMC_ENVELOPE_KSI_N\s+9\b", hip_h)
    assert "tamcmc_hip_envelope_gradient_sums(" in hip_h
    assert (pkg.ENVELOPE_GRAD_N, pkg.ENVELOPE_KSI_N) == (13, 9)
    assert hasattr(pkg.lib(), "tamcmc_hip_envelope_gradient_sums") and hasattr(pkg.HipContext, "envelope_gradient_sums")

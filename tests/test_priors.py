"""Log-prior parity (row a1 of SURVEY section 8: generate_model = prior -> model -> likelihood).
CPU: the product's host priors (csrc/priors_impl.h, long double) against the oracle restatement and against analytic
values; parity unpinned by the reference (its tests never evaluate a prior).

Further down: the host code and the oracle against tests/prior_reference.py (50-digit restatement of the reference's text, independent
of both) on the cases of tests/prior_cases.py -- every primitive id, every hard constraint, every prior class."""
from decimal import Decimal

import numpy as np
import pytest


def test_primitive_priors_known_answers(oracle):
    L = oracle.lib
    assert float(L.orc_logP_uniform(2.0, 6.0, 3.0)) == pytest.approx(-np.log(4.0), rel=1e-15)
    assert float(L.orc_logP_uniform(2.0, 6.0, 7.0)) == -np.inf
    assert float(L.orc_logP_uniform_abs(2.0, 6.0, -3.0)) == pytest.approx(-np.log(4.0), rel=1e-15)
    assert float(L.orc_logP_gaussian(1.0, 0.5, 1.7)) == pytest.approx(-np.log(np.sqrt(2 * np.pi) * 0.5) - 0.5 * (0.7 / 0.5) ** 2, rel=1e-14)
    # Jeffreys: (1/(h+hmin)) / ln((hmax+hmin)/hmin) on 0 < h < hmax
    assert float(L.orc_logP_jeffrey(1.0, 1e4, 12.0)) == pytest.approx(np.log((1 / 13.0) / np.log(10001.0)), rel=1e-14)
    assert float(L.orc_logP_jeffrey(1.0, 1e4, -1.0)) == -np.inf and float(L.orc_logP_jeffrey(1.0, 1e4, 2e4)) == -np.inf
    # GU: flat on [a,b], Gaussian tail below a; normalisation ln(|b-a| + sqrt(2 pi)/2 sigma)
    C = np.log(45.0 + 0.5 * np.sqrt(2 * np.pi) * 2.0)
    assert float(L.orc_logP_gaussian_uniform(0.0, 45.0, 2.0, 10.0)) == pytest.approx(-C, rel=1e-14)
    assert float(L.orc_logP_gaussian_uniform(0.0, 45.0, 2.0, -3.0)) == pytest.approx(-0.5 * 1.5 ** 2 - C, rel=1e-14)
    assert float(L.orc_logP_gaussian_uniform(0.0, 45.0, 2.0, 50.0)) == -np.inf


def test_host_priors_match_oracle(pkg, oracle, synth):
    from tamcmc_c_amd import sampler
    rng = np.random.default_rng(4)
    for star in (synth.make_c3_star(nx=2000, step=1.0), synth.make_c2_star(nx=1000)):
        idx = star.index_to_relax
        v0, st = sampler.log_prior(star)
        assert st == 0 and np.isfinite(v0)
        assert v0 == pytest.approx(oracle.call_prior(star), rel=1e-14)
        n_inf = 0
        for trial in range(200):
            p = star.params.copy()
            p[idx] *= 1.0 + 0.02 * rng.standard_normal(idx.size)
            if trial % 7 == 0:
                p[idx[rng.integers(idx.size)]] *= -1.0     # push something out of its support
            a, st = sampler.log_prior(star, p)
            b = oracle.call_prior(star, p)
            assert st == 0
            if np.isinf(b):
                assert a == b
                n_inf += 1
            else:
                assert a == pytest.approx(b, rel=1e-13, abs=1e-12)
        assert n_inf > 5


def test_smoothness_and_d02_terms(pkg, synth):
    """priors_MS_Global extras: second-difference smoothness of each degree's frequency list ~ N(0, scoef) and
    d02 ~ GU(0, Dnu/3, 0.015 Dnu) (priors_calc.cpp:281-313)."""
    from tamcmc_c_amd import sampler
    star = synth.make_c3_star(nx=2000, step=1.0)
    base, _ = sampler.log_prior(star)
    off = sampler.log_prior(_with_extra(star, 0, 0.0))[0]          # smoothness off
    nmax = int(star.plength[0])
    f = star.params[nmax + 3:nmax + 3 + 4 * nmax].reshape(4, nmax)
    d2 = np.zeros_like(f)
    d2[:, 1:-1] = f[:, 2:] - 2 * f[:, 1:-1] + f[:, :-2]
    d2[:, 0] = d2[:, 1]
    d2[:, -1] = d2[:, -2]
    want = np.sum(-np.log(np.sqrt(2 * np.pi) * 2.0) - 0.5 * (d2 / 2.0) ** 2)
    assert base - off == pytest.approx(want, rel=1e-12)


def _with_extra(star, i, v):
    import copy
    s = copy.copy(star)
    s.extra_priors = star.extra_priors.copy()
    s.extra_priors[i] = v
    return s


def test_asymptotic_priors_match_oracle(pkg, oracle, synth):
    """Prior class io_asymptotic (priors_asymptotic, priors_calc.cpp:319-512) for the red-giant model: product host code vs oracle,
    incl. the hard constraints and the smoothness terms (which the reference switches on the prior id of the first noise
    parameter -- kept, see csrc/priors_impl.h)."""
    from tamcmc_c_amd import sampler
    star = synth.make_c5_star(nx=2000, nmax=7)
    o = np.cumsum([0] + list(star.plength))
    rng = np.random.default_rng(3)
    base = star.params.copy()
    cases = [base]
    for _ in range(6):
        p = base.copy()
        p[star.index_to_relax] *= 1 + 1e-3 * rng.standard_normal(star.nvars)
        cases.append(p)
    bad = {"negative visibility": (o[1], -0.1), "a3/a1 over the limit": (o[6] + 4, 0.5), "negative Wfactor": (o[3] + 6, -0.2),
           "negative Hfactor": (o[3] + 7, -0.2), "negative width-law parameter": (o[7] + 2, -1.0), "outside a uniform prior": (o[3] + 3, 1.5)}
    for k, (idx, val) in bad.items():
        p = base.copy()
        p[idx] = val
        cases.append(p)
    got = np.array([sampler.log_prior(star, p)[0] for p in cases])
    ref = np.array([oracle.call_prior(star, p) for p in cases])
    assert np.all(np.isfinite(ref[:7])) and np.all(ref[7:] == -np.inf)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)) and np.allclose(got[:7], ref[:7], rtol=1e-14)
    # smoothness: active because the first noise parameter carries a Uniform prior (id 1); a kink in the l=0 ladder is penalised
    assert star.priors_switch[o[8]] == 1
    p = base.copy()
    p[o[2] + 3] += 0.4
    d = sampler.log_prior(star, p)[0] - got[0]
    sd = lambda y: np.array([y[2] - 2 * y[1] + y[0]] + list(y[2:] - 2 * y[1:-1] + y[:-2]) + [y[-1] - 2 * y[-2] + y[-3]])
    want = -0.5 * (np.sum(sd(p[o[2]:o[3]]) ** 2) - np.sum(sd(base[o[2]:o[3]]) ** 2)) / 2.0 ** 2
    assert np.isclose(d, want, rtol=1e-9)


# ---- parity with the 50-digit reference (tests/prior_reference.py) on the cases of tests/prior_cases.py ----
@pytest.fixture(scope="module")
def cases(synth):
    import prior_cases
    z = prior_cases.zoo(synth)
    ex, f64 = prior_cases.references(synth)
    return prior_cases, z, ex, f64


def test_reference_cases_are_what_they_claim(cases):
    """The reference alone: every "fail" case is rejected by the constraint it names, its twin and every "inside" vector are finite, no
    computed deciding quantity lies within 1e-9 (relative) of its threshold, and the cases reach what they were built to reach."""
    pc, z, ex, _ = cases
    for name, zoo in z.items():
        for c, r in zip(zoo.cases, ex[name]):
            assert r.near_threshold() >= 1e-9, (name, c.label, r.near_threshold())
            if c.kind == "fail":
                assert r.failed is not None and r.failed.startswith(c.expect), (name, c.label, r.failed)
            elif c.kind in ("pass", "inside"):
                assert r.failed is None, (name, c.label, r.failed)
        assert sum(c.kind == "inside" for c in zoo.cases) >= 20
    # every primitive id both inside and (where its support ends) outside
    seen = {}
    for name, zoo in z.items():
        for r in ex[name]:
            for nm, t in zip(r.names, r.terms):
                if nm.startswith("id "):
                    seen.setdefault(int(nm.split()[1]), set()).add(bool(t == r.A.ninf))
    assert seen == {1: {False, True}, 2: {False}, 4: {False, True}, 5: {False, True}, 6: {False, True}, 7: {False}, 8: {False, True},
                    10: {False, True}}
    # the lane partitions: fewer than 64 additive terms without d02 terms (Nfl0 != Nfl2) and lmax < 3; more than 256
    def n_terms(zoo):  # the count the device loops over: Np generic terms + the d02 and smoothness ones
        pl, Np = zoo.star.plength, zoo.star.params.size
        extra = (pl[2] if pl[2] == pl[4] else 0) + sum(pl[2 + l] for l in range(pl[1] + 1))
        return Np + extra
    assert n_terms(z["zoo_small"]) < 64 and z["zoo_small"].star.plength[2] != z["zoo_small"].star.plength[4]
    assert z["zoo_small"].star.plength[1] == 1 and z["zoo_small2"].star.plength[1] == 2
    assert n_terms(z["zoo_large"]) > 256 and 128 < n_terms(z["zoo_global"]) < 256
    fails = {c.expect for zoo in z.values() for c in zoo.cases if c.kind == "fail"}
    for j in range(2, 7):
        assert "|a%d/a1| over its limit" % j in fails
    assert {"a1 < 0", "negative visibility", "noise check 1", "noise check 2", "noise check 3", "ratio sum l=1", "ratio sum l=2",
            "ratio sum l=3", "|a3/a1| over its limit (a1 fitted)", "|a3/a1| over its limit (sqrt(a1) cos i, sin i)", "negative inclination",
            "|a3/rot_env| over its limit", "negative width-law parameter", "negative Wfactor", "negative Hfactor",
            "Gaussian width under the Stello bound", "negative a1 or a2", "numax + mu_numax < 0"} <= fails


def _misses(what, name, zoo, refs, values):
    """Finiteness must agree exactly; a finite value must be a double that a number within 4 x 2^-63 x scale of the reference rounds to.
    (Both entries hand their long double back as a double.  The bound is the long double's, so it is applied before that rounding, not
    after: the value must lie between the correctly rounded ends of [reference - tol, reference + tol].)  Returns the cases outside."""
    out = []
    for c, r, got in zip(zoo.cases, refs, values):
        if r.failed is not None:
            assert got == -np.inf, (what, name, c.label, got, r.failed)
            continue
        assert np.isfinite(got), (what, name, c.label, got)
        tol = 4 * Decimal(2) ** -63 * r.scale
        lo, hi = float(r.value - tol), float(r.value + tol)
        if not lo <= got <= hi:
            mid = (Decimal(got) + Decimal(lo if got < lo else hi)) / 2   # the long double lay beyond this rounding boundary
            out.append((c.label, got, float(r.value), "at least %.2f tol off" % float(abs(mid - r.value) / tol)))
    return out


@pytest.mark.parametrize("name", __import__("prior_cases").ZOO_NAMES)
def test_host_priors_match_the_50_digit_reference(pkg, cases, name):
    """The host's sum carries the rounding of its additions along (pr::TermSum, csrc/priors_impl.h).  With plain left-to-right
    long-double additions one of the 836 finite vectors -- zoo_v2, "id 7 on parameter 14 (Visibility_l1): b_max + 30 sigma2", 174 terms
    at magnitudes up to 860 -- came out at least 2.27 tol from the exact sum: additions alone, which the bound does not budget for."""
    from tamcmc_c_amd import sampler
    pc, z, ex, _ = cases
    zoo = z[name]
    got = []
    for c in zoo.cases:
        v, st = sampler.log_prior(zoo.star, c.params)
        assert st == 0, (name, c.label, st)
        got.append(v)
    miss = _misses("host", name, zoo, ex[name], got)
    assert not miss, miss


def test_oracle_priors_match_the_50_digit_reference(oracle, cases):
    """Where the oracle implements the class and options: classes 2 (not the ratio sums of impose_normHnlm = 1), 3 and 4."""
    pc, z, ex, _ = cases
    n = 0
    for name, zoo in z.items():
        if zoo.star.prior_class not in (2, 3, 4) or (zoo.star.prior_class == 2 and int(zoo.star.extra_priors[8]) != 0):
            continue
        n += 1
        miss = _misses("oracle", name, zoo, ex[name], [oracle.call_prior(zoo.star, c.params) for c in zoo.cases])
        assert not miss, (name, miss)
    assert n == 8


def test_cost_of_double_arithmetic_sets_the_device_tolerance(synth, cases):
    """r = the largest |float64 restatement - reference| / (2^-52 scale) over all finite cases (7.26 when this was written: the 30-sigma
    Gaussian tails, terms of -450 summed left to right); K = max(4, 4 r) (29.0).  tol_prior = K 2^-52 scale must not be looser than
    what test_device_priors_match_host already asserts (rel 1e-13, abs 1e-11) on that test's vectors."""
    import prior_reference
    pc, z, ex, f64 = cases
    for name in z:
        for a, b in zip(ex[name], f64[name]):
            assert (a.failed is None) == (b.failed is None) and (a.failed is None or a.failed == b.failed)
    K = pc.device_K(synth)
    r = pc._CACHE["r"]
    print("\nr = %.3f, K = %.2f" % (r, K))
    assert 0.5 < r < 16 and K == max(4.0, 4 * r)
    star, P = pc.existing_gpu_test_vectors(synth)
    finite = 0
    for b in range(6):
        res = prior_reference.star_log_prior(star, P[b])
        if res.failed is None:   # (the others are compared for being -inf only, there as here)
            finite += 1
            assert pc.tol_prior(res, K) <= max(1e-13 * abs(float(res.value)), 1e-11)
    assert finite >= 1

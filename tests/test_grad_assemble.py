"""The one host assembly of a gradient batch (tamcmc-c_amd/csrc/grad_assemble.h: assemble_gradient, tempered_loglike) on the CPU: a
small C++ driver (tests/grad_assemble_driver.cpp, compiled with g++, and a second time with AddressSanitizer + UBSan as the stand-alone
program it is) runs it on the cases below; the rule is restated here in numpy longdouble and compared bit for bit.

Shape of every case: C = 2 chains x Nvars = 3 variables of Np = 5 parameters, T = (1, 2.5), p = 1.9 (call_likelihood truncates it to 1).
The restatement: logL = (double)((long double)(-(long)p) * S / T); the applied step is (x0 + h) - x0 in doubles; the likelihood's share
of component k is (logL_k - logL_0) / h_applied from full sums, logL(difference) / h_applied from base + differences, or the ready
derivative; with a prior a non-finite likelihood share counts as 0 and the prior's share is forward, else backward, else flat; a failed
slot is NaN and the first failed status in slot order is returned."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, NV, NP, E = 2, 3, 5, 4
B = C * E
T = np.array([1.0, 2.5])
P_LIKE = 1.9
IDX = [4, 0, 2]
FULL, DIFF, READY = 0, 1, 2
LD = np.longdouble


def build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "grad_assemble_driver.cpp")],
                   check=True, capture_output=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("grad_assemble")
    return [build(tmp, "driver", []), build(tmp, "driver_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def hexd(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64))


def unhex(line):
    return np.array([int(t, 16) for t in line.split()], dtype=np.uint64).view(np.float64)


def run(exe, case):
    share = case["share"]
    head = [C, NV, NP, share, repr(P_LIKE), int(case["lpp"] is not None), int(case["status"] is not None), int(case["want_pr0"]),
            int(case["want_gp"])]
    parts = [" ".join(str(v) for v in head), hexd(case["params"]), " ".join(str(i) for i in IDX), hexd(case["hstep"]), hexd(T), hexd(case["S"])]
    if share == READY:
        parts.append(hexd(case["dlogL"]))
    if case["lpp"] is not None:
        parts += [hexd(case["lpp"]), hexd(case["lpm"])]
    if case["status"] is not None:
        parts.append(" ".join(str(int(s)) for s in case["status"]))
    r = subprocess.run([exe], input="\n".join(parts) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    out = r.stdout.split("\n")
    return int(out[0]), unhex(out[1]), (None if out[2].strip() == "-" else unhex(out[2])), unhex(out[3]).reshape(C, NV), \
        (None if out[4].strip() == "-" else unhex(out[4]).reshape(C, NV))


def tempered(S, Tm):
    """call_likelihood on a sum: -(long)p * S in long double, / T, one rounding to double."""
    f = LD(np.float64(S))
    f = LD(-int(P_LIKE)) * f
    return np.float64(f / LD(Tm))


def restate(case):
    """(status, logL0, logPr0, grad, grad_prior) by the rule of the module docstring."""
    share, S, st, lpp, lpm = case["share"], case["S"], case["status"], case["lpp"], case["lpm"]
    logL0, logPr0 = np.zeros(C), np.zeros(C)
    grad, gprior = np.zeros((C, NV)), np.zeros((C, NV))
    first = 0
    with np.errstate(all="ignore"):
        for ch in range(C):
            def failed(e):
                nonlocal first
                s = 0 if (st is None or share == READY) else int(st[ch * E + e])
                if first == 0:
                    first = s
                return s != 0
            L0 = np.float64(np.nan) if failed(0) else tempered(S[ch * E] if share == FULL else S[ch], T[ch])
            logL0[ch] = L0
            pr0 = np.float64(lpp[ch * E]) if lpp is not None else np.float64(0.0)
            logPr0[ch] = pr0
            for k in range(NV):
                x0 = np.float64(case["params"][ch, IDX[k]])
                happ = np.float64(np.float64(x0 + np.float64(case["hstep"][k])) - x0)
                if share == READY:
                    g = np.float64(case["dlogL"][ch, k])
                elif failed(k + 1):
                    g = np.float64(np.nan)
                elif share == DIFF:
                    g = np.float64(tempered(S[C + ch * E + k + 1], T[ch]) / happ)
                else:
                    g = np.float64(np.float64(tempered(S[ch * E + k + 1], T[ch]) - L0) / happ)
                if lpp is not None:
                    if not np.isfinite(g):
                        g = np.float64(0.0)
                    prp, prm = np.float64(lpp[ch * E + k + 1]), np.float64(lpm[ch * E + k + 1])
                    if np.isfinite(prp):
                        gp = np.float64(np.float64(prp - pr0) / happ)
                    elif np.isfinite(prm):
                        gp = np.float64(np.float64(pr0 - prm) / happ)
                    else:
                        gp = np.float64(0.0)
                    g = np.float64(g + gp)
                    gprior[ch, k] = gp
                grad[ch, k] = g
    return first, logL0, logPr0, grad, gprior


def make_cases():
    rng = np.random.default_rng(20261020)
    params = rng.normal(0.0, 30.0, (C, NP))
    hstep = np.array([1e-7 * abs(params[0, 4]), -3e-6, 2.0 ** -20])   # (x0 + h) - x0 is not h for the first two
    S_full = 1.0e4 + rng.normal(0.0, 1.0, B)
    S_diff = np.concatenate([S_full[::E], rng.normal(0.0, 1e-3, B)])
    dlogL = rng.normal(0.0, 50.0, (C, NV))
    lpp = -5.0 + rng.normal(0.0, 0.1, B)
    lpm = -5.0 + rng.normal(0.0, 0.1, B)
    ninf = -np.inf
    # chain 0: forward finite / forward -inf, backward finite / -inf at both; chain 1: the same rules on other components
    lpp_mix, lpm_mix = lpp.copy(), lpm.copy()
    lpp_mix[0 * E + 2] = ninf
    lpp_mix[0 * E + 3] = ninf; lpm_mix[0 * E + 3] = ninf
    lpp_mix[1 * E + 1] = ninf; lpm_mix[1 * E + 1] = ninf
    lpp_mix[1 * E + 3] = ninf
    st_base = np.zeros(B, dtype=np.int32); st_base[0 * E + 0] = -5; st_base[1 * E + 2] = -4    # a base slot, then a perturbed one
    st_pert = np.zeros(B, dtype=np.int32); st_pert[1 * E + 2] = -4                           # the perturbed slot alone
    bad = dlogL.copy(); bad[0, 1] = np.nan; bad[1, 2] = np.inf

    def case(share, S, **kw):
        d = dict(share=share, params=params, hstep=hstep, S=S, dlogL=None, lpp=None, lpm=None, status=None, want_pr0=True, want_gp=True)
        d.update(kw)
        return d
    return {
        "full-no-prior": case(FULL, S_full),
        "diff-prior-forward-backward-flat": case(DIFF, S_diff, lpp=lpp_mix, lpm=lpm_mix, status=np.zeros(B, dtype=np.int32)),
        "full-prior-forward-backward-flat": case(FULL, S_full, lpp=lpp_mix, lpm=lpm_mix),
        "full-failed-base-and-perturbed": case(FULL, S_full, status=st_base),
        "diff-failed-base-and-perturbed": case(DIFF, S_diff, status=st_base),
        "diff-failed-base-and-perturbed-prior": case(DIFF, S_diff, status=st_base, lpp=lpp, lpm=lpm),
        "full-failed-perturbed-alone": case(FULL, S_full, status=st_pert),
        "ready-nonfinite-no-prior": case(READY, S_full[::E].copy(), dlogL=bad),
        "ready-nonfinite-prior": case(READY, S_full[::E].copy(), dlogL=bad, lpp=lpp_mix, lpm=lpm_mix),
        "ready-finite-prior": case(READY, S_full[::E].copy(), dlogL=dlogL, lpp=lpp, lpm=lpm),
        "diff-prior-null-outputs": case(DIFF, S_diff, lpp=lpp_mix, lpm=lpm_mix, want_pr0=False, want_gp=False),
        "full-no-prior-null-outputs": case(FULL, S_full, want_pr0=False, want_gp=False),
    }


CASES = make_cases()


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("sanitized", [0, 1], ids=["plain", "asan-ubsan"])
def test_assembly_matches_the_restated_rule(drivers, name, sanitized):
    case = CASES[name]
    rc, logL0, logPr0, grad, gprior = run(drivers[sanitized], case)
    w_rc, w_logL0, w_logPr0, w_grad, w_gprior = restate(case)
    assert rc == w_rc
    assert same_bits(logL0, w_logL0), (logL0, w_logL0)
    assert same_bits(grad, w_grad), (grad, w_grad)
    assert (logPr0 is None) == (not case["want_pr0"]) and (gprior is None) == (not case["want_gp"])
    if logPr0 is not None:
        assert same_bits(logPr0, w_logPr0)
    if gprior is not None and case["lpp"] is not None:   # (without a prior grad_prior is not written)
        assert same_bits(gprior, w_gprior)


def test_the_cases_reach_what_they_are_for():
    """The inputs really hold each situation the assembly has a rule for (so that a pass is not a pass on easy numbers)."""
    _, L0, _, grad, gp = restate(CASES["full-prior-forward-backward-flat"])
    assert gp[0, 0] != 0 and gp[0, 1] != 0 and gp[0, 2] == 0 and gp[1, 0] == 0 and gp[1, 1] != 0 and gp[1, 2] != 0
    rc, L0, _, grad, _ = restate(CASES["full-failed-base-and-perturbed"])
    assert rc == -5 and np.isnan(L0[0]) and np.isnan(grad[0]).all() and np.isnan(grad[1, 1]) and np.isfinite(grad[1, [0, 2]]).all()
    rc, L0, _, grad, _ = restate(CASES["diff-failed-base-and-perturbed"])
    assert rc == -5 and np.isnan(L0[0]) and np.isfinite(grad[0]).all() and np.isnan(grad[1, 1])
    assert restate(CASES["full-failed-perturbed-alone"])[0] == -4
    _, _, _, grad, _ = restate(CASES["ready-nonfinite-no-prior"])
    assert np.isnan(grad[0, 1]) and np.isinf(grad[1, 2])
    _, _, _, grad, gp = restate(CASES["ready-nonfinite-prior"])
    assert np.isfinite(grad).all() and grad[0, 1] == gp[0, 1] and grad[1, 2] == gp[1, 2]
    x0 = CASES["full-no-prior"]["params"][0, IDX[0]]
    assert (x0 + CASES["full-no-prior"]["hstep"][0]) - x0 != CASES["full-no-prior"]["hstep"][0]
    assert int(P_LIKE) == 1 and tempered(3.0, 2.5) == np.float64(LD(-3.0) / LD(2.5))

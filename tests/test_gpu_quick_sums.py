"""GPU tests (-m gpu) of the per-chain accumulators the fused step's decision shortcut reads (FusedArgs::qacc, csrc/dev_step_impl.h): every
likelihood tile adds its sum into one of eight keys of its chain (the workgroup's id & 7), the next launch's workgroups read the chain's
sixteen doubles through scalar loads, the chain's commit workgroup zeroes the set that comes free and counts a shortcut that decided
otherwise than the exact test (quick_mismatch).  None of that may move a bit of a chain -- a missed zero, a stale read or a lost add
would -- so every fused run is compared with the lockstep kernels, at the numbers of tiles at which the keys fill differently."""
import os
import subprocess

import numpy as np
import pytest

from test_step_hazards import _plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 512                      # workgroup = 64 lanes x 8 bins
N1, N2 = 64, 27                 # two run() calls
LEARN = (24, 40)                # adaptation after the even iterations of [24, 40): lockstep from 24 to the next quiet run of >= 3, at 39
STRETCHES = ((0, 24), (39, 64), (64, 91))      # the fused stretches of the two calls (csrc/step_schedule.h: next_stretch)
RUNS = ((1, 0), (2, 0), (3, 0), (2, 1), (3, 1))  # (step scheme, TAMCMC_OPT_QUICK_DECIDE): lockstep | one launch | two groups | the two, forced


def _star(oracle, synth, nx):
    star = synth.make_c2_star(nx=nx)
    _, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    star.set_spectrum_from_model(m0, nx)
    return star


def _ctx(pkg, star):
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST, workgroup=64)
    c.set_spectrum(star.x, star.y)
    return c


def _same_chain(got, ref, what):
    assert np.array_equal(got[0], ref[0]), what
    assert np.array_equal(got[1], ref[1]), what
    for key in ("iteration", "swaps", "swap_attempts", "accepted0"):
        assert got[2][key] == ref[2][key], (what, key)
    for key in ("vars", "logL", "logPrior", "logPost", "Pmove", "sigma"):
        assert np.array_equal(got[2][key], ref[2][key]), (what, key)


def _five_runs(pkg, oracle, synth, nx, nchains, dN_mixing, seed):
    """Two calls of one sampler, 64 iterations with a learning window (fused -> lockstep -> fused) and 27 more (armed start), five times:
    (samples, statistics, state, info) of each run."""
    star = _star(oracle, synth, nx)
    ctx = _ctx(pkg, star)
    kw = dict(nchains=nchains, lambda_temp=1.4, seed=seed, Nt_learn=LEARN, periods_learn=(2,), dN_mixing=dN_mixing, engine="device")
    out = []
    for scheme, forced in RUNS:
        ctx.set_option(pkg.OPT_STEP_SCHEME, scheme)
        ctx.set_option(pkg.OPT_QUICK_DECIDE, forced)
        d = pkg.Sampler(ctx, star, **kw)
        s1, t1 = d.run(N1, stats=True)
        s2, t2 = d.run(N2, stats=True)
        out.append((np.concatenate([s1, s2]), np.concatenate([t1, t2]), d.state(), d.info()))
        d.close()
    ctx.set_option(pkg.OPT_STEP_SCHEME, 0)
    ctx.set_option(pkg.OPT_QUICK_DECIDE, 0)
    ctx.close()
    return out


def _check_five(out, nchains):
    ref = out[0]
    assert ref[3]["iter_fused"] == 0 and ref[3]["quick_fallbacks"] == 0 and ref[3]["quick_mismatch"] == 0
    assert np.isfinite(ref[1]).all() and (ref[0][1:, 0] != ref[0][:-1, 0]).any()    # the cold chain moves
    for k, (scheme, forced) in enumerate(RUNS):
        if k == 0:
            continue
        info = out[k][3]
        print("\nscheme %d forced %d: %s" % (scheme, forced, {q: info[q] for q in (
            "iter_fused", "fused_stretches", "quick_fallbacks", "quick_sure", "quick_mismatch", "iter_window", "iter_joint")}))
        assert info["fused_available"] == 1, info
        assert info["iter_fused"] == sum(b - a for a, b in STRETCHES) and info["fused_stretches"] == len(STRETCHES), info
        assert info["iter_fused"] + info["iter_lockstep"] == N1 + N2, info
        tests = nchains * (info["iter_fused"] - info["fused_stretches"])
        if forced:
            assert info["quick_fallbacks"] + info["quick_sure"] == tests, (info, tests)
            assert info["quick_fallbacks"] > 0
        else:
            assert info["quick_fallbacks"] * 1000 <= tests + 1000, (info, tests)
        assert info["quick_sure"] == out[1][3]["quick_sure"]
        _same_chain(out[k], ref, (scheme, forced))
        assert info["quick_mismatch"] == 0, info


# Tiles by nx: 500 -> ONE partial tile (seven keys of every chain never receive an add and must read as zero); 4000 -> 8, one per key, the
# last partial; 4700 -> 10, keys 0 and 1 receive two adds; 33500 -> 66.  7 chains: one launch per iteration; 8: two chain groups under
# scheme 3.  dN_mixing 1 and 3: a swap pair in every iteration / iterations with and without one.  Every nx meets both chain counts and
# both mixings; the four combinations are spread over the shapes.
@pytest.mark.parametrize("nx,nchains,dN_mixing", [(500, 7, 3), (500, 8, 1), (4000, 7, 1), (4000, 8, 3), (4700, 7, 3), (4700, 8, 1),
                                                  (33500, 7, 1), (33500, 8, 3)])
def test_accumulated_sums_leave_the_chains_bitwise_unchanged(pkg, oracle, synth, nx, nchains, dN_mixing):
    assert (nx + TILE - 1) // TILE in (1, 8, 10, 66) and nx % TILE != 0
    out = _five_runs(pkg, oracle, synth, nx, nchains, dN_mixing, seed=41)
    _check_five(out, nchains)
    if nchains == 8:
        assert out[2][3]["chain_groups"] == 2, out[2][3]


@pytest.fixture(scope="module")
def draws(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quick_sums") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "step_hazard_driver.cpp")],
                   check=True, capture_output=True, timeout=300)

    def pairs_of(C, seed0=1, count=600):
        txt = subprocess.run([exe, "pairs", str(C), str(N1 + N2), str(seed0), str(count)], check=True, capture_output=True, text=True, timeout=60).stdout
        return {int(w[1]): [int(v) for v in w[2:]] for w in (line.split() for line in txt.splitlines())}
    return pairs_of


def _census(C, xs, pairs):
    """What the three fused stretches hold, from the sampler's own swap draw: straddles of the chain groups by kind, and the window and
    joint iterations of the plan (test_step_hazards._plan)."""
    n = dict(lone=0, then_boundary_pair=0)
    windows = joints = 0
    for a, b in STRETCHES:
        A = pairs[a:b]
        plan = _plan(C, xs, A + [-1])
        windows += sum(p[1] for p in plan[:-1])
        joints += sum(p[0] == C for p in plan[:-1])
        for k in range(len(A) - 1):
            if A[k] != xs - 1:
                continue
            n["then_boundary_pair"] += A[k + 1] == xs
            if A[k + 1] not in (xs - 1, xs) and not (k > 0 and A[k - 1] in (xs - 1, xs)):
                n["lone"] += 1
                assert plan[k][1] and plan[k + 1][1]      # both of its iterations run as windows
    return n, windows, joints


def test_a_chain_carries_its_accumulators_across_the_groups(pkg, oracle, synth, draws):
    """8 chains in two groups, a swap step in every iteration, the seed chosen by what its swap draws hold in the fused stretches of the
    two calls: a lone straddle (chain xsplit rides with the first group for two iterations and returns: its accumulators are added to,
    read and zeroed from both streams), a straddle followed by the pair on the moved boundary (one joint launch), and a straddle in the
    last iteration of the first call (the closing launches keep the window's ranges; the second call starts armed)."""
    nchains, xs = 8, 4
    by_seed = draws(nchains)
    seed = None
    for sd in sorted(by_seed):
        n, _, _ = _census(nchains, xs, by_seed[sd])
        if n["lone"] >= 1 and n["then_boundary_pair"] >= 1 and by_seed[sd][N1 - 1] == xs - 1:
            seed = sd
            break
    assert seed is not None, "no seed among %d holds every case" % len(by_seed)
    n, windows, joints = _census(nchains, xs, by_seed[seed])
    print("\nseed %d: %s, %d window and %d joint iterations" % (seed, n, windows, joints))
    out = _five_runs(pkg, oracle, synth, 4000, nchains, 1, seed=seed)
    _check_five(out, nchains)
    for k in (2, 4):                                       # the runs in two groups
        info = out[k][3]
        assert info["chain_groups"] == 2 and info["iter_window"] == windows and info["iter_joint"] == joints, (info, windows, joints)
    assert windows >= 3 and joints >= 1


def test_three_thousand_launches_miss_no_zero(pkg, oracle, synth):
    """One call of 3000 iterations, a swap step in each, two chain groups: a zero missed, or an add lost, once in a thousand launches
    leaves a sum that decides a test the wrong way or sends it to the exact test -- the chain differs, or quick_mismatch counts."""
    N, nchains = 3000, 8
    star = _star(oracle, synth, 4000)
    ctx = _ctx(pkg, star)
    kw = dict(nchains=nchains, lambda_temp=1.4, seed=53, Nt_learn=(10**9, 10**9 + 1), periods_learn=(2,), dN_mixing=1, engine="device")
    out = []
    for scheme in (1, 3):
        ctx.set_option(pkg.OPT_STEP_SCHEME, scheme)
        d = pkg.Sampler(ctx, star, **kw)
        s, t = d.run(N, stats=True)
        out.append((s, t, d.state(), d.info()))
        d.close()
    ctx.set_option(pkg.OPT_STEP_SCHEME, 0)
    ctx.close()
    info = out[1][3]
    print("\n%s" % {q: info[q] for q in ("iter_fused", "quick_fallbacks", "quick_sure", "quick_mismatch", "iter_window", "iter_joint")})
    assert out[0][3]["iter_fused"] == 0
    assert info["iter_fused"] == N and info["fused_stretches"] == 1 and info["chain_groups"] == 2 and info["iter_window"] > 0, info
    _same_chain(out[1], out[0], "3000 iterations")
    assert info["quick_mismatch"] == 0, info
    assert info["quick_fallbacks"] * 1000 <= nchains * (N - 1) + 1000, info


def test_kind2_records_meet_accumulators_that_stay_zero(pkg, oracle, synth):
    """The kind-2 case of tests/test_gpu_tile_head.py with ONE tile per chain: a proposal outside a prior's support leaves an empty slot,
    its only tile is skipped and adds nothing, so all sixteen doubles of the chain stay zero for that iteration -- and the record decides
    without them.  The events are counted from the lockstep kernels, one iteration per call; the fused run with the default margin must
    report exactly that many (quick_sure), be the same chain and count no mismatch."""
    star = _star(oracle, synth, 500)
    fidx = [i for i, nm in enumerate(star.names) if nm == "Frequency_l"]
    for i in (fidx[2], fidx[5]):
        star.priors[0, i] = star.params[i] - 0.02
    ctx = _ctx(pkg, star)
    N, nchains = 120, 7
    kw = dict(nchains=nchains, lambda_temp=1.4, seed=31, Nt_learn=(10**9, 10**9 + 1), periods_learn=(2,), dN_mixing=1, engine="device")
    ctx.set_option(pkg.OPT_STEP_SCHEME, 1)
    d = pkg.Sampler(ctx, star, **kw)
    smp, stt, alone, swaps = [], [], 0, 0
    for k in range(N):
        a, b = d.run(1, stats=True)
        smp.append(a); stt.append(b)
        st = d.state()
        pm = st["Pmove"].copy()
        A = -1
        if k > 0:                                    # dN_mixing = 1: a swap step at every iteration but the first
            A = d.draws(k)[3]
            if st["swaps"] != swaps:
                pm[[A, A + 1]] = pm[[A + 1, A]]
            swaps = st["swaps"]
        if k < N - 1:                                # (the last iteration is decided by the closing launch, which has no tiles)
            alone += sum(1 for m in range(nchains) if pm[m] == 0.0 and not (A >= 0 and m in (A, A + 1)))
    ref = (np.concatenate(smp), np.concatenate(stt))
    assert d.info()["iter_fused"] == 0
    d.close()
    assert alone >= 8, alone
    ctx.set_option(pkg.OPT_STEP_SCHEME, 0)
    d = pkg.Sampler(ctx, star, **kw)
    a, b = d.run(N, stats=True)
    info = d.info()
    d.close()
    ctx.close()
    assert info["iter_fused"] == N and info["fused_stretches"] == 1, info
    assert info["quick_sure"] == alone, (info, alone)
    assert info["quick_mismatch"] == 0, info
    assert info["quick_fallbacks"] * 1000 <= nchains * (N - 1) + 1000, info
    assert np.array_equal(a, ref[0]) and np.array_equal(b, ref[1])

"""GPU tests (-m gpu) of the fused step's two chain groups around a swap pair that straddles them: the boundary between the groups
moves by one chain for the two iterations concerned (a window, csrc/step_schedule.h: StepPlanner) and both groups keep launching.
The chains must stay bit for bit those of the lockstep kernels through every shape a window can take, so the seed is chosen on the CPU
-- by the sampler's own swap draw, printed by tests/step_hazard_driver.cpp -- for a run that holds all of them:
a lone straddle; the same pair straddling twice in a row; a straddle followed by the pair on the moved boundary (one joint launch); a
straddle followed by a swap inside the second group; a window that ends a stretch, here the first of two run() calls."""
import os
import subprocess

import numpy as np
import pytest

from test_step_hazards import _plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N1, N2 = 100, 140          # two run() calls, each one fused stretch (no learning window)
CASES = ("lone", "twice", "then_boundary_pair", "then_second_group", "ends_stretch")


@pytest.fixture(scope="module")
def draws(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("straddle") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "step_hazard_driver.cpp")],
                   check=True, capture_output=True, timeout=300)

    def pairs_of(C, seed0=1, count=400):
        out = subprocess.run([exe, "pairs", str(C), str(N1 + N2), str(seed0), str(count)], check=True, capture_output=True, text=True, timeout=60).stdout
        return {int(w[1]): [int(v) for v in w[2:]] for w in (line.split() for line in out.splitlines())}
    return pairs_of


def _census(C, xs, pairs):
    """What the two stretches [0, N1) and [N1, N1 + N2) hold, from the draw alone: the cases above, and the window and joint iterations
    of the plan (restated in test_step_hazards._plan; the last entry of a stretch's plan is its closing launches)."""
    n = dict.fromkeys(CASES, 0)
    windows = joints = 0
    for a, b in ((0, N1), (N1, N1 + N2)):
        A = pairs[a:b]
        plan = _plan(C, xs, A + [-1])
        windows += sum(p[1] for p in plan[:-1])
        joints += sum(p[0] == C for p in plan[:-1])
        for k in range(len(A)):
            if A[k] != xs - 1:
                continue
            if k + 1 == len(A):
                n["ends_stretch"] += 1
                assert plan[-1][0] == xs + 1          # the closing launches keep the window's ranges
                continue
            nxt = A[k + 1]
            n["twice"] += nxt == xs - 1
            n["then_boundary_pair"] += nxt == xs
            n["then_second_group"] += nxt > xs
            prev_straddles = k > 0 and A[k - 1] == xs - 1
            if not prev_straddles and nxt not in (xs - 1, xs) and not (k > 0 and A[k - 1] == xs):
                n["lone"] += 1
                assert plan[k][1] and plan[k + 1][1]      # both of its iterations run as windows
    # ... and from the draw alone, without the plan: an iteration is a window or a joint launch when its own pair or (past a stretch's
    # first iteration) the previous one is (xs-1, xs), and joint when the other of the two is (xs, xs+1)
    near = boundary = 0
    for a, b in ((0, N1), (N1, N1 + N2)):
        for k in range(a, b):
            two = (pairs[k], pairs[k - 1] if k > a else -1)
            near += xs - 1 in two
            boundary += xs - 1 in two and xs in two
    assert windows + joints == near and joints == boundary, (windows, joints, near, boundary)
    return n, windows, joints


def _seed_with_every_case(C, xs, by_seed):
    for seed in sorted(by_seed):
        pairs = by_seed[seed]
        n, _, _ = _census(C, xs, pairs)
        if all(n[c] >= 1 for c in CASES) and pairs[N1 - 1] == xs - 1:     # ... and a window lies across the boundary of the two calls
            return seed
    raise AssertionError("no seed among %d holds every case" % len(by_seed))


def _star(pkg, oracle, synth, nx=3001, seed=5):
    star = synth.make_c2_star(nx=nx)
    _, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    star.set_spectrum_from_model(m0, seed)
    return star


@pytest.fixture()
def ctx(pkg):
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST, bins_per_thread=4, workgroup=64)   # 64 x 4 bins per tile: 12 tiles, the last one partial
    yield c
    c.set_option(pkg.OPT_STEP_SCHEME, 0)
    c.set_option(pkg.OPT_QUICK_DECIDE, 0)
    c.close()


def _kw(nchains, seed):
    return dict(nchains=nchains, lambda_temp=1.4, seed=seed, Nt_learn=(10**9, 10**9 + 1), periods_learn=(2,), dN_mixing=1, chain_groups=2,
                engine="device")


@pytest.mark.parametrize("nchains", [7, 8])
def test_windows_keep_the_lockstep_chain_bit_for_bit(pkg, oracle, synth, ctx, draws, nchains):
    """Lockstep kernels | fused steps in two groups | the same with TAMCMC_OPT_QUICK_DECIDE = 1 (every tile decides by the exact test):
    identical samples, statistics, move and swap counts over 100 + 140 iterations, and the counters say how each iteration ran."""
    xs = nchains // 2
    by_seed = draws(nchains)
    seed = _seed_with_every_case(nchains, xs, by_seed)
    n, windows, joints = _census(nchains, xs, by_seed[seed])
    print("\n%d chains, groups [0, %d) [%d, %d), seed %d: %s, %d window and %d joint iterations" % (nchains, xs, xs, nchains, seed, n, windows, joints))
    assert all(n[c] >= 1 for c in CASES), n
    assert windows >= 2 * n["lone"] + n["ends_stretch"] and joints >= n["then_boundary_pair"]
    star = _star(pkg, oracle, synth)
    ctx.set_spectrum(star.x, star.y)
    out = []
    for scheme, forced in ((1, 0), (3, 0), (3, 1)):
        ctx.set_option(pkg.OPT_STEP_SCHEME, scheme)
        ctx.set_option(pkg.OPT_QUICK_DECIDE, forced)
        d = pkg.Sampler(ctx, star, **_kw(nchains, seed))
        s1, t1 = d.run(N1, stats=True)
        s2, t2 = d.run(N2, stats=True)
        out.append((np.concatenate([s1, s2]), np.concatenate([t1, t2]), d.state(), d.info()))
        d.close()
    ref_s, ref_t, ref_state, ref_info = out[0]
    assert ref_info["iter_fused"] == 0 and ref_info["iter_window"] == 0 and ref_info["iter_joint"] == 0, ref_info
    assert ref_state["swap_attempts"] == N1 + N2 - 1 and 0 < ref_state["swaps"] < ref_state["swap_attempts"]
    assert (ref_s[:, 0] != ref_s[0, 0]).any()      # chain 0 moved
    for s, t, state, info in out[1:]:
        assert info["chain_groups"] == 2 and info["iter_fused"] == N1 + N2 and info["fused_stretches"] == 2 and info["iter_lockstep"] == 0, info
        assert info["iter_window"] == windows and info["iter_joint"] == joints, (info, windows, joints)
        assert np.array_equal(s, ref_s) and np.array_equal(t, ref_t)
        for key in ("iteration", "accepted0", "swap_attempts", "swaps"):
            assert state[key] == ref_state[key], key
        for key in ("vars", "logL", "logPrior", "logPost", "Pmove", "sigma"):
            assert np.array_equal(state[key], ref_state[key]), key
    tests = nchains * (N1 + N2 - 2)
    assert out[2][3]["quick_fallbacks"] + out[2][3]["quick_sure"] == tests and out[1][3]["quick_sure"] == out[2][3]["quick_sure"]


def test_records_written_into_pinned_buffers_through_a_window(pkg, oracle, synth, ctx, draws):
    """Two samplers on one context take turns, a batched evaluation in between; one records into page-locked arrays (the commit
    workgroups write every iteration's record straight into them, from whichever launch and stream holds the chain), the other into
    device buffers copied at the end of the call.  Same records, with a window across the boundary of the two calls."""
    nchains, xs = 8, 4
    by_seed = draws(nchains)
    seed = _seed_with_every_case(nchains, xs, by_seed)
    assert by_seed[seed][N1 - 1] == xs - 1
    star = _star(pkg, oracle, synth)
    ctx.set_spectrum(star.x, star.y)
    ctx.set_option(pkg.OPT_STEP_SCHEME, 3)
    a, b = pkg.Sampler(ctx, star, **_kw(nchains, seed)), pkg.Sampler(ctx, star, **_kw(nchains, seed))
    for n in (N1, N2):
        ps, pt = pkg.pinned_empty((n, nchains, a.nvars)), pkg.pinned_empty((n, nchains, 3))
        ps[:] = np.nan; pt[:] = np.nan
        a.run(n, out=(ps, pt))
        ctx.loglike_params_batch(star.model_id, star.params, star.plength)
        s, t = b.run(n, stats=True)
        assert np.array_equal(ps, s) and np.array_equal(pt, t), n
    _, windows, joints = _census(nchains, xs, by_seed[seed])
    for smp in (a, b):
        info = smp.info()
        assert info["iter_fused"] == N1 + N2 and info["iter_window"] == windows and info["iter_joint"] == joints, info
    assert np.array_equal(a.state()["vars"], b.state()["vars"])
    a.close(); b.close()

"""The hybrid adjoint gradient of a red giant (model id 25; TAMCMC_OPT_GRADIENT = TAMCMC_GRADIENT_ADJOINT with TAMCMC_OPT_RGB_ADJOINT = 1)
against the windowed finite-difference batch it replaces, FAST arithmetic, one GPU, one process.  Two shapes: the C5 star at its
defaults (2e5 bins, 40 chains) and the small star of tests/test_gpu_rgb_adjoint.py (4000 bins, 3 chains).

  batch     wall time of one synchronous tamcmc_hip_fd_gradient call, the two routes interleaved call by call: two warm-up calls each, then
            the median of `reps` calls with [min, max];
  split     HIP events inside the hybrid batch (timing on, a context of its own): table build with the classification, base launch, row
            pass, noise pass + folds, fallback delta launches, contraction -- medians over the same number of calls;
  langevin  iterations per second of both engines on both routes (tools/rgb_mala_probe.py's measurement: two warm-up calls, median of
            `lreps` calls of `iters` iterations with [min, max], no adaptation);
  counters  linearised and fallback slots over a walk of `walk` iterations of the device engine on the hybrid route.

    python tools/rgb_adjoint_probe.py [--reps 10] [--lreps 5] [--iters 50] [--walk 350] [--shapes c5,small] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SPLIT = ("tables_ms", "base_launch_ms", "row_pass_ms", "noise_pass_ms", "fallback_delta_ms", "contraction_ms")


def model_row(pkg, star):
    """The star's own model row (the spectrum is that row times exponential noise)."""
    c = pkg.HipContext(0, precision=pkg.PRECISION_STRICT)
    c.set_spectrum(star.x, np.ones_like(star.x))
    _, model, st = c.loglike_params_batch(star.model_id, star.params, star.plength, want_model=True)
    c.close()
    assert (st == 0).all()
    return model[0]


def stat(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def hybrid(pkg, ctx, on):
    ctx.set_option(pkg.OPT_RGB_ADJOINT, 1)
    ctx.set_option(pkg.OPT_GRADIENT, pkg.GRADIENT_ADJOINT if on else pkg.GRADIENT_FD)


def rate(s, warm, reps, iters):
    for _ in range(warm):
        s.run(iters, record=False)
    r = []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.run(iters, record=False)
        r.append(iters / (time.perf_counter() - t0))
    return stat(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--lreps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--walk", type=int, default=350)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--shapes", default="c5,small")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = entry.load_package()
    from tamcmc_c_amd import synth
    small = synth.make_c5_star(nx=4000, nmax=4, dnu=20.0, nferr=4)
    o = np.cumsum([0] + list(small.plength))
    small.params[o[3] + 1] = 200.0
    small.priors[:2, o[3] + 1] = [199.0, 201.0]
    shapes = {"c5": (synth.make_c5_star, 40, 1.15), "small": (lambda: small, 3, 1.6)}
    res = {"reps": a.reps, "warm": a.warm, "lreps": a.lreps, "iters": a.iters, "walk": a.walk, "seed": a.seed, "shapes": {}}
    for name in a.shapes.split(","):
        make, nch, lam = shapes[name]
        star = make()
        idx = star.index_to_relax
        y = model_row(pkg, star) * np.random.default_rng(7).exponential(1.0, star.x.size)
        P = np.tile(star.params, (nch, 1))
        P[1:, : star.plength[0]] *= 1 + 0.01 * np.random.default_rng(1).standard_normal((nch - 1, star.plength[0]))
        T = lam ** np.arange(nch)
        h = 1e-7 * np.maximum(np.abs(star.params[idx]), 1e-3)
        shape = {"nx": int(star.x.size), "chains": nch, "nvars": int(idx.size), "lambda_temp": lam}
        ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
        ctx.set_spectrum(star.x, y)
        ctx.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 1)
        # ---- one batch, the two routes call by call ----
        t = {False: [], True: []}
        g = {}
        for i in range(a.warm + a.reps):
            for on in (False, True):
                hybrid(pkg, ctx, on)
                t0 = time.perf_counter()
                _, g[on] = ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T)
                if i >= a.warm:
                    t[on].append((time.perf_counter() - t0) * 1e3)
        shape["windowed_ms"], shape["hybrid_ms"] = stat(t[False]), stat(t[True])
        shape["hybrid_vs_windowed_rel"] = float(np.nanmax(np.abs(g[True] - g[False])) / np.nanmax(np.abs(g[False])))
        # ---- the split of the hybrid batch and its slots (timing on) ----
        ct = pkg.HipContext(0, precision=pkg.PRECISION_FAST, timing=True)
        ct.set_spectrum(star.x, y)
        hybrid(pkg, ct, True)
        sp = []
        for i in range(a.warm + a.reps):
            ct.reset_kernel_stats()
            ct.fd_gradient(star.model_id, P, star.plength, idx, h, T)
            if i >= a.warm:
                sp.append(ct.rgb_adjoint_times())
        for k, col in zip(SPLIT, np.array(sp).T):
            shape[k] = stat(col)
        shape["batch_slots_linearised_fallback"] = ct.rgb_adjoint_stats()
        # ---- Langevin iterations per second, both engines, both routes ----
        kw = dict(nchains=nch, lambda_temp=lam, use_drift=1, seed=a.seed, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,), dN_mixing=1)
        for engine in ("host", "device"):
            for on in (False, True):
                hybrid(pkg, ctx, on)
                s = pkg.Sampler(ctx, star, engine=engine, **kw)
                shape["%s_%s_iterations_per_s" % (engine, "hybrid" if on else "windowed")] = rate(s, a.warm, a.lreps, a.iters)
                s.close()
        # ---- slots over a walk ----
        ct.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 1)
        s = pkg.Sampler(ct, star, engine="device", **kw)
        ct.reset_kernel_stats()
        s.run(a.walk, record=False)
        shape["walk_slots_linearised_fallback"] = ct.rgb_adjoint_stats()
        shape["walk_accepted0"] = s.state()["accepted0"]
        s.close()
        ct.close()
        ctx.close()
        res["shapes"][name] = shape
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

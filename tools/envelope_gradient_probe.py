"""Timing probe of the Gaussian-envelope fits' gradient batch (model ids 0, 1) on one MI355X: TAMCMC_OPT_ENVELOPE_GRADIENT 0 (brute force,
Nvars + 1 evaluations per chain) against 1 (the analytic likelihood share, one pass per chain), in the same process.

  * one tamcmc_hip_fd_gradient_posterior call at (id, Nx, C) in {(1, 5 400, 10), (0, 32 393, 10), (1, 10^6, 20), (0, 10^6, 20)}: host wall
    time per call (median, p90; the call ends in a stream synchronise) and device time of the likelihood's kernels (HIP events,
    TAMCMC_OPT_TIMING: k_env_ksi + k_env_eval + k_finalize, or k_env_ksi_grad + k_env_grad + k_env_grad_fold; the prior's
    kernel is outside the bracket on both routes);
  * host-engine Langevin iterations/s on the 1161491 fixture (model_Harvey_Gaussian, 10 chains), both ways, and the random walk.

Usage: python tools/envelope_gradient_probe.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

SHAPES = ((1, 5400, 10), (0, 32393, 10), (1, 1000000, 20), (0, 1000000, 20))


def star_for(synth, pkg, model_id, nx):
    star = synth.make_envelope_star(model_id, nx=nx, seed=3)
    ctx = pkg.HipContext(0)
    ctx.set_spectrum(star.x, np.ones_like(star.x))
    _, m, _ = ctx.loglike_params_batch(model_id, star.params, star.plength, want_model=True)
    ctx.close()
    star.set_spectrum_from_model(m[0], seed=4)
    return star


def time_batch(pkg, ctx, star, C, option, reps):
    rng = np.random.default_rng(C)
    P = np.tile(star.params, (C, 1))
    P[1:, star.relax == 1] *= 1.0 + 0.01 * rng.standard_normal((C - 1, star.nvars))
    T = 1.5 ** np.arange(C)
    h = 1e-7 * np.maximum(np.abs(star.params[star.index_to_relax]), 1e-3)
    ctx.set_option(pkg.OPT_ENVELOPE_GRADIENT, option)
    for _ in range(5):
        ctx.fd_gradient_posterior(star, P, h, Tcoefs=T)
    ctx.reset_kernel_stats()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.fd_gradient_posterior(star, P, h, Tcoefs=T)
        walls.append(time.perf_counter() - t0)
    ms, launches, evals = ctx.kernel_stats()
    return {"model_id": star.model_id, "Nx": int(star.x.size), "C": C, "Nvars": int(star.nvars), "option": option,
            "passes_per_call": evals // launches, "device_us": ms * 1e3 / launches, "wall_us": float(np.median(walls)) * 1e6,
            "wall_p90_us": float(np.percentile(walls, 90)) * 1e6, "reps": reps}


def sampler_rate(pkg, inputs, sampler, use_drift, option, n):
    gold = os.path.join(ROOT, "tests", "golden", "envelope")
    star, _ = inputs.load_simple_star(os.path.join(gold, "1161491_Gaussfit.model"), os.path.join(gold, "1161491_Gaussfit.data"), 1)
    ctx = pkg.HipContext(0)
    ctx.set_spectrum(star.x, star.y)
    ctx.set_option(pkg.OPT_ENVELOPE_GRADIENT, option)
    s = sampler.Sampler(ctx, star, nchains=10, lambda_temp=1.5, use_drift=use_drift, Nt_learn=(100, 200, 400), periods_learn=(1, 5))
    s.run(500, record=False)
    rates = []
    for _ in range(3):
        t0 = time.perf_counter()
        s.run(n, record=False)
        rates.append(n / (time.perf_counter() - t0))
    s.close()
    ctx.close()
    return {"star": "1161491", "Nx": int(star.x.size), "chains": 10, "use_drift": use_drift, "option": option, "iterations": n,
            "iter_per_s": float(np.median(rates)), "iter_per_s_runs": rates}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    pkg = g.load_package()
    from tamcmc_c_amd import inputs, sampler, synth
    res = {"batches": [], "sampler": []}
    for model_id, nx, C in SHAPES:
        star = star_for(synth, pkg, model_id, nx)
        ctx = pkg.HipContext(0, timing=True)
        ctx.set_spectrum(star.x, star.y)
        for option in (0, 1, 0, 1):   # each route twice, interleaved: drift of the clocks shows as a difference between the repeats
            r = time_batch(pkg, ctx, star, C, option, reps=200 if nx < 100000 else 30)
            print(json.dumps(r), flush=True)
            res["batches"].append(r)
        ctx.close()
    for use_drift, option, n in ((1, 0, 2000), (1, 1, 2000), (0, 0, 4000), (1, 0, 2000), (1, 1, 2000)):
        r = sampler_rate(pkg, inputs, sampler, use_drift, option, n)
        print(json.dumps(r), flush=True)
        res["sampler"].append(r)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

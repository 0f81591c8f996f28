"""Timing probe of the Gaussian-envelope fits (model ids 0, 1; csrc/envelope.hip) on one MI355X.

  * one batched tamcmc_hip_loglike_params_batch call at Nx in {5 400, 32 393, 10^6} and B in {4, 20, 80} for each model:
    host wall time per call (the call ends in a stream synchronise) and device time of its kernels (HIP events around
    k_env_ksi + k_env_eval + k_finalize, TAMCMC_OPT_TIMING);
  * host-driven sampler iterations/s on the 1161491 fixture (model_Harvey_Gaussian, 5 380 bins), random walk and Langevin.

Roofs: bytes = 24 B per bin and vector (x, y, ln x read by every vector's workgroups; the unique bytes are 24 B per bin) over
6.29 TB/s (measured HBM copy rate); fp64 issue = the per-bin instruction estimate below over 256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles
(one wave64 fp64 VALU issue every 2 cycles per SIMD).  Usage: python tools/envelope_probe.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

# fp64 wave-instruction issues per bin (tools/ubench.hip costs: exp ~21, log ~72, IEEE divide ~12.6, sin ~40, fma/add/mul 1)
SLOTS = {1: 3 * 21 + 3 * 12.6 + 72 + 15,          # Gaussian exp + 2 power-law exp, 2 reciprocals + y/M, ln M, adds/muls
         0: 4 * 21 + 5 * 12.6 + 40 + 72 + 20 + (3 * 21 + 3 * 12.6 + 6)}  # + sinc^2, + the trapezoid pass
HBM = 6.29e12
ISSUE = 256 * 4 * 2.4e9 / 2


def star_for(synth, pkg, model_id, nx):
    star = synth.make_envelope_star(model_id, nx=nx, seed=3)
    ctx = pkg.HipContext(0)
    ctx.set_spectrum(star.x, np.ones_like(star.x))
    _, m, _ = ctx.loglike_params_batch(model_id, star.params, star.plength, want_model=True)
    ctx.close()
    star.set_spectrum_from_model(m[0], seed=4)
    return star


def time_call(pkg, star, model_id, B, reps):
    rng = np.random.default_rng(B)
    P = np.tile(star.params, (B, 1))
    P[1:, star.relax == 1] *= 1.0 + 0.01 * rng.standard_normal((B - 1, star.nvars))
    ctx = pkg.HipContext(0, timing=True)
    ctx.set_spectrum(star.x, star.y)
    for _ in range(10):
        ctx.loglike_params_batch(model_id, P, star.plength)
    ctx.reset_kernel_stats()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.loglike_params_batch(model_id, P, star.plength)
        walls.append(time.perf_counter() - t0)
    ms, launches, _ = ctx.kernel_stats()
    ctx.close()
    wall = float(np.median(walls))
    dev = ms * 1e-3 / launches
    nx = star.x.size
    t_bytes = 24.0 * nx * B / HBM
    t_issue = SLOTS[model_id] * nx * B / 64 / ISSUE
    return {"model_id": model_id, "Nx": nx, "B": B, "wall_us": wall * 1e6, "wall_p90_us": float(np.percentile(walls, 90)) * 1e6,
            "device_us": dev * 1e6, "hbm_roof_frac": t_bytes / dev, "fp64_issue_frac": t_issue / dev,
            "bound_by": "fp64 issue" if t_issue > t_bytes else "bytes"}


def sampler_rate(pkg, inputs, sampler, use_drift, n):
    gold = os.path.join(ROOT, "tests", "golden", "envelope")
    star, _ = inputs.load_simple_star(os.path.join(gold, "1161491_Gaussfit.model"), os.path.join(gold, "1161491_Gaussfit.data"), 1)
    ctx = pkg.HipContext(0)
    ctx.set_spectrum(star.x, star.y)
    s = sampler.Sampler(ctx, star, nchains=10, lambda_temp=1.5, use_drift=use_drift, Nt_learn=(100, 200, 400), periods_learn=(1, 5))
    s.run(500, record=False)
    t0 = time.perf_counter()
    s.run(n, record=False)
    dt = time.perf_counter() - t0
    s.close()
    ctx.close()
    return {"star": "1161491", "Nx": star.x.size, "chains": 10, "use_drift": use_drift, "iterations": n, "iter_per_s": n / dt}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    pkg = g.load_package()
    from tamcmc_c_amd import inputs, sampler, synth
    res = {"calls": [], "sampler": []}
    for model_id in (1, 0):
        for nx in (5400, 32393, 1000000):
            star = star_for(synth, pkg, model_id, nx)
            for B in (4, 20, 80):
                r = time_call(pkg, star, model_id, B, reps=200 if nx < 100000 else 40)
                print(json.dumps(r), flush=True)
                res["calls"].append(r)
    for use_drift, n in ((0, 4000), (1, 1000)):
        r = sampler_rate(pkg, inputs, sampler, use_drift, n)
        print(json.dumps(r), flush=True)
        res["sampler"].append(r)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

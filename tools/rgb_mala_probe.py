"""Langevin iterations per second of the two engines on a red giant (model id 25): the host-driven engine (one gradient batch per
iteration through tamcmc_hip_fd_gradient_posterior, proposal and linear algebra on the host) and the device-resident engine with
TAMCMC_OPT_RGB_DEVICE_LANGEVIN = 1 (the same batch between two small kernels, nothing crossing PCIe inside an iteration).  FAST
arithmetic, one GPU, same seed, one process; per engine two warm-up calls, then the median of `reps` calls of `iters` iterations with
[min, max].  Two shapes: the C5 star at its defaults (2e5 bins, 40 chains) and the small star of tests/test_gpu_rgb_device_langevin.py
(4000 bins, 3 chains).  No adaptation inside the measured calls.

    python tools/rgb_mala_probe.py [--reps 5] [--iters 50] [--out FILE.json]
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


def model_row(pkg, star):
    """The star's own model row (the spectrum is that row times exponential noise)."""
    c = pkg.HipContext(0, precision=pkg.PRECISION_STRICT)
    c.set_spectrum(star.x, np.ones_like(star.x))
    _, model, st = c.loglike_params_batch(star.model_id, star.params, star.plength, want_model=True)
    c.close()
    assert (st == 0).all()
    return model[0]


def rate(s, warm, reps, iters):
    """Iterations per second of s.run(iters, record=False): (median, min, max) over reps calls after warm calls."""
    for _ in range(warm):
        s.run(iters, record=False)
    r = []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.run(iters, record=False)
        r.append(iters / (time.perf_counter() - t0))
    return float(np.median(r)), float(np.min(r)), float(np.max(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = entry.load_package()
    from tamcmc_c_amd import synth
    small = synth.make_c5_star(nx=4000, nmax=4, dnu=20.0, nferr=4)
    o = np.cumsum([0] + list(small.plength))
    small.params[o[3] + 1] = 200.0
    small.priors[:2, o[3] + 1] = [199.0, 201.0]
    res = {"reps": a.reps, "iters": a.iters, "warm": a.warm, "seed": a.seed, "shapes": {}}
    for name, star, nch, lam in (("c5", synth.make_c5_star(), 40, 1.15), ("small", small, 3, 1.6)):
        y = model_row(pkg, star) * np.random.default_rng(7).exponential(1.0, star.x.size)
        ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
        ctx.set_spectrum(star.x, y)
        ctx.set_option(pkg.OPT_RGB_DEVICE_LANGEVIN, 1)
        shape = {"nx": int(star.x.size), "chains": nch, "nvars": int(star.index_to_relax.size), "lambda_temp": lam}
        for engine in ("host", "device"):
            s = pkg.Sampler(ctx, star, nchains=nch, lambda_temp=lam, use_drift=1, seed=a.seed, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,),
                            dN_mixing=1, engine=engine)
            shape[engine + "_iterations_per_s"] = rate(s, a.warm, a.reps, a.iters)
            st = s.state()
            shape[engine + "_accepted0"] = st["accepted0"]
            shape[engine + "_swaps"] = st["swaps"]
            s.close()
        ctx.close()
        res["shapes"][name] = shape
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

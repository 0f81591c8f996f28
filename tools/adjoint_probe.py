"""Microseconds per gradient batch at the headline (C3) shape -- 1e5 bins, 20 chains, 93 variables -- windowed finite differences against the
adjoint route (TAMCMC_OPT_GRADIENT), interleaved in one session, three runs each; then Langevin steps per second of the device engine
either way.  A report, not a pass/fail gate.  Event-timed: from the base launch to the last sum (the unpack kernel in front of both routes
is outside the bracket, and the same); wall: the whole call, transfers included.
timeout -k 10 300 python tools/adjoint_probe.py [--calls 20] [--steps 300]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--steps", type=int, default=300)
args = ap.parse_args()

pkg = entry.load_package()
from tamcmc_c_amd import synth

star = synth.make_c3_star()
ctx = pkg.HipContext(0, precision=pkg.PRECISION_STRICT, timing=True)
ctx.set_spectrum(star.x, np.ones_like(star.x))
_, m0, _ = ctx.loglike_params_batch(star.model_id, star.params, star.plength, want_model=True)
star.set_spectrum_from_model(m0[0], seed=20240301)
ctx.set_option(pkg.OPT_PRECISION, pkg.PRECISION_FAST)
ctx.set_option(pkg.OPT_WORKGROUP, 64)
ctx.set_option(pkg.OPT_BINS_PER_THREAD, 8)
ctx.set_spectrum(star.x, star.y)
idx = star.index_to_relax
rng = np.random.default_rng(1)
P = np.tile(star.params, (20, 1))
P[1:, idx] *= 1 + 0.002 * rng.standard_normal((19, idx.size))
T = 1.3 ** np.arange(20)
h = 1e-7 * np.maximum(np.abs(star.params[idx]), 1e-3)
ROUTES = (("windowed FD", pkg.GRADIENT_FD), ("adjoint", pkg.GRADIENT_ADJOINT))

grads = {}
for run in range(3):
    for name, val in ROUTES:
        ctx.set_option(pkg.OPT_GRADIENT, val)
        _, grads[name] = ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T, 1.0)   # (warm-up: buffers of this route)
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T, 1.0)
        wall = (time.perf_counter() - t0) / args.calls
        ms, nl, _ = ctx.kernel_stats()
        print(f"run {run} {name:12s}: {1e3 * ms / nl:8.1f} us per batch (events), {1e6 * wall:8.1f} us per call (wall)", flush=True)
d = np.abs(grads["adjoint"] - grads["windowed FD"]) / np.max(np.abs(grads["windowed FD"]), axis=1, keepdims=True)
print(f"adjoint against windowed FD: {100 * np.mean(d > 1e-4):.0f} % of components differ by more than 1e-4 of the gradient's scale, "
      f"largest {d.max():.1e}", flush=True)

ctx.set_option(pkg.OPT_TIMING, 0)
for run in range(3):
    for name, val in ROUTES:
        ctx.set_option(pkg.OPT_GRADIENT, val)
        s = pkg.Sampler(ctx, star, engine="device", use_drift=1, nchains=20, lambda_temp=1.3, seed=7, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,))
        s.run(20, record=False)
        t0 = time.perf_counter()
        s.run(args.steps, record=False)
        dt = time.perf_counter() - t0
        s.close()
        print(f"run {run} {name:12s}: {args.steps / dt:8.0f} Langevin steps/s (device engine, 20 chains)", flush=True)
ctx.close()

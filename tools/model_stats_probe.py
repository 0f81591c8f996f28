"""Posterior model spectrum at the headline (C3) shape -- 1e5 bins, 111 parameters, 2048 vectors drawn around the star's truth: wall time of
ModelStats.add_params + result() (tamcmc_hip_model_stats_*: the reduction over the samples axis on the device, seven planes of Nx doubles
come back) against the route the library had before it, in the same process -- loglike_params_batch(want_model=True) in chunks of 64 with
a numpy accumulation of the same sums (every model row crosses PCIe).  Two warm-up calls, median of --calls with [min, max], like the other
probes.  Both routes use one STRICT context (the accumulator's arithmetic does not depend on the mode); the two results are compared bit
for bit first.  A report, not a pass/fail gate.
timeout -k 10 500 python tools/model_stats_probe.py [--vectors 2048] [--calls 10] [--chunk 0] [--host-chunk 64] [--nx 100000]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry

ap = argparse.ArgumentParser()
ap.add_argument("--vectors", type=int, default=2048)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--chunk", type=int, default=0, help="vectors per launch of the device route (0 = the library's default)")
ap.add_argument("--host-chunk", type=int, default=64, help="vectors per loglike_params_batch call of the host route")
ap.add_argument("--nx", type=int, default=100000)
args = ap.parse_args()

pkg = entry.load_package()
from tamcmc_c_amd import synth

star = synth.make_c3_star(nx=args.nx)
ctx = pkg.HipContext(0, precision=pkg.PRECISION_STRICT)
ctx.set_spectrum(star.x, np.ones_like(star.x))
_, m0, _ = ctx.loglike_params_batch(star.model_id, star.params, star.plength, want_model=True)
star.set_spectrum_from_model(m0[0], seed=20240301)
ctx.set_spectrum(star.x, star.y)
idx = star.index_to_relax
rng = np.random.default_rng(1)
P = np.tile(star.params, (args.vectors, 1))
P[:, idx] *= 1 + 2e-4 * rng.standard_normal((args.vectors, idx.size))
Nx = star.x.size
print(f"C3 star: {Nx} bins, {star.params.size} parameters, {args.vectors} vectors, STRICT rows", flush=True)


def device_route():
    ms = ctx.model_stats(star, chunk=args.chunk)
    ms.add_params(P)
    out = ms.result()
    ms.close()
    return out


def host_route():
    """The accumulator law (tests/model_stats_numpy.py) fed chunk by chunk with the rows the library copies back; no background (the rows do not
    carry it: a second pass over zero-height tables would double this route's time)."""
    R = None
    A1, A2, Q = np.zeros(Nx), np.zeros(Nx), np.zeros(Nx)
    mn, mx = np.full(Nx, np.inf), np.full(Nx, -np.inf)
    W = 0.0
    for lo in range(0, args.vectors, args.host_chunk):
        _, rows, status = ctx.loglike_params_batch(star.model_id, P[lo:lo + args.host_chunk], star.plength, want_model=True)
        for M, st in zip(rows, status):
            if st != 0:
                continue
            if R is None:
                R = M.copy()
            d = M - R
            A1 = A1 + d
            A2 = A2 + d * d
            mn = np.where(M < mn, M, mn)
            mx = np.where(M > mx, M, mx)
            Q = Q + star.y / M
            W = W + 1.0
    v = (A2 - A1 * A1 / W) / W
    return {"mean": R + A1 / W, "var": np.where(v < 0, 0.0, v), "min": mn, "max": mx, "ratio": Q / W}


a, b = device_route(), host_route()
for k in ("mean", "var", "min", "max", "ratio"):
    assert np.array_equal(a[k], b[k]), k
print("the two routes agree bit for bit (mean, var, min, max, ratio); relative spread sqrt(var)/mean: median %.2e" %
      np.median(np.sqrt(a["var"]) / a["mean"]), flush=True)

res = {}
for name, fn in (("device", device_route), ("host", host_route)):
    t = []
    for call in range(args.calls + 2):
        t0 = time.perf_counter()
        fn()
        if call >= 2:
            t.append(time.perf_counter() - t0)
    res[name] = t
    print(f"{name} route: {1e3 * np.median(t):.1f} ms per {args.vectors} vectors (wall, median of {args.calls}) [{1e3 * min(t):.1f}, {1e3 * max(t):.1f}]",
          flush=True)
print("host / device: %.2f  (device route moves %.1f MB to the host, host route %.1f MB)" %
      (np.median(res["host"]) / np.median(res["device"]), 7 * Nx * 8 / 1e6, args.vectors * Nx * 8 / 1e6), flush=True)
ctx.close()

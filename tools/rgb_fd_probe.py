"""One red-giant finite-difference gradient batch at the C5 shape (2e5 bins, 40 chains, the C5 star's free parameters), brute force and
windowed, against the only way to get that gradient without the batch: Nvars + 1 plain loglike_params_batch calls of 40 vectors each
(an entry this change does not touch).  Wall time of the synchronous calls, same process, warm-up first, median of the repetitions.

    python tools/rgb_fd_probe.py [--nx 200000] [--chains 40] [--reps 10] [--out FILE.json]
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


def median_ms(fn, warm, reps):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=200000)
    ap.add_argument("--chains", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = entry.load_package()
    from tamcmc_c_amd import synth
    star = synth.make_c5_star(nx=a.nx)
    idx = star.index_to_relax
    rng = np.random.default_rng(1)
    P = np.tile(star.params, (a.chains, 1))
    P[1:, : star.plength[0]] *= 1 + 0.01 * rng.standard_normal((a.chains - 1, star.plength[0]))
    T = 1.15 ** np.arange(a.chains)
    h = 1e-7 * np.maximum(np.abs(star.params[idx]), 1e-3)
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    logL, m0, st = ctx_model(pkg, star)
    ctx.set_spectrum(star.x, m0 * np.random.default_rng(7).exponential(1.0, m0.size))
    V = np.repeat(P[:, None, :], idx.size + 1, axis=1)
    for k, i in enumerate(idx):
        V[:, k + 1, i] += h[k]
    res = {"nx": a.nx, "chains": a.chains, "nvars": int(idx.size), "reps": a.reps}
    for name, w in (("brute_force_ms", 0), ("windowed_ms", 1)):
        ctx.set_option(pkg.OPT_FD_WINDOWED, w)
        res[name] = median_ms(lambda: ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T), a.warm, a.reps)

    def plain():
        for e in range(idx.size + 1):
            ctx.loglike_params_batch(star.model_id, V[:, e, :], star.plength, T)
    res["plain_calls_ms"] = median_ms(plain, 1, a.reps)
    ctx.set_option(pkg.OPT_FD_WINDOWED, 0)
    _, g_f = ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T)
    ctx.set_option(pkg.OPT_FD_WINDOWED, 1)
    _, g_w = ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T)
    res["windowed_vs_brute_rel"] = float(np.max(np.abs(g_w - g_f)) / np.max(np.abs(g_f)))
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def ctx_model(pkg, star):
    """The star's own model row (the spectrum is that row times exponential noise)."""
    c = pkg.HipContext(0, precision=pkg.PRECISION_STRICT)
    c.set_spectrum(star.x, np.ones_like(star.x))
    logL, model, st = c.loglike_params_batch(star.model_id, star.params, star.plength, want_model=True)
    c.close()
    assert (st == 0).all()
    return logL, model[0], st


if __name__ == "__main__":
    main()

"""Fisher information at the headline (C3) shape -- 1e5 bins, 93 variables, 20 chains, FAST arithmetic -- and at the red-giant (C5) shape
of bench.py -- 2e5 bins, 40 chains, TAMCMC_OPT_RGB_FISHER = 1: wall time of one tamcmc_hip_fisher
call and its split into table build, row launches and Gram + fold (HIP events), median of --calls calls after two warm-ups; the Gram
against the time the same U takes to stream from HBM once and against the fp64 matrix peak; for comparison (2 Nvars + 1) / (Nvars + 1)
brute-force gradient batches on the same context.  Then, on the same star with the device engine: iterations of learning until chain 0's
acceptance over a 500-iteration window first lies in [0.15, 0.35]
(iterations counted from the start of the run; the first 100 are burn-in without adaptation, as in bench.py's learning leg), from the default proposal law and from the Fisher-seeded one, same seed
(one observation per law).  The red-giant leg also prints the three form counters (central / one-sided / unfrozen) of a call with
hstep_rel = 1e-6.  A report, not a pass/fail gate.
timeout -k 10 500 python tools/fisher_probe.py [--shapes c3,c5] [--calls 10] [--learn-max 20000] [--hbm-tbs 6.3] [--fp64-matrix-tflops 78.6]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--shapes", default="c3,c5")
ap.add_argument("--learn-max", type=int, default=20000)
ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM bandwidth, TB/s (8.0 on the data sheet)")
ap.add_argument("--fp64-matrix-tflops", type=float, default=78.6, help="fp64 matrix peak, TFLOP/s (MI355X data sheet)")
args = ap.parse_args()

pkg = entry.load_package()
from tamcmc_c_amd import synth

def leg(shape):
    if shape == "c5":
        star, C, lam, spec_seed = synth.make_c5_star(nx=200000, nmax=10, dnu=10.0, bias_type=1, nferr=6), 40, 1.15, 7   # bench.py's red-giant leg
    else:
        star, C, lam, spec_seed = synth.make_c3_star(), 20, 1.3, 20240301
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_STRICT, timing=True)
    ctx.set_option(pkg.OPT_RGB_FISHER, 1)
    ctx.set_spectrum(star.x, np.ones_like(star.x))
    _, m0, _ = ctx.loglike_params_batch(star.model_id, star.params, star.plength, want_model=True)
    star.set_spectrum_from_model(m0[0], seed=spec_seed)
    ctx.set_option(pkg.OPT_PRECISION, pkg.PRECISION_FAST)
    ctx.set_spectrum(star.x, star.y)
    idx = star.index_to_relax
    Nv, Nx = idx.size, star.x.size
    rng = np.random.default_rng(1)
    P = np.tile(star.params, (C, 1))
    P[1:, idx] *= 1 + 0.002 * rng.standard_normal((C - 1, idx.size))
    T = lam ** np.arange(C)
    h = 1e-6 * np.maximum(np.abs(star.params[idx]), 1e-2)
    print(f"shape {shape} (model id {star.model_id}): {Nx} bins, {Nv} variables, {C} chains, FAST", flush=True)

    wall, split = [], []
    for call in range(args.calls + 2):
        t0 = time.perf_counter()
        F = ctx.fisher(star.model_id, P, star.plength, idx, h, T, 1.0)
        dt = time.perf_counter() - t0
        if call >= 2:
            wall.append(dt)
            split.append(ctx.fisher_times())
    assert np.all(np.isfinite(F))
    tab, rows, gram = (float(np.median([s[i] for s in split])) for i in range(3))
    print(f"tamcmc_hip_fisher: {1e3 * np.median(wall):.2f} ms per call (wall, median of {args.calls}); events: table build {tab:.3f} ms, "
          f"row launches {rows:.3f} ms, Gram + fold {gram:.3f} ms; wall min / max {1e3 * min(wall):.2f} / {1e3 * max(wall):.2f} ms", flush=True)
    if shape == "c5":
        print("forms (central, one-sided, unfrozen) of the last call, %d pairs: %s" % (C * Nv, ctx.rgb_fisher_stats()), flush=True)
    u_bytes = C * (2 * Nv + 1) * Nx * 8.0          # the three row sets U is formed from, read once
    flops = C * 2.0 * Nv * Nv * Nx / 2.0 * (1 + 1.0 / Nv)  # the upper triangle of U U^T
    print(f"Gram + fold: {gram / (1e3 * u_bytes / (args.hbm_tbs * 1e12)):.2f} x the time {u_bytes / 1e9:.2f} GB take to stream from HBM once at "
          f"{args.hbm_tbs} TB/s; {100 * flops / (gram * 1e-3) / (args.fp64_matrix_tflops * 1e12):.2f} % of the fp64 matrix peak "
          f"({flops / 1e9:.1f} GFLOP in the upper triangle)", flush=True)

    ctx.set_option(pkg.OPT_FD_WINDOWED, 0)
    bf = []
    for call in range(args.calls + 2):
        t0 = time.perf_counter()
        ctx.fd_gradient(star.model_id, P, star.plength, idx, h, T, 1.0)
        if call >= 2:
            bf.append(time.perf_counter() - t0)
    ctx.set_option(pkg.OPT_FD_WINDOWED, 1)
    ratio = (2 * Nv + 1) / (Nv + 1)
    print(f"brute-force gradient batch ({Nv + 1} evaluations per chain): {1e3 * np.median(bf):.2f} ms per call (wall); x {ratio:.2f} = "
          f"{1e3 * ratio * np.median(bf):.2f} ms for the Fisher call's {2 * Nv + 1} rows per chain", flush=True)

    ctx.set_option(pkg.OPT_TIMING, 0)
    for law in ("default", "seeded"):
        s = pkg.Sampler(ctx, star, nchains=C, lambda_temp=lam, seed=11, engine="device", Nt_learn=(100, 10**9), periods_learn=(1,), c0=2.0)
        if law == "seeded":
            s.seed_proposal_fisher()
        cov = s.get_proposal(0)[1]
        moves, first, it = [0], None, 0
        while it < args.learn_max and first is None:
            s.run(100, record=False)
            it += 100
            moves.append(int(s.move_counts()[0]))
            if len(moves) > 5:
                acc = (moves[-1] - moves[-6]) / 500.0
                if 0.15 <= acc <= 0.35:
                    first = (it, acc)
        s.close()
        tail = f"first in [0.15, 0.35] after {first[0]} iterations (acceptance {first[1]:.3f} over the last 500)" if first else \
            f"not in [0.15, 0.35] within {args.learn_max} iterations (last window {(moves[-1] - moves[-6]) / 500.0:.3f})"
        print(f"learning from the {law} law (sqrt of the smallest / largest variance {np.sqrt(np.diag(cov).min()):.3g} / {np.sqrt(np.diag(cov).max()):.3g}): {tail}",
              flush=True)
    ctx.close()


for shape in args.shapes.split(","):
    leg(shape)

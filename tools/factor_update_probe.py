"""Learning-iteration time of the device engine against TAMCMC_OPT_FACTOR_REFRESH = R (rank-one steps of the proposal factor, a full
factorisation every R-th adapting iteration; R = 0: a full factorisation in every one, the default).

    python tools/factor_update_probe.py [repeats] [iterations per repeat] [--only-headline]

Headline shape: bench.py's learning leg -- 1e5 bins, 93 free variables, 20 chains, lambda = 1.3, the learning window open from iteration
100 on, records into pinned buffers.  Then the 153-variable star of tests/sampler_cases.py (6000 bins, 20 chains), whose adaptation works
in device memory.  One process, one sampler per R on one context, all of them warmed up (400 + 64 iterations) before the first timed
call; the timed calls are interleaved (R = 0, 8, 32, 128, 0, 8, ...), so drift of the clocks or of the machine's load hits every R
alike.  Reported per R: median, min and max of the repeats in us per learning iteration, and for R > 0 the median difference to R = 0
beside the spread (max - min) of R = 0's own repeats -- the yardstick: R = 0 in the same process is the default path.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry

pkg = entry.load_package()
import torch
from tamcmc_c_amd import synth

RS = (0, 8, 32, 128)


def spectrum(star, seed):
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_STRICT)
    ctx.set_spectrum(star.x, np.ones_like(star.x))
    _, m0, _ = ctx.loglike_params_batch(star.model_id, star.params, star.plength, want_model=True)
    y = star.set_spectrum_from_model(m0[0], seed=seed)
    ctx.set_option(pkg.OPT_PRECISION, pkg.PRECISION_FAST)
    ctx.set_spectrum(star.x, y)
    return ctx


def measure(label, star, ctx, chains, repeats, steps):
    samplers, bufs = {}, {}
    for R in RS:
        ctx.set_option(pkg.OPT_FACTOR_REFRESH, R)
        s = pkg.Sampler(ctx, star, nchains=chains, lambda_temp=1.3, seed=11, engine="device", Nt_learn=(100, 10**9), periods_learn=(1,),
                        dN_mixing=1, c0=2.0)
        ctx.set_option(pkg.OPT_FACTOR_REFRESH, 0)
        s.run(400, record=False)
        bufs[R] = (pkg.pinned_empty((steps, chains, s.nvars)), pkg.pinned_empty((steps, chains, 3)))
        s.run(64, out=(bufs[R][0][:64], bufs[R][1][:64]))
        samplers[R] = s
    times = {R: [] for R in RS}
    for _ in range(repeats):
        for R in RS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            samplers[R].run(steps, out=bufs[R])
            torch.cuda.synchronize()
            times[R].append(1e6 * (time.perf_counter() - t0) / steps)
    print("%s: %d variables, %d chains, %d bins, adaptation workspace in %s; %d repeats of %d learning iterations, us per iteration" %
          (label, samplers[0].nvars, chains, star.x.size, "LDS" if samplers[0].info()["adapt_in_lds"] else "device memory", repeats, steps))
    base = np.array(times[0])
    for R in RS:
        t = np.array(times[R])
        i = samplers[R].info()
        line = "  R = %3d: median %7.2f  min %7.2f  max %7.2f   (rank-one steps %d, scheduled full %d, forced full %d)" % (
            R, np.median(t), t.min(), t.max(), i["factor_updates"], i["factor_refreshes"], i["factor_refreshes_forced"])
        if R:
            line += "   median - median(R = 0) = %+.2f; spread of R = 0: %.2f" % (np.median(t) - np.median(base), base.max() - base.min())
        print(line)
    for s in samplers.values():
        s.close()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if len(args) > 0 else 5
    steps = int(args[1]) if len(args) > 1 else 1500
    star = synth.make_c3_star(seed=20240229, nx=100000, step=2000.0 / 100000)
    ctx = spectrum(star, 20240301)
    measure("headline", star, ctx, 20, repeats, steps)
    ctx.close()
    if "--only-headline" in sys.argv:
        return
    wide = synth.make_c3_star(seed=7, nx=6000, nmax=24, lmax=3, step=0.6, fmin=15 * 135.1 - 80.0)
    ctx = spectrum(wide, 1153)
    measure("wide", wide, ctx, 20, repeats, max(steps // 3, 100))
    ctx.close()


if __name__ == "__main__":
    main()

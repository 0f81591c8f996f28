"""Gaussian-envelope fits (model ids 0 / 1): iterations per second of the three routes that can run their random-walk chains -- the
host-driven engine, the device engine's lockstep kernels (TAMCMC_OPT_STEP_SCHEME = 1: k_iterate -> k_env_ksi / k_env_eval) and the
device engine's automatic routing (k_env_step, one launch per iteration, up to 32 768 bins for id 1 and 6 144 for id 0; the lockstep
kernels above).  A measurement tool, not a test.

The three routes alternate in one process, `--rounds` times; each turn runs at least `--seconds` of timed iterations after a warm-up, in
calls of `--call` iterations without records, and ends when the last call has returned (every call returns with the sampler's streams
idle).  No adaptation: the proposal law stays the initial one, so every route does the same work per iteration.  Printed per shape and
route: iterations/s as median [min, max] over the rounds, and which kernels ran (the engine's own counters).

Shapes: the 1161491 fixture (id 1, 5 380 bins), a 32 393-bin synthetic star, a 65 536-bin one (above the one-launch limit: the
automatic route is the lockstep route there), 10 chains each; `--nx` adds synthetic sizes (a scan for the crossover: DESIGN section 9
has id 0's, taken with the limit at 32 768 bins for both ids), `--model-id` picks the synthetic stars' model.

    python tools/envelope_engine_probe.py [--model-id 0|1] [--nx 8192,16384] [--no-fixture] [--no-default] [--chains 10] [--seconds 1.0] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUTES = (("host", "host", 0), ("device lockstep", "device", 1), ("device automatic", "device", 0))


def shapes(pkg, a):
    from tamcmc_c_amd import inputs, synth
    import envelope_numpy as en
    gold = os.path.join(ROOT, "tests", "golden", "envelope")
    out = []
    if not a.no_fixture:
        star, _ = inputs.load_simple_star(os.path.join(gold, "1161491_Gaussfit.model"), os.path.join(gold, "1161491_Gaussfit.data"), 1)
        out.append(("1161491 fixture (id 1)", star))
    for nx in ([] if a.no_default else [32393, 65536]) + a.nx:
        star = synth.make_envelope_star(a.model_id, nx=nx, seed=1)
        star.set_spectrum_from_model(np.asarray(en.model(a.model_id, star.params, star.x), dtype=np.float64), seed=101)
        out.append(("synthetic id %d" % a.model_id, star))
    return out


def turn(s, call, seconds):
    s.run(call, record=False)  # warm-up: buffers, first launches
    n, t0 = 0, time.perf_counter()
    while True:
        s.run(call, record=False)
        n += call
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-id", type=int, default=1)
    ap.add_argument("--nx", type=lambda v: [int(x) for x in v.split(",") if x], default=[])
    ap.add_argument("--chains", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--call", type=int, default=1000)
    ap.add_argument("--no-fixture", action="store_true")
    ap.add_argument("--no-default", action="store_true", help="only the --nx sizes")
    a = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    from tamcmc_c_amd import sampler
    for name, star in shapes(pkg, a):
        ctx = pkg.HipContext(0)
        ctx.set_spectrum(star.x, star.y)
        ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_ENGINE, 1)
        rates = {r[0]: [] for r in ROUTES}
        ran = {}
        for _ in range(a.rounds):
            for label, engine, scheme in ROUTES:
                ctx.set_option(pkg.OPT_STEP_SCHEME, scheme)
                s = sampler.Sampler(ctx, star, nchains=a.chains, lambda_temp=1.5, seed=7, Nt_learn=(10**9, 10**9 + 1), periods_learn=(1,),
                                    engine=engine)
                rates[label].append(turn(s, a.call, a.seconds))
                info = s.info()
                ran[label] = "k_env_step" if info["iter_fused"] else ("lockstep kernels" if info["engine"] else "host loop")
                s.close()
        ctx.close()
        res = {"shape": name, "bins": int(star.x.size), "chains": a.chains}
        for label, _, _ in ROUTES:
            v = sorted(rates[label])
            res[label] = {"iter_per_s": round(float(np.median(v)), 1), "min": round(v[0], 1), "max": round(v[-1], 1), "ran": ran[label]}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

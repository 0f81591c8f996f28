"""Gaussian-envelope fits (model ids 0 / 1): iterations per second of the three routes that can run their Langevin chains -- the
host-driven engine with the brute-force gradient batch (TAMCMC_OPT_ENVELOPE_GRADIENT = 0), the host-driven engine with the analytic
gradient (= 1), and the device-resident engine (TAMCMC_OPT_ENVELOPE_DEVICE_LANGEVIN = 1: k_mala_settle -> k_env_mala_front -> the
analytic kernels -> k_env_mala_chain -> k_mala_test, nothing crossing PCIe inside an iteration).  A measurement tool, not a test.

The three routes alternate in one process on one context, `--rounds` times; each turn runs at least `--seconds` of timed iterations
after a warm-up call, in calls of `--call` iterations without records, and ends when the last call has returned (every call returns
with the sampler's streams idle).  No adaptation: the proposal law stays the initial one, so every route does the same work per
iteration.  Printed per shape and route: iterations/s as median [min, max] over the rounds, and whether the device route's median
exceeds the maximum of either host route -- the baseline is the host engine's figure of the same process, never an earlier session's.

Shapes: the 1161491 fixture (id 1, 5 380 bins, 10 chains), synthetic id 0 at 5 400 and 32 393 bins (10 chains), synthetic id 1 at 10^6
bins with 20 chains.

    python tools/envelope_mala_probe.py [--seconds 1.0] [--rounds 3] [--call 200] [--only fixture,id0-5400,id0-32393,id1-1000000]
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

ROUTES = (("host, brute-force gradient", "host", 0), ("host, analytic gradient", "host", 1), ("device", "device", 1))


def shapes(only):
    from tamcmc_c_amd import inputs, synth
    import envelope_numpy as en
    gold = os.path.join(ROOT, "tests", "golden", "envelope")
    out = []
    if not only or "fixture" in only:
        star, _ = inputs.load_simple_star(os.path.join(gold, "1161491_Gaussfit.model"), os.path.join(gold, "1161491_Gaussfit.data"), 1)
        out.append(("1161491 fixture (id 1)", star, 10))
    for model_id, nx, chains in ((0, 5400, 10), (0, 32393, 10), (1, 10**6, 20)):
        if only and "id%d-%d" % (model_id, nx) not in only:
            continue
        star = synth.make_envelope_star(model_id, nx=nx, seed=1)
        star.set_spectrum_from_model(np.asarray(en.model(model_id, star.params, star.x), dtype=np.float64), seed=101)
        out.append(("synthetic id %d" % model_id, star, chains))
    return out


def turn(s, call, seconds):
    s.run(call, record=False)  # warm-up: buffers, first launches, the initial gradient
    n, t0 = 0, time.perf_counter()
    while True:
        s.run(call, record=False)
        n += call
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--call", type=int, default=200)
    ap.add_argument("--only", type=lambda v: [x for x in v.split(",") if x], default=[])
    a = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    from tamcmc_c_amd import sampler
    for name, star, chains in shapes(a.only):
        ctx = pkg.HipContext(0)
        ctx.set_spectrum(star.x, star.y)
        ctx.set_option(pkg.OPT_ENVELOPE_DEVICE_LANGEVIN, 1)
        rates = {r[0]: [] for r in ROUTES}
        for _ in range(a.rounds):
            for label, engine, analytic in ROUTES:
                ctx.set_option(pkg.OPT_ENVELOPE_GRADIENT, analytic)
                s = sampler.Sampler(ctx, star, nchains=chains, lambda_temp=1.5, seed=7, use_drift=1, Nt_learn=(10**9, 10**9 + 1),
                                    periods_learn=(1,), engine=engine)
                rates[label].append(turn(s, a.call, a.seconds))
                s.close()
        ctx.close()
        res = {"shape": name, "bins": int(star.x.size), "chains": chains}
        for label, _, _ in ROUTES:
            v = sorted(rates[label])
            res[label] = {"iter_per_s": round(float(np.median(v)), 1), "min": round(v[0], 1), "max": round(v[-1], 1)}
        host_max = max(res[ROUTES[0][0]]["max"], res[ROUTES[1][0]]["max"])
        res["device median exceeds the host routes' maximum"] = bool(res["device"]["iter_per_s"] > host_max)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

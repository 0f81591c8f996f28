"""A device Langevin sampler whose context changes the route of its gradient batch (csrc/fd_route.h) between two calls: run_mala lays the
batch out again when the route differs from the one it holds (csrc/dev_sampler.hip) and starts from a gradient taken on the new route."""
import math

import numpy as np
import pytest

from test_gpu_adjoint import _constrained_star

pytestmark = pytest.mark.gpu


def test_device_langevin_sampler_follows_the_route_between_calls(pkg, oracle, synth):
    """The C2 slice with every multiplet inside its 11 000 bins, 5 chains, FAST at 64x8, one sampler: 3 iterations under each of windowed ->
    brute force (TAMCMC_OPT_FD_WINDOWED 0) -> adjoint (TAMCMC_OPT_GRADIENT) -> windowed.  After each, the gradient the sampler holds is the
    direct call's under the same options at the held positions, with the construction and the tolerance of
    test_gpu_adjoint.test_device_langevin_engine_follows_the_host_engine_under_the_option (rtol 1e-7, atol 1e-7 max|g|, valid chains only,
    at least one), and the recorded statistics are finite."""
    star = _constrained_star(oracle, synth)
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST, workgroup=64, bins_per_thread=8)
    try:
        ctx.set_spectrum(star.x, star.y)
        d = pkg.Sampler(ctx, star, engine="device", use_drift=1, nchains=5, lambda_temp=1.5, seed=21, Nt_learn=(20, 60), periods_learn=(1,),
                        c0=3.0, dN_mixing=1)
        T = np.array([math.pow(1.5, m) for m in range(5)])
        routes = (("windowed", 1, pkg.GRADIENT_FD), ("brute", 0, pkg.GRADIENT_FD), ("adjoint", 0, pkg.GRADIENT_ADJOINT),
                  ("windowed", 1, pkg.GRADIENT_FD))
        for name, windowed, gradient in routes:
            ctx.set_option(pkg.OPT_FD_WINDOWED, windowed)
            ctx.set_option(pkg.OPT_GRADIENT, gradient)
            _, stt = d.run(3, stats=True)
            g, gp, valid = d.gradient()
            held = np.tile(star.params, (5, 1))
            held[:, star.index_to_relax] = d.state()["vars"]
            hs = 1e-7 * np.maximum(np.abs(d.get_proposal(0)[0]), 1e-3)
            _, _, g_direct = ctx.fd_gradient_posterior(star, held, hs, T)
            v = np.flatnonzero(valid)
            err = np.abs(g[v] - g_direct[v]) - 1e-7 * np.abs(g_direct[v])
            print("\n%s: %d valid chains, max |g| %.3e, max (|dg| - rtol |g|) %.3e against atol %.3e" %
                  (name, v.size, np.abs(g_direct).max(), err.max() if v.size else float("nan"), 1e-7 * np.abs(g_direct).max()))
            assert np.all(np.isfinite(stt)), name
            assert v.size and np.allclose(g[v], g_direct[v], rtol=1e-7, atol=1e-7 * np.abs(g_direct).max()), name
        d.close()
    finally:
        ctx.close()


def test_device_langevin_sampler_at_a_geometry_without_the_delta_kernel(pkg, oracle, synth):
    """The same star and sampler at 64 x 16, where the likelihood kernel has no DELTA variant: the batch of a windowed request takes the
    brute-force route (fd_route.h).  Five iterations; the held gradient against the direct call at the held positions, constructed and
    bounded as above -- the direct call takes the same route, and with TAMCMC_OPT_FD_WINDOWED = 0 it returns the same bits."""
    star = _constrained_star(oracle, synth)
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST, workgroup=64, bins_per_thread=16)
    try:
        ctx.set_spectrum(star.x, star.y)
        d = pkg.Sampler(ctx, star, engine="device", use_drift=1, nchains=5, lambda_temp=1.5, seed=21, Nt_learn=(20, 60), periods_learn=(1,),
                        c0=3.0, dN_mixing=1)
        T = np.array([math.pow(1.5, m) for m in range(5)])
        _, stt = d.run(5, stats=True)
        g, gp, valid = d.gradient()
        held = np.tile(star.params, (5, 1))
        held[:, star.index_to_relax] = d.state()["vars"]
        hs = 1e-7 * np.maximum(np.abs(d.get_proposal(0)[0]), 1e-3)
        _, _, g_direct = ctx.fd_gradient_posterior(star, held, hs, T)
        ctx.set_option(pkg.OPT_FD_WINDOWED, 0)
        _, _, g_brute = ctx.fd_gradient_posterior(star, held, hs, T)
        v = np.flatnonzero(valid)
        err = np.abs(g[v] - g_direct[v]) - 1e-7 * np.abs(g_direct[v])
        print("\n64 x 16: %d valid chains, max |g| %.3e, max (|dg| - rtol |g|) %.3e against atol %.3e" %
              (v.size, np.abs(g_direct).max(), err.max() if v.size else float("nan"), 1e-7 * np.abs(g_direct).max()))
        assert np.all(np.isfinite(stt))
        assert v.size and np.allclose(g[v], g_direct[v], rtol=1e-7, atol=1e-7 * np.abs(g_direct).max())
        assert np.array_equal(g_direct, g_brute)
        assert d.info()["iter_lockstep"] == 5
        d.close()
    finally:
        ctx.close()

"""Posterior model spectrum on the GPU (tamcmc_hip_model_stats_*, csrc/model_stats.hip): the handle's results against the sequential
numpy replay of the accumulator law (tests/model_stats_numpy.py) over the STRICT model rows tamcmc_hip_loglike_params_batch writes for
the same vectors -- bit for bit, in every arithmetic mode and tile geometry of the context, for every chunking of the stream.

Small stars from synth.py; the vectors are the star's parameters with the free ones jittered.  `SMALL` is make_c3_star(nx=1000, nmax=4)
on a grid that holds its modes (0.6 muHz bins from 2000 muHz: windows that begin and end inside the spectrum); the first test also takes
the builder's own grid, 1950 .. 1970 muHz, which lies below every mode (all windows cover the whole spectrum)."""
import numpy as np
import pytest

import model_stats_numpy as msn
import strict_numpy

pytestmark = pytest.mark.gpu

GEOMS = [(256, 1), (256, 2), (256, 4), (64, 4), (64, 8), (64, 16)]   # every accepted (TAMCMC_OPT_WORKGROUP, _BINS_PER_THREAD)
B13 = 13
SMALL = dict(nx=1000, nmax=4, step=0.6, fmin=2000.0)


def jitter(star, B, seed, rel=2e-4):
    rng = np.random.default_rng(seed)
    P = np.tile(star.params, (B, 1))
    idx = star.index_to_relax
    P[:, idx] *= 1.0 + rel * rng.standard_normal((B, idx.size))
    return P


def open_ctx(pkg, star, precision=0, geom=None, seed=3):
    """A context holding the star's grid and (once per star) data drawn around its own STRICT model."""
    ctx = pkg.HipContext(0, precision=precision)
    if geom:
        ctx.set_option(pkg.OPT_WORKGROUP, geom[0])
        ctx.set_option(pkg.OPT_BINS_PER_THREAD, geom[1])
    if star.y is None:
        ctx.set_spectrum(star.x, np.ones_like(star.x))
        _, m0, st = ctx.loglike_params_batch(star.model_id, star.params, star.plength, want_model=True)
        assert st[0] == 0
        star.set_spectrum_from_model(m0[0], seed)
    ctx.set_spectrum(star.x, star.y)
    return ctx


def zero_hv_rows(pkg, ctx, star, P):
    """Model rows of the vectors' own host tables with every hv zeroed: the background alone, summed by the likelihood kernel's statements."""
    stride = max(int(star.plength[8]), 1)
    mults, offs, noise, nhs, nns = [], [0], np.zeros((len(P), stride)), [], []
    for b, p in enumerate(P):
        st, m, nz, nh = pkg.build_mode_table(star.model_id, p, star.plength, star.x)
        assert st == 0
        m = m.copy()
        m["hv"][:] = 0.0
        mults.append(m); offs.append(offs[-1] + len(m)); noise[b, :nz.size] = nz; nhs.append(nh); nns.append(nz.size)
    _, rows = ctx.loglike_batch(np.concatenate(mults), offs, noise, nhs, nns, want_model=True)
    return rows


def expected(pkg, star, P, weights=None, background=True):
    """(replay over the STRICT rows of P, the rows, the status): computed on a STRICT context of default geometry."""
    ctx = open_ctx(pkg, star)
    _, rows, status = ctx.loglike_params_batch(star.model_id, P, star.plength, want_model=True)
    good = status == 0
    bg = None
    if background:
        bg = np.zeros_like(rows)
        bg[good] = zero_hv_rows(pkg, ctx, star, P[good])
    ctx.close()
    return msn.replay(rows, y=star.y, weights=weights, bg_rows=bg, status=status), rows, status


def run(ctx, star, P, weights=None, chunk=0, calls=None):
    ms = ctx.model_stats(star, chunk=chunk)
    lo = 0
    for n in (calls or [len(P)]):
        ms.add_params(P[lo:lo + n], None if weights is None else weights[lo:lo + n])
        lo += n
    res = ms.result()
    ms.close()
    return res


def same(res, ref, what=""):
    for k in msn.KEYS:
        if ref[k] is not None:
            assert np.array_equal(res[k], ref[k], equal_nan=True), (what, k, float(np.nanmax(np.abs(res[k] - ref[k]))))
    assert res["W"] == ref["W"] and res["counts"] == ref["counts"], (what, res["W"], ref["W"], res["counts"], ref["counts"])


@pytest.fixture(scope="module")
def small(pkg, synth):
    """The small C3 star (id 23), 13 jittered vectors, their replay: computed once, shared, left unchanged."""
    star = synth.make_c3_star(**SMALL)
    P = jitter(star, B13, 11)
    ref, rows, status = expected(pkg, star, P)
    assert (status == 0).all()
    return star, P, ref, rows


@pytest.mark.parametrize("grid", ["modes inside", "builder's grid"])
def test_bitwise_replay_in_every_arithmetic_mode(pkg, synth, small, grid):
    """1. mean, var, min, max, ratio bit for bit the replay over the STRICT rows; background the replay over the zero-hv rows; a FAST and
    a FAST_DIRECT context give the STRICT context's bits."""
    if grid == "modes inside":
        star, P, ref, _ = small
    else:
        star = synth.make_c3_star(nx=1000, nmax=4)
        P = jitter(star, B13, 12)
        ref, _, _ = expected(pkg, star, P)
    assert ref["counts"] == (B13, 0, 0) and ref["var"].max() > 0
    for prec in (pkg.PRECISION_STRICT, pkg.PRECISION_FAST, pkg.PRECISION_FAST_DIRECT):
        ctx = open_ctx(pkg, star, prec)
        same(run(ctx, star, P), ref, prec)
        ctx.close()


def test_independent_parity(pkg, small):
    """2. Mean and envelope against strict_numpy.eval_table on build_mode_table rows.  A STRICT model row with active Harvey terms lies
    within 1e-15 relative per bin of the host restatement (tests/test_gpu_parity.py:105 and :110, `("strict", 1e-15, ...)`: device pow
    against libm); min and max are 1-Lipschitz in the rows, and the mean adds the law's own (n + 2) 2^-53 max|M|
    (tests/test_model_stats_reference.py) to that."""
    star, P, _, _ = small
    rows = []
    for p in P:
        st, m, nz, nh = pkg.build_mode_table(star.model_id, p, star.plength, star.x)
        assert st == 0
        rows.append(strict_numpy.eval_table(m, nz, nh, star.x))
    rows = np.array(rows)
    ctx = open_ctx(pkg, star)
    res = run(ctx, star, P)
    ctx.close()
    top = rows.max(axis=0)
    mean = np.asarray(np.mean(rows.astype(np.longdouble), axis=0), dtype=np.float64)
    em, en, ex = np.abs(res["mean"] - mean), np.abs(res["min"] - rows.min(axis=0)), np.abs(res["max"] - top)
    print("parity / bound: mean %.3g min %.3g max %.3g" % (np.max(em / ((1e-15 + (B13 + 3) * 2.0 ** -53) * top)), np.max(en / (1e-15 * top)),
                                                           np.max(ex / (1e-15 * top))))
    assert np.all(em <= (1e-15 + (B13 + 3) * 2.0 ** -53) * top)  # (+1: the reference mean's own rounding to double)
    assert np.all(en <= 1e-15 * top) and np.all(ex <= 1e-15 * top)


@pytest.mark.parametrize("asym", [0.0, 25.0])
@pytest.mark.parametrize("nx", [100, 257, 1000])
def test_geometry(pkg, synth, nx, asym):
    """3. Below one tile of 256 bins, one bin over it, several tiles with a ragged end; truncation parameter 3 on 2060 .. 2360 muHz: the
    l = 2 multiplet at 2072 muHz has its window clipped at the first bin, l = 0 at 2351 muHz at the last, the four multiplets above
    2399 muHz lie wholly outside the spectrum (the builder leaves them a stub window at the last bins; at 257 bins it straddles the
    tile edge); l = 0 .. 3 with and without asymmetry; every workgroup geometry of the context."""
    star = synth.make_c3_star(nx=nx, nmax=4, step=300.0 / nx, fmin=2060.0)
    star.params[int(star.plength[:9].sum()) + 1] = 3.0          # Truncation_parameter
    star.params[star.names.index("Lorentzian_asymetry")] = asym
    st, m, _, _ = pkg.build_mode_table(star.model_id, star.params, star.plength, star.x)
    assert st == 0 and sorted(set(m["l"].tolist())) == [0, 1, 2, 3] and (m["asym"] == asym).all()
    assert ((m["i0"] == 0) & (m["i1"] < nx)).any() and ((m["i0"] > 0) & (m["i1"] == nx) & (m["fc"] < star.x[-1])).any()
    assert (m["fc"] > star.x[-1]).sum() >= 4
    P = jitter(star, 5, 100 + nx)
    ref, _, status = expected(pkg, star, P)
    assert (status == 0).all()
    for geom in GEOMS:
        ctx = open_ctx(pkg, star, pkg.PRECISION_FAST if geom[0] == 64 else pkg.PRECISION_STRICT, geom)
        same(run(ctx, star, P), ref, geom)
        ctx.close()


def test_chunking_and_streaming(pkg, small):
    """4. chunk = 5 in one call, three calls of 4, 4 and 5 vectors, and a repeat after reset: the bits of chunk = 0, one call."""
    star, P, ref, _ = small
    ctx = open_ctx(pkg, star)
    same(run(ctx, star, P), ref, "one call")
    same(run(ctx, star, P, chunk=5), ref, "chunk 5")
    same(run(ctx, star, P, calls=[4, 4, 5]), ref, "three calls")
    ms = ctx.model_stats(star, chunk=5)
    ms.add_params(P[::-1])
    ms.reset()
    with pytest.raises(pkg.TamcmcError) as e:
        ms.result()
    assert e.value.code == pkg.ERR_BAD_ARG
    ms.add_params(P)
    same(ms.result(), ref, "after reset")
    ms.close()
    ctx.close()


def test_weights(pkg, small):
    """5. Zero-weight vectors (first position included) change nothing but their count; W and counts; a negative or NaN weight is
    refused and leaves the handle as it was."""
    star, P, _, rows = small
    w = np.random.default_rng(5).uniform(0.5, 2.0, B13)
    w[[0, 4, 12]] = 0.0
    keep = w > 0
    ref_all, _, _ = expected(pkg, star, P, weights=w)
    ref_kept, _, _ = expected(pkg, star, P[keep], weights=w[keep])
    assert ref_all["counts"] == (10, 0, 3) and ref_kept["counts"] == (10, 0, 0)
    ctx = open_ctx(pkg, star)
    res_all, res_kept = run(ctx, star, P, w, chunk=4), run(ctx, star, P[keep], w[keep])
    same(res_all, ref_all, "with zeros")
    same(res_kept, ref_kept, "without")
    for k in msn.KEYS:
        assert np.array_equal(res_all[k], res_kept[k]), k
    W = 0.0
    for v in w[keep]:
        W = W + v
    assert res_all["W"] == W
    ms = ctx.model_stats(star)
    ms.add_params(P[:6], w[:6])
    before = ms.result()
    for bad in (-1.0, np.nan, np.inf):
        wb = np.ones(7)
        wb[5] = bad
        with pytest.raises(pkg.TamcmcError) as e:
            ms.add_params(P[6:], wb)
        assert e.value.code == pkg.ERR_BAD_ARG
    same(ms.result(), before, "after refused weights")
    ms.close()
    ctx.close()


@pytest.mark.parametrize("model_id", [23, 25])
def test_failed_tables_are_skipped_and_counted(pkg, synth, small, model_id):
    """6. A vector with a NaN frequency is skipped and counted; the rest is the batch without it, bit for bit.  Id 25: the NaN sits in an
    l = 2 frequency, which only the device's row builder sees -- the status the kernel reads is the device's."""
    if model_id == 23:
        star, P = small[0], small[1].copy()
        bad_at = star.names.index("Frequency_l") + 2
    else:
        star = synth.make_c5_star(nx=3000, nmax=5, nferr=4)
        P = jitter(star, 7, 25, rel=1e-5)
        bad_at = int(np.sum(star.plength[:4]))  # first l = 2 frequency
    P[0, bad_at] = np.nan     # first position: the reference plane must come from the first ACCEPTED vector
    P[3, bad_at] = np.nan
    ref, _, status = expected(pkg, star, P, background=False)
    assert status[0] != 0 and status[3] != 0 and (np.delete(status, [0, 3]) == 0).all()
    good = status == 0
    ctx = open_ctx(pkg, star)
    res, res_good = run(ctx, star, P, chunk=3), run(ctx, star, P[good])
    ctx.close()
    same(res, ref, "with failed vectors")
    assert res["counts"] == (len(P) - 2, 2, 0) and res_good["counts"] == (len(P) - 2, 0, 0)
    for k in msn.KEYS:
        assert np.array_equal(res[k], res_good[k]), k
    assert np.isfinite(res["mean"]).all()


def test_add_vars_takes_a_sampler_record_in_place(pkg, synth):
    """7. Chain 0 of a 6-iteration record of a 3-chain sampler, passed with its stride, against add_params on the scattered vectors."""
    star = synth.make_c2_star(nx=2000)
    ctx = open_ctx(pkg, star, pkg.PRECISION_FAST)
    smp = pkg.Sampler(ctx, star, nchains=3)
    rec, _ = smp.run(6)
    smp.close()
    assert rec.shape == (6, 3, star.nvars)
    P = np.tile(star.params, (6, 1))
    P[:, star.index_to_relax] = rec[:, 0, :]
    ref = run(ctx, star, P)
    w = np.array([1.0, 0.5, 2.0, 0.0, 1.0, 3.0])
    for weights in (None, w):
        ms = ctx.model_stats(star, chunk=4)
        ms.add_vars(rec, chain=0, weights=weights)
        got = ms.result()
        ms.close()
        same(got, ref if weights is None else run(ctx, star, P, w), "record in place")
    ms = ctx.model_stats(star)
    ms.add_vars(np.ascontiguousarray(rec[:, 0, :]))
    same(ms.result(), ref, "2-D rows")
    ms.close()
    other = ctx.model_stats(star)
    other.add_vars(rec, chain=1)
    assert not np.array_equal(other.result()["mean"], ref["mean"])
    other.close()
    no_relax = ctx.model_stats(star.model_id, star.params, star.plength)   # created without relax: add_params only
    no_relax.Nvars = star.nvars
    with pytest.raises(pkg.TamcmcError) as e:
        no_relax.add_vars(rec)
    assert e.value.code == pkg.ERR_BAD_ARG
    no_relax.close()
    ctx.close()


def _v3_star(synth):
    s = synth.make_classic_star(**SMALL)
    p, pl = synth.classic_to_v3(s.params, s.plength)
    o = int(s.plength[:9].sum())
    relax = np.concatenate([s.relax[:o], np.ones(p.size - s.params.size + 1, dtype=np.int32), s.relax[o + 1:]])
    return synth.Star(13, p, pl, s.x, relax, np.zeros((4, p.size)), np.zeros(p.size, dtype=np.int32), None, prior_class=2)


STARS = {3: lambda s: s.make_classic_star(**SMALL), 11: lambda s: s.make_c2_star(nx=2000), 12: lambda s: s.make_v2_star(**SMALL),
         13: _v3_star, 14: lambda s: s.make_hnlm_star(nx=2000), 23: lambda s: s.make_c3_star(**SMALL),
         25: lambda s: s.make_c5_star(nx=3000, nmax=5, nferr=4), 27: lambda s: s.make_c5_star(nx=3000, nmax=5, nferr=4, cte_width=True)}


@pytest.mark.parametrize("model_id", sorted(STARS))
def test_every_model_id(pkg, synth, model_id):
    """8. Each table model at its smallest synthetic star against the replay over its own STRICT rows (ids 25 / 27: make_c5_star at
    nx=3000, nmax=5, nferr=4, the smallest the red-giant GPU tests use; their tables exist on the device only, so no zero-hv rows: the
    background of these two is held to its definition instead -- no larger than the envelope's floor, and the same for both widths' star)."""
    star = STARS[model_id](synth)
    assert star.model_id == model_id
    P = jitter(star, 6, 40 + model_id, rel=1e-5 if model_id in (25, 27) else 2e-4)
    host_tables = model_id not in (25, 27)
    ref, _, status = expected(pkg, star, P, background=host_tables)
    assert (status == 0).all()
    ctx = open_ctx(pkg, star, pkg.PRECISION_FAST)
    res = run(ctx, star, P, chunk=4)
    ctx.close()
    same(res, ref, model_id)
    assert (res["var"] > 0).any() and np.all(res["min"] <= res["mean"]) and np.all(res["mean"] <= res["max"])
    if not host_tables:
        assert np.all(res["background"] > 0) and np.all(res["background"] <= res["max"])


@pytest.mark.parametrize("model_id", [0, 1])
def test_envelope_models_are_out_of_scope(pkg, synth, model_id):
    star = synth.make_envelope_star(model_id, nx=64)
    ctx = pkg.HipContext(0)
    ctx.set_spectrum(star.x, np.ones_like(star.x))
    with pytest.raises(pkg.TamcmcError) as e:
        ctx.model_stats(star)
    assert e.value.code == pkg.ERR_BAD_MODEL
    ctx.close()


def test_error_contract(pkg, synth, small):
    """9. No spectrum; get on an empty handle; Nx changed after creation; chunk > 65535."""
    star, P, ref, _ = small
    bare = pkg.HipContext(0)
    with pytest.raises(pkg.TamcmcError) as e:
        bare.model_stats(star)
    assert e.value.code == pkg.ERR_NO_SPECTRUM
    bare.close()
    ctx = open_ctx(pkg, star)
    with pytest.raises(pkg.TamcmcError) as e:
        ctx.model_stats(star, chunk=65536)
    assert e.value.code == pkg.ERR_BAD_ARG
    ctx.model_stats(star, chunk=65535).close()
    ms = ctx.model_stats(star)
    with pytest.raises(pkg.TamcmcError) as e:
        ms.result()
    assert e.value.code == pkg.ERR_BAD_ARG
    ms.add_params(P)
    same(ms.result(), ref)
    ctx.set_spectrum(star.x[:900], star.y[:900])
    for call in (lambda: ms.add_params(P), ms.result):
        with pytest.raises(pkg.TamcmcError) as e:
            call()
        assert e.value.code == pkg.ERR_BAD_ARG
    ctx.set_spectrum(star.x, star.y)   # the length it was created for: the planes are intact
    same(ms.result(), ref, "after the spectrum came back")
    ms.close()
    ctx.close()

"""The likelihood tile against its 50-digit reference (-m gpu): every bin of every directed case (tile_cases.py) through
HipContext.loglike_batch(want_model=True) in STRICT, FAST_DIRECT and FAST, with the numpy.longdouble twin of tile_reference.py as M.

Per bin:
    STRICT       |dM| <= K_STRICT 2^-53 M
    FAST_DIRECT  |dM| <= 1e-12 M                                    (the header's statement: no far field, no background series)
    FAST         |dM| <= 1e-12 M + TAU_FAR F(x) + TAU_ASYM F_asym(x)   (F: sum of the |far components| at the bin, by the far rule restated
                                                                     in tile_reference.py; the two taus are pinned by test_tile_bounds.py)
logL, relative to the reference's: 1e-12 (STRICT), 1e-11 (both FAST modes).
Which path a tile took is observable: FAST and FAST_DIRECT run the same near-field and per-bin background code, so their rows are equal
bit for bit on a tile with no far row and no background series, and differ on a tile that has either.  That pins the far gate and the
gate of the background series from both sides.
Every case runs at both geometries of its tile size (one wave x 4, 8, 16 bins per lane; four waves x 1, 2, 4), and which geometry took a
bin must not show where the arithmetic is stated per bin: test_rows_do_not_show_the_geometry.
"""
import numpy as np
import pytest

import tile_cases as tc
import tile_reference as tr
from tile_series import TAU_ASYM, TAU_FAR

pytestmark = pytest.mark.gpu

# STRICT keeps the reference's operation order in double: its distance from the exact row is the reference's own rounding.  Worst
# |dM| / (2^-53 M) over every bin of every case here and of test_gpu_parity.py::test_random_tables_on_awkward_grids, measured on the
# MI355X: r = 111.67 (far_gate, tiles of 256 bins, "l0 asym+30 A1000 far": an asymmetric row 51 muHz from nu_c, where x / nu_c - 1
# is formed from a rounded quotient and multiplied by asym = 30; the other cases stay below: 48.3 the random tables, 13.1 the
# background case, 10.2 the windows case, 7.2 the common denominator, 4.9 the early stop, 3.5 the wing, 2.5 the narrow modes).
# K_STRICT = 4 r, the margin of the log-prior's parity test.
STRICT_WORST_RATIO = 111.67
K_STRICT = 4.0 * STRICT_WORST_RATIO
FAST_TOL = 1e-12
U = 2.0 ** -53

# (workgroup, bins per thread): tiles of 512, 1024, 256 bins from the one-wave / four-wave kernel, then the other kernel's tile of each size
GEOMS = ((64, 8), (256, 4), (64, 4), (256, 1), (256, 2), (64, 16))
PAIRS = (((64, 4), (256, 1)), ((64, 8), (256, 2)), ((64, 16), (256, 4)))   # the two geometries of each tile size: 256, 512, 1024 bins
PARAMS = [(wg, K, c.name) for wg, K in GEOMS for c in tc.cases(wg * K)]


@pytest.fixture(scope="module")
def ctxs(pkg):
    assert pkg.MULT_DTYPE == tc.MULT_DTYPE
    c = {"strict": pkg.HipContext(0, precision=pkg.PRECISION_STRICT), "fast": pkg.HipContext(0, precision=pkg.PRECISION_FAST),
         "fast_direct": pkg.HipContext(0, precision=pkg.PRECISION_FAST_DIRECT)}
    yield c
    for v in c.values():
        v.close()


def run_modes(pkg, ctxs, case, ref, wg, K, p=1.0):
    """{mode: (logL, model)}: one launch per mode with every evaluation of the case."""
    mults, offsets, noise, nhs, nns = case.launch_args()
    out = {}
    for name, c in ctxs.items():
        c.set_option(pkg.OPT_WORKGROUP, wg)
        c.set_option(pkg.OPT_BINS_PER_THREAD, K)
        c.set_spectrum(case.x, ref.y)
        out[name] = c.loglike_batch(mults, offsets, noise, nhs, nns, ref.T, p, want_model=True)
    return out


def check_rows(label, got, M, F, Fa):
    """The three per-bin assertions for one evaluation; returns STRICT's worst ratio.  Every figure is printed before it is asserted."""
    err = {k: np.abs(v.astype(tr.LD) - M) for k, v in got.items()}
    r_strict = float(np.max(err["strict"] / (U * M)))
    r_direct = float(np.max(err["fast_direct"] / M))
    bound = FAST_TOL * M + TAU_FAR * F + TAU_ASYM * Fa
    r_fast = float(np.max(err["fast"] / bound))
    r_fast_m = float(np.max(err["fast"] / M))
    print("%-44s STRICT %7.2f ulp | FAST_DIRECT %.2e | FAST %.2e of M, %.3f of its bound" % (label, r_strict, r_direct, r_fast_m, r_fast))
    for k, v in got.items():
        assert np.all(np.isfinite(v)), (label, k)
    assert r_strict <= K_STRICT, (label, r_strict)
    assert r_direct <= FAST_TOL, (label, r_direct, int(np.argmax(err["fast_direct"] / M)))
    assert r_fast <= 1.0, (label, r_fast, r_fast_m, int(np.argmax(err["fast"] / bound)))
    return r_strict


def check_logl(label, got, ref_l):
    for name, tol in (("strict", 1e-12), ("fast_direct", 1e-11), ("fast", 1e-11)):
        e = abs(float((tr.LD(got[name]) - ref_l) / ref_l))
        print("%-44s logL %-11s %.2e" % (label, name, e))
        assert e <= tol, (label, name, e)


def check_paths(case, b, fast, direct):
    """FAST == FAST_DIRECT bit for bit on the tiles that have neither a far row nor the background series; not equal on the others."""
    rows, noise, nh, nn = case.evals[b]
    far_tiles = {t for _, t in tr.far_map(rows, case.nx, case.tile_bins, case.x0, case.step)}
    for t in range(case.ntiles):
        sl = slice(t * case.tile_bins, min((t + 1) * case.tile_bins, case.nx))
        xc, h = case.geometry(t)
        series = nh > 0 and any(noise[3 * k + 1] != 0.0 for k in range(nh)) and tr.series_gate(noise, nh, xc, h)
        same = np.array_equal(fast[sl], direct[sl])
        if t in far_tiles or series:
            if sl.stop - sl.start >= 64:   # (the ragged last tile has three bins: they may well agree)
                assert not same, (case.name, case.labels[b], t, "the tile polynomial was not used")
        else:
            assert same, (case.name, case.labels[b], t, "a tile without far row or series differs from FAST_DIRECT")


@pytest.mark.parametrize("wg,K,name", PARAMS)
def test_directed_case(pkg, ctxs, wg, K, name):
    ref = tc.reference(wg * K, name)
    case = ref.case
    out = run_modes(pkg, ctxs, case, ref, wg, K)
    worst = 0.0
    for b in range(len(case.evals)):
        label = "%s/%d %s" % (name, wg * K, case.labels[b])
        got = {k: v[1][b] for k, v in out.items()}
        worst = max(worst, check_rows(label, got, ref.M[b], ref.F[b], ref.Fa[b]))
        check_logl(label, {k: v[0][b] for k, v in out.items()}, ref.logL[1][b])
        check_paths(case, b, got["fast"], got["fast_direct"])
    print("STRICT worst ratio of %s/%d: %.2f" % (name, wg * K, worst))


@pytest.mark.parametrize("tile_bins,name", [(tb, c.name) for tb in (256, 512, 1024) for c in tc.cases(tb)])
def test_rows_do_not_show_the_geometry(pkg, ctxs, tile_bins, name):
    """STRICT is the reference's operation order PER BIN (strict_mult and the STRICT branch of likelihood_terms, loglike_tile.h: rows in
    table order, one IEEE operation per statement, no value of the tile in any of them), so which lane of which workgroup takes a bin must
    not show: every case's STRICT row is the same bits at all six geometries -- the two kernels at each tile size and the three tile sizes.
    FAST_DIRECT is guaranteed less, and that is asserted: its per-bin argument is formed from the bin's offset to the TILE CENTRE
    (fast_mult: t = fma(x - x_c, 2/gamma, -A_m) with A_m staged per tile) and the common-denominator branch is chosen from a bound on the
    tile (F_SAFE), so the row depends on the tile's bins -- but on nothing else of the geometry: the two geometries of one tile size
    (64x4 / 256x1, 64x8 / 256x2, 64x16 / 256x4) stage the same scalars and run the same statements per bin, and the library is built
    without contraction (every fused operation is an explicit fma).  Their rows are equal bit for bit; across tile sizes they are not
    claimed equal (x_c differs: roundings of ~1e-16 t) and not compared.  FAST adds sums over lanes (the tile polynomial's coefficients
    are reduced over WGS / 16 parts in an order that follows the workgroup size): no equality is claimed for it."""
    ref = tc.reference(tile_bins, name)
    case = ref.case
    strict, direct = {}, {}
    for wg, K in GEOMS:
        out = run_modes(pkg, {k: ctxs[k] for k in ("strict", "fast_direct")}, case, ref, wg, K)
        strict[wg, K], direct[wg, K] = out["strict"][1], out["fast_direct"][1]
    first = strict[GEOMS[0]]
    assert np.all(np.isfinite(first))
    for geom in GEOMS[1:]:
        diff = np.argwhere(strict[geom] != first)
        assert diff.size == 0, ("STRICT", name, tile_bins, GEOMS[0], geom, len(diff), diff[:4].tolist())
    for ga, gb in PAIRS:
        diff = np.argwhere(direct[ga] != direct[gb])
        assert diff.size == 0, ("FAST_DIRECT", name, tile_bins, ga, gb, len(diff), diff[:4].tolist())


def test_far_rows_take_the_polynomial_and_near_rows_do_not(pkg, ctxs):
    """The gate from both sides, by name: 1e-3 inside it the row joins the tile polynomial (FAST differs from FAST_DIRECT on tile 1 and
    carries the polynomial's truncation, more than 1e-12 of the far term at the gate in the wing); 1e-3 outside, and with a window one
    bin short of the tile, it is evaluated per bin (bit-identical rows)."""
    wg, K = 64, 8
    ref = tc.reference(512, "far_gate")
    case = ref.case
    out = run_modes(pkg, ctxs, case, ref, wg, K)
    sl = slice(512, 1024)
    seen = 0
    for e, j, tile, isfar in case.far_expect:
        fast, direct = out["fast"][1][e][sl], out["fast_direct"][1][e][sl]
        assert np.array_equal(fast, direct) != isfar, case.labels[e]
        if isfar and case.labels[e].startswith("l0 asym+0 A1000"):
            err = np.max(np.abs(fast.astype(tr.LD) - ref.M[e][sl]) / ref.F[e][sl])
            print("%s: truncation %.3e of the far term (tau_far %.3e)" % (case.labels[e], float(err), TAU_FAR))
            assert 0.5 * TAU_FAR <= float(err) <= TAU_FAR * 1.01 + 4e-15
            seen += 1
    assert seen == 1


def test_background_gate_follows_the_exponent(pkg, ctxs):
    """Every (evaluation, tile) of the background case takes the series exactly where the restated gate admits it."""
    ref = tc.reference(512, "background")
    case = ref.case
    out = run_modes(pkg, ctxs, case, ref, 64, 8)
    for e, t, series in case.series_expect:
        if case.evals[e][1][1] == 0.0 and case.evals[e][2] == 1:
            continue   # no active term: the series is the white noise alone, equal to the per-bin sum
        sl = slice(t * 512, min((t + 1) * 512, case.nx))
        same = np.array_equal(out["fast"][1][e][sl], out["fast_direct"][1][e][sl])
        if sl.stop - sl.start >= 64:
            assert same != series, (case.labels[e], t, series)


def test_p2_and_temperatures(pkg, ctxs):
    """logL = -(long)p (..) / T with p = 2."""
    ref = tc.reference(256, "windows")
    out = run_modes(pkg, ctxs, ref.case, ref, 64, 4, p=2.0)
    for b in range(len(ref.case.evals)):
        check_logl("windows/256 p=2 %s" % ref.case.labels[b], {k: v[0][b] for k, v in out.items()}, ref.logL[2][b])

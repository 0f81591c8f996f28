"""The reference of the likelihood tile checks itself (CPU): the numpy.longdouble twin that the GPU tests run over every bin against the
50-digit definition, on every directed case; its logL against the oracle's long-double sum; and the directed cases against what they
claim to be (which rows the far rule takes, which tiles the background gate admits, how well-conditioned logL is)."""
from decimal import Decimal, localcontext

import numpy as np
import pytest

import tile_cases as tc
import tile_reference as tr

TWIN_TOL = 2.0 ** -60
GEOMS = (256, 512, 1024)
ALL = [(tb, c.name) for tb in GEOMS for c in tc.cases(tb)]


def _checked_bins(c):
    """Every bin of the case's edge tiles, every 16th elsewhere."""
    keep = np.zeros(c.nx, dtype=bool)
    keep[::16] = True
    for t in c.edge_tiles:
        keep[t * c.tile_bins:min((t + 1) * c.tile_bins, c.nx)] = True
    return np.flatnonzero(keep)


@pytest.mark.parametrize("tb,name", ALL)
def test_twin_matches_the_definition(tb, name):
    ref = tc.reference(tb, name)
    c = ref.case
    bins = _checked_bins(c)
    worst = 0.0
    for b, ev in enumerate(c.evals):
        # (an evaluation's rows reach only the bins of their windows: elsewhere the row is the background alone, checked once per noise vector)
        exact = tr.model_row_exact(ev[0], ev[1], ev[2], ev[3], c.x, bins)
        with localcontext() as ctx:
            ctx.prec = tr.PREC
            for i in bins:
                # the twin's value, exactly: a longdouble is the sum of its double head and double tail
                head = float(ref.M[b][i])
                tail = float(ref.M[b][i] - tr.LD(head))
                m = Decimal(head) + Decimal(tail)
                err = abs(m - exact[int(i)]) / exact[int(i)]
                worst = max(worst, float(err))
    print("%s/%d: twin within %.2f x 2^-60 of the definition" % (name, tb, worst / TWIN_TOL))
    assert worst <= TWIN_TOL


@pytest.mark.parametrize("tb,name", ALL)
def test_cases_are_what_they_claim(tb, name):
    ref = tc.reference(tb, name)
    c = ref.case
    for e, j, tile, isfar in c.far_expect:
        t0, t1 = tile * c.tile_bins, min((tile + 1) * c.tile_bins, c.nx)
        xc, h = c.geometry(tile)
        assert tr.row_is_far(c.evals[e][0][j], t0, t1, xc, h) == isfar, (c.labels[e], j)
    # logL is a well-conditioned sum on every evaluation: its relative tolerance means what it says
    for b in range(len(c.evals)):
        m = ref.M[b]
        mass = float((ref.y / m).sum() + np.abs(np.log(m)).sum())
        assert mass <= 20.0 * abs(float(ref.logL[1][b] * tr.LD(ref.T[b]))), c.labels[b]
        assert np.all(m > 0)


def test_directed_terms_dominate_their_tile():
    """Far gate, early stop and wing: the far rows are >= 0.9 of M on tile 1; background: the Harvey terms are >= 0.9 of M at the gate."""
    for tb in GEOMS:
        for name in ("far_gate", "early_stop", "wing"):
            ref = tc.reference(tb, name)
            c = ref.case
            sl = slice(tb, 2 * tb)
            for e, j, tile, isfar in c.far_expect:
                if isfar and len(c.evals[e][0]) == 1:
                    assert float(np.min((ref.F[e][sl] + ref.Fa[e][sl]) / ref.M[e][sl])) >= 0.9, (name, c.labels[e])
    ref = tc.reference(512, "background")
    c = ref.case
    for b, ev in enumerate(c.evals):
        if ev[2] == 1 and ev[1][1] != 0.0:
            flips = [t for (e, t, s), (e2, t2, s2) in zip(c.series_expect, c.series_expect[1:]) if e == b == e2 and s != s2]
            assert len(flips) == 1, c.labels[b]   # per-bin tiles, then series tiles: one gate crossing per evaluation
            sl = slice(flips[0] * 512, (flips[0] + 2) * 512)
            assert float(np.min((ref.M[b][sl] - tr.LD(1e-2)) / ref.M[b][sl])) >= 0.9, c.labels[b]
    # consecutive tiles straddle eps = 0.02 and every exponent's own gate
    gates = sorted({t for e, t, s in c.series_expect if s and (e, t - 1, False) in set(c.series_expect)})
    assert gates[0] == 25 and len(gates) >= 5, gates


@pytest.mark.parametrize("p", (1, 2))
def test_twin_loglike_matches_the_oracle_sum(oracle, p):
    """chi22p restated: against the oracle's long-double sum of the same (double-rounded) model row, and against the 50-digit sum."""
    for name in ("windows", "narrow"):
        ref = tc.reference(256, name)
        for b in (0, len(ref.case.evals) - 2):
            md = np.asarray(ref.M[b], dtype=np.float64)
            mine = tr.loglike_ld(md, ref.y, 1.0, p)
            theirs = oracle.chi22p_ld(ref.y, md, p)
            assert abs(float(mine) - theirs) <= 4 * 2.0 ** -53 * abs(theirs)
            exact = tr.loglike_exact(md, ref.y, 1.0, p)
            head = float(mine)
            got = Decimal(head) + Decimal(float(mine - tr.LD(head)))
            assert abs(got - exact) <= Decimal(TWIN_TOL) * abs(exact) * 8   # 2^-57: a sum of nx rounded logarithms, each within 2^-63

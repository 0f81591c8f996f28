"""The table reference's own figures (no GPU, no library): its pieces against identities they must satisfy, its double twin against
the definition on every case -- r_twin per field, which sets the tolerance K = max(4, 4 r_twin) of the parity tests -- and the count of
rows whose window a rounding may decide, from the reference alone.

r_twin over every case of tests/table_cases.py (the figures are the reference's, not the product's):  nu 1.72, hv 5.86 (id 11: the arctangent and two changes of unit sit in front of the Wigner sum), gamma 0.56 -- printed by
test_twin_against_definition and pinned in table_check.R_TWIN.  Knife-edge rows: none in the directed cases, none in the random ones.
"""
import math
from decimal import Decimal
from fractions import Fraction

import pytest

import table_cases as tc
import table_check as chk
import table_reference as tr


def test_pslm_qlm_identities():
    for l in range(1, 4):
        for s in range(1, 2 * l + 1):
            assert tr.pslm(s, l, l) == l, (s, l)                       # the normalisation Pslm(l) = l (Schou et al. 1994)
            for m in range(-l, l + 1):
                assert tr.pslm(s, l, -m) == (-1) ** s * tr.pslm(s, l, m)
            if s % 2 == 0:
                assert sum(tr.pslm(s, l, m) for m in range(-l, l + 1)) == 0
        assert sum(tr.qlm(l, m) for m in range(-l, l + 1)) == 0           # (the distortion does not move a multiplet's mean)
    assert tr.pslm(2, 1, 0) == -2 and tr.pslm(3, 2, 1) == -4 and tr.qlm(1, 0) == Fraction(2, 3) * Fraction(2, 5)


@pytest.mark.parametrize("inc", tc.INCLINATIONS + [-37.0, 123.0])
def test_closed_form_visibilities(inc):
    """The closed forms sum to 1 per degree, vanish where they should, and agree with the twin's Wigner sum to its rounding."""
    from decimal import Context, localcontext
    with localcontext(Context(prec=tr.PREC)):
        for l in (1, 2, 3):
            v = tr.Exact.visibilities(l, Decimal(inc))
            assert abs(sum(v) - 1) < Decimal(10) ** -45
            assert all(v[k] == v[2 * l - k] and v[k] >= 0 for k in range(2 * l + 1))
            w, sc = tr.Twin.visibilities(l, inc), tr.visibility_scale(l, inc)
            for k in range(2 * l + 1):
                assert tr.ratio(w[k], v[k], sc[k]) <= 4 * chk.R_TWIN["hv"], (l, k, w[k], v[k])
    with localcontext(Context(prec=tr.PREC)):
        z2 = tr.Exact.visibilities(2, Decimal(tc.INCLINATIONS[5]))[2]
        z3 = tr.Exact.visibilities(3, Decimal(tc.INCLINATIONS[6]))[3]
        z31 = tr.Exact.visibilities(3, Decimal(tc.INCLINATIONS[7]))[2]
        assert max(z2, z3, z31) < Decimal(10) ** -30                     # (the double nearest the zero, squared)
        assert tr.Exact.visibilities(1, Decimal(90))[1] == 0 and tr.Exact.visibilities(1, Decimal(0))[1] == 1


def test_trigonometry_against_libm():
    for y, x in ((0.7, 0.6), (-0.7, 0.6), (0.7, -0.6), (1e-9, 3.0), (5.0, 1e-7), (0.8, 0.0), (-0.8, 0.0), (0.0, 0.9), (12.5, 0.3)):
        a = float(tr.Exact.atan_deg(y, x))
        assert a == pytest.approx(tr.Twin.atan_deg(y, x), rel=1e-14, abs=1e-300), (y, x)
    for d in (0.0, 1e-8, 30.0, 45.0, 89.99999999, 90.0, 137.0, -61.0, 360.5):
        s, c = tr.Exact.sincos_deg(Decimal(d))
        assert float(s) == pytest.approx(math.sin(math.radians(d)), abs=1e-15) and float(c) == pytest.approx(math.cos(math.radians(d)), abs=1e-15)


def test_interpolation_and_segments():
    xs, ys = [1.0, 2.0, 4.0, 8.0], [10.0, 20.0, 0.0, 4.0]
    assert [tr._segment(xs, v) for v in (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 7.9, 8.0, 9.0)] == [0, 0, 0, 0, 1, 1, 2, 2, 2]
    for xi, want in ((0.0, 0.0), (1.5, 15.0), (3.0, 10.0), (6.0, 2.0), (10.0, 6.0)):
        v, scale = tr._interpol(tr.Exact, xs, ys, xi)
        assert v == Decimal(want) and scale >= abs(want)


def test_twin_against_definition():
    """r_twin: the twin's distance from the definition per field over every case, in units of 2^-52 scale; its windows equal the
    definition's outside the knife-edge rows."""
    worst = {"nu": (0.0, None), "hv": (0.0, None), "gamma": (0.0, None)}
    rows = 0
    for g in tc.all_groups():
        for i in range(len(g.vectors)):
            ref, tw = g.reference(i), g.twin(i)
            assert ref["status"] == tw["status"], (g, g.names[i])
            exempt = chk.exempt_rows(g, i)
            for r, (a, b) in enumerate(zip(ref["rows"], tw["rows"])):
                rows += 1
                assert (a["l"], a["fc"], a["asym"]) == (b["l"], b["fc"], b["asym"])
                if r not in exempt:
                    assert (a["i0"], a["i1"]) == (b["i0"], b["i1"]), (g, g.names[i], r, a["edges"])
                cands = [("gamma", tr.ratio(b["gamma"], a["gamma"], a["gamma_scale"]))] if a["gamma_scale"] else []
                for k in range(2 * a["l"] + 1):
                    cands += [(f, tr.ratio(b[f][k], a[f][k], a[f + "_scale"][k])) for f in ("nu", "hv")]
                for f, v in cands:
                    if v > worst[f][0]:
                        worst[f] = (v, f"{g.name}[{g.names[i]}] row {r}")
    print("r_twin", {f: (round(v, 2), w) for f, (v, w) in worst.items()}, "rows", rows)
    assert rows > 10000
    for f, (v, w) in worst.items():
        assert v <= chk.R_TWIN[f], (f, v, w)
        assert v >= 0.25, (f, v)                                          # (a twin that IS the definition would measure nothing)


def test_knife_edge_rows_counted_from_the_reference():
    """Rows whose window a rounding may decide: none in the directed cases, at most one over all random ones (here: none)."""
    directed, random_ = [], []
    for g in tc.all_groups():
        for i in range(len(g.vectors)):
            hits = [(g.name, g.names[i], r) for r in chk.exempt_rows(g, i)]
            (directed if g.directed else random_).extend(hits)
    print("knife-edge rows: directed", directed, "random", random_)
    assert directed == []
    assert len(random_) <= 1


def test_cases_reach_what_they_claim():
    """The directed cases hit the paths they are named after (seen in the reference's own output)."""
    seen_status, clip_hi, clip_lo, one_bin, last_seg = set(), 0, 0, 0, 0
    for g in tc.all_groups():
        for i in range(len(g.vectors)):
            ref = g.reference(i)
            seen_status.add(ref["status"])
            for row in ref["rows"]:
                one_bin += row["i1"] - row["i0"] == 1
                clip_hi += row["fc"] < g.grid.x_first - 1.0 and row["i0"] == 0 and row["i1"] >= 1
                clip_lo += row["fc"] > g.grid.x_last + 1.0 and row["i1"] == g.grid.Nx
    assert seen_status == {tr.OK, tr.ERR_EMPTY_WINDOW, tr.ERR_NAN_WINDOW}
    assert clip_hi > 20 and clip_lo > 20 and one_bin >= 6 * 6
    g = [g for g in tc.groups(tr.AJ) if g.name.endswith("clip-on-x-last")][0]
    row = g.reference(0)["rows"][5]
    assert row["l"] == 1 and row["i0"] == g.grid.Nx - 9 and dict((n, d) for n, d, _ in row["edges"])["clip_lo"] == 0.0
    for mid in tc.IDS:
        for g in tc.groups(mid):
            if "-edge-" in "".join(g.names):
                i0 = {n: g.reference(i)["rows"] for i, n in enumerate(g.names) if n.startswith("edge-")}
                r = g.plength[2] // 2 * (1 if mid not in (tr.CLASSIC, tr.V2, tr.V3) else 1 + min(int(g.plength[1]), 3))
                assert i0["edge-i0-above"][r]["i0"] == i0["edge-i0-below"][r]["i0"] + 1, g
                assert i0["edge-i1-above"][r]["i1"] == i0["edge-i1-below"][r]["i1"] + 1, g

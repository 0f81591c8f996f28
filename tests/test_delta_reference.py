"""CPU checks of tests/delta_reference.py and tests/delta_cases.py: the longdouble twin against the 50-digit definition, the restated series
and moment form against the truncation terms of the budget, and the classification restatement on the directed cases -- every case
reaches the paths it is named for, with the margins its expectations hang on.  No device code runs here: tables come from the host
builder (tamcmc_build_mode_table)."""
import numpy as np
import pytest

import delta_cases as dc
import delta_reference as dr

CONFIGS = [dr.config("fast", 64, 8), dr.config("fast", 64, 4), dr.config("fast", 256, 4), dr.config("fast_direct", 256, 4),
           dr.config("fast_direct", 64, 8)]
GATED = ("light", "gate_fails", "pairs_not_light", "heights_only", "noise")   # variables whose path expectation hangs on the moment gate
_HOST = {}


def _host(pkg, synth, name):
    """(case, tables, references) from host-built tables, once per process."""
    if name not in _HOST:
        c = dc.case(pkg, synth, name)
        tabs = dc.host_tables(pkg, c)
        _HOST[name] = (c, tabs, dc.references((name, "host"), c, tabs))
    return _HOST[name]


def _slots(c, tabs, refs):
    E = c.idx.size + 1
    for ch in range(c.P.shape[0]):
        for k in range(E - 1):
            yield ch, k, tabs[ch * E], tabs[ch * E + 1 + k], refs[ch][k]


def _summary(pkg, synth, name):
    """Per (config name): budgets and tile paths of every slot."""
    c, tabs, refs = _host(pkg, synth, name)
    out = {}
    for cfg in CONFIGS:
        rows = []
        for ch, k, t0, t1, r in _slots(c, tabs, refs):
            tp = dr.tile_paths(r, t0, t1, c.star.x, cfg)
            rows.append((ch, k, r, tp, dr.slot_budget(r, t0, t1, c.star.x, cfg, tp)))
        out[cfg.name] = rows
    return c, out


@pytest.mark.parametrize("name", ["closed_form", "series", "noise", "moments", "full_table", "window_edge", "heights_only"])
def test_twin_matches_the_definition(pkg, synth, name):
    """|twin - definition| per bin, scaled to the slot's range, is at most 1/10 of the smallest budget the slot's reference serves.
    closed_form (the smallest case): every slot, every 16th bin of its range and the bins of largest |u|; the others: chain 0, 24 bins."""
    c, tabs, refs = _host(pkg, synth, name)
    worst = 0.0
    for ch, k, t0, t1, r in _slots(c, tabs, refs):
        if name != "closed_form" and ch > 0:
            continue
        s = r.slot
        if s.hi <= s.lo:
            continue
        n = (s.hi - s.lo + 15) // 16 if name == "closed_form" else 24
        bins = np.unique(np.concatenate([np.linspace(s.lo, s.hi - 1, n).astype(int), s.lo + np.argsort(np.abs(r.u[s.lo:s.hi]))[-4:]]))
        ex = dr.delta_exact(t0, t1, c.star.x, c.y, bins)
        err = max(abs(float(ex[int(i)] - dr.Decimal(_ld_str(r.f[int(i)])))) for i in bins)
        budget = min(dr.slot_budget(r, t0, t1, c.star.x, cfg).total for cfg in CONFIGS)
        ratio = err * (s.hi - s.lo) / (0.1 * budget)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ch, k, err, budget)
    print("%s: worst |twin - definition| x bins / (budget / 10) = %.3g" % (name, worst))


def _ld_str(v):
    """A longdouble as a decimal string that Decimal reads exactly enough (25 significant digits: 2^-64 is 5e-20)."""
    return np.format_float_scientific(v, precision=24, unique=False)


def test_series_and_moment_form_stay_inside_their_truncation_terms():
    """The five-term series up to |u| = 0.01 and the moment form up to |u| = 1e-5, in Python doubles, against the definition: the error is
    inside the budget's truncation term plus the doubles' own rounding (8 x 2^-53 (|yr| + 1) |u|).  This pins the budget, not the kernel."""
    yrs = [0.0, 1e-3, 0.3, 0.5, 1.0, 2.5, 9.0, 40.0]
    worst_s = worst_m = 0.0
    for sign in (1.0, -1.0):
        for au in [1e-8, 1e-6, 1e-5, 1e-4, 1e-3, 3e-3, 7e-3, 0.01]:
            for yr in yrs:
                u = sign * au
                ex = float(dr.bin_exact(u, yr))
                rnd = 8 * dr.EPS * (abs(yr) + 1.0) * au
                bs = (abs(yr) + 1.0 / 6.0) * au ** 6 / (1.0 - au)
                es = abs(dr.series5(u, yr) - ex)
                assert es <= bs + rnd, (u, yr, es, bs)
                worst_s = max(worst_s, es / (bs + rnd))
                if au <= dr.MOMENT_GATE:
                    bm = (abs(yr) + 1.0 / 3.0) * au ** 3 / (1.0 - au)
                    em = abs(dr.moment2(u, yr) - ex)
                    assert em <= bm + rnd, (u, yr, em, bm)
                    worst_m = max(worst_m, em / (bm + rnd))
    print("series: worst error / bound %.3g; moment form: %.3g" % (worst_s, worst_m))
    # a wrong third coefficient is outside the term: the bound has teeth at the steps the cases take
    bad = lambda u, yr: dr.series5(u, yr) + (0.3 - 1.0 / 3.0) * u ** 3
    assert abs(bad(3e-3, 1.0) - float(dr.bin_exact(3e-3, 1.0))) > 100 * ((1.0 + 1.0 / 6.0) * 3e-3 ** 6 + 16 * dr.EPS * 3e-3)


def test_a_table_against_itself(pkg, synth):
    c, tabs, _ = _host(pkg, synth, "closed_form")
    r = dr.slot_reference(tabs[0], tabs[0], c.star.x, c.y)
    assert float(r.dS) == 0.0 and (r.slot.lo, r.slot.hi) == (0, 0) and not r.slot.drows and not r.slot.light
    assert not r.slot.full and not r.slot.noise_changed and set(r.slot.kinds) == {0}
    assert dr.tile_paths(r, tabs[0], tabs[0], c.star.x, CONFIGS[0]) == []
    b = dr.slot_budget(r, tabs[0], tabs[0], c.star.x, CONFIGS[0])
    assert b.total == 0.0 and b.walked == 0


@pytest.mark.parametrize("name", list(dc.MAKERS))
def test_margins(pkg, synth, name):
    """Every gate a case's path expectations depend on is cleared by its margin: a factor 2 for the moment gate (variables named for a
    gated path), 1e-3 relative for the geometric far rule (every overlapping row of every slot) and for max |u| against 0.01 (closed_form; a bin
    that close to the threshold is granted the series' truncation by the budget, whichever form it takes)."""
    c, summ = _summary(pkg, synth, name)
    for cfg, rows in summ.items():
        for ch, k, r, tp, b in rows:
            if cfg.startswith("fast("):
                assert min([t.far_margin for t in tp] or [1.0]) >= 1e-3, (name, cfg, ch, k)
            if c.why[k] in GATED:
                assert all(t.decided for t in tp), (name, cfg, ch, k, [t.gate for t in tp if not t.decided])
            if c.why[k] == "closed":
                assert float(np.max(np.abs(r.u))) > dr.U_SERIES * (1 + dr.U_MARGIN)
            if c.why[k] == "just_inside":
                assert float(np.max(np.abs(r.u))) < dr.U_SERIES * (1 - dr.U_MARGIN)


def test_paths_series(pkg, synth):
    c, summ = _summary(pkg, synth, "series")
    rows = summ["fast(64,8)"]
    names = [c.star.names[i] for i in c.idx]
    for ch, k, r, tp, b in rows:
        s = r.slot
        if names[k] == "Height_l0":
            assert s.counts["heights_only"] >= 2 and s.counts["pair"] == 0 and s.light and not s.full
        if names[k] == "Width_l0":
            assert s.counts["pair"] >= 2 and s.counts["heights_only"] == 0
        if names[k] == "Frequency_l" and s.counts["pair"] == 1:
            assert s.light and b.n_done_tiles > 0 and float(r.M0.min()) > 0
        if c.why[k] == "series_high_order":
            assert float(np.max(np.abs(r.u))) >= 9e-4, (ch, k)   # terms 3 to 5 matter at the 1e-6 .. 1e-10 level
        else:
            assert float(np.max(np.abs(r.u))) <= 1e-2 and b.n_closed_bins == 0
    assert all(float(row["asym"]) != 0.0 for row in _host(pkg, synth, "series")[1][0].rows)
    assert sum(1 for _, k, r, _, _ in rows if r.slot.light) >= 6 and sum(1 for _, k, r, _, _ in rows if r.slot.full) >= 2
    assert len({int(row["l"]) for _, k, r, _, _ in rows for row, _ in r.slot.pieces}) == 4   # every degree


def test_paths_closed_form(pkg, synth):
    c, summ = _summary(pkg, synth, "closed_form")
    for cfg, rows in summ.items():
        for ch, k, r, tp, b in rows:
            mx = float(np.max(np.abs(r.u)))
            if c.why[k] == "closed":
                assert b.n_closed_bins > 0 and mx > 0.01
            else:
                assert b.n_closed_bins == 0 and 0.005 < mx < 0.01, mx


def test_paths_heights_only(pkg, synth):
    c, summ = _summary(pkg, synth, "heights_only")
    for ch, k, r, tp, b in summ["fast(64,4)"]:
        s = r.slot
        assert s.counts["heights_only"] >= 2 and s.counts["pair"] == 0 and s.counts["one_sided"] == 0 and s.light
        assert len(s.drows) == s.counts["heights_only"] and all(tag == "dh" for _, tag in s.drows)
        assert b.n_done_tiles > 0


def test_paths_window_edge(pkg, synth):
    c, tabs, refs = _host(pkg, synth, "window_edge")
    for ch, k, t0, t1, r in _slots(c, tabs, refs):
        moved = [j for j, kind in enumerate(r.slot.kinds) if kind == 2 and (t0.rows[j]["i0"] != t1.rows[j]["i0"] or t0.rows[j]["i1"] != t1.rows[j]["i1"])]
        assert moved, (ch, k)
        # the bins only one of the two windows holds belong to the affected range, and dM is one-sided there
        j = moved[0]
        assert r.slot.lo <= min(t0.rows[j]["i0"], t1.rows[j]["i0"]) and r.slot.hi >= max(t0.rows[j]["i1"], t1.rows[j]["i1"])


def test_paths_noise(pkg, synth):
    c, summ = _summary(pkg, synth, "noise")
    _, tabs, _ = _host(pkg, synth, "noise")
    E = c.idx.size + 1
    assert float(tabs[0].noise[1]) == 0.0 and float(tabs[0].noise[4]) != 0.0 and float(tabs[2 * E].noise[1]) != 0.0
    for cfg, rows in summ.items():
        for ch, k, r, tp, b in rows:
            s = r.slot
            assert s.noise_changed and not s.full and not s.light and not s.drows and (s.lo, s.hi) == (0, c.star.x.size)
            assert b.n_done_tiles == 0 and b.walked == c.star.x.size
            if k >= 4 and ch < 2:   # height / exponent of the switched-off term: the row changed, the model did not
                assert float(r.dS) == 0.0 and not np.any(r.dM)
            else:
                assert float(r.dS) != 0.0
            if cfg in ("fast(64,8)", "fast(64,4)"):
                assert b.n_moment_tiles == len(tp)   # the difference of two background series, through delta_moment_shortcut


def test_paths_full_table(pkg, synth):
    c, summ = _summary(pkg, synth, "full_table")
    for cfg, rows in summ.items():
        for ch, k, r, tp, b in rows:
            s = dr.slot_of(r, next(x for x in CONFIGS if x.name == cfg))
            if c.why[k] == "full":
                assert s.full == cfg.startswith("fast(") and not s.light and b.n_moment_tiles == 0
                assert len(s.drows) == (20 if s.full else 2 * s.counts["pair"]) and (s.full or len(s.drows) > 20)
            else:
                assert not s.full and not s.light and len(s.drows) == 20 > dr.FAR_ROWS and s.counts["pair"] == 10
                assert b.n_done_tiles == 0
                if cfg == "fast(64,4)":
                    assert b.n_moment_tiles >= 1   # delta_moment_shortcut inside the tile, not k_fd_far


def test_paths_moments(pkg, synth):
    c, summ = _summary(pkg, synth, "moments")
    clamped = 0
    for cfg in ("fast(64,8)", "fast(64,4)"):
        for ch, k, r, tp, b in summ[cfg]:
            s = r.slot
            assert s.light and len(s.drows) in (1, 2)
            far_only = [t for t in tp if t.gate is not None and t.far]
            assert far_only, (cfg, ch, k)
            if c.why[k] == "gate_fails":
                assert b.n_done_tiles == 0 and all(t.gate > dr.GATE_MARGIN for t in far_only) and b.walked == s.hi - s.lo
            else:
                assert b.n_done_tiles == len(far_only) + sum(1 for t in tp if t.gate is not None and not t.far) and b.n_done_tiles >= 3
                # far-only tiles on BOTH sides of the near tiles for the mode whose window lies inside the grid
                if s.lo > 0:
                    peak = int(np.argmax(np.abs(r.dM))) // (tp[0].t1 - tp[0].t0)
                    assert min(t.tile for t in tp if t.moment) < peak < max(t.tile for t in tp if t.moment)
            clamped += s.lo == 0
    assert clamped > 0
    for cfg in ("fast(256,4)", "fast_direct(256,4)", "fast_direct(64,8)"):
        assert all(b.n_moment_tiles == 0 and b.walked == r.slot_pairs.hi - r.slot_pairs.lo for _, _, r, _, b in summ[cfg])

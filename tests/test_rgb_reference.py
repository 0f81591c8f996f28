"""The red-giant reference's own figures (no GPU): its pieces against libm and against identities, its longdouble twin against the
definition on every case (r_twin per field, which sets K), the branches the directed cases are there for, the count of vectors a rounding
may decide (zero), the definition-level layer (the solver's roots against the zeros of p - g found by bisection between the poles), and
the oracle (oracle/armm_oracle.c) against the definition on every case.

Figures (printed by the tests): r_twin nu 2.8e-4, zeta 3.2e-5, hr 3.2e-5, heights 1.1e-4, widths 1.8e-5 (the twin carries 11 more bits than
a double): K = 4.  The oracle against the definition: every field within K on every case.  Knife-edge vectors: none.
The host unpack (csrc/rgb_unpack.h through tests/rgb_unpack_driver.cpp) is held to stage (a) field by field.

The clip z > 1 and the lift hr -> 1e-10 behind it are reached through the bias spline (clip-on-a-pole); an unbiased mode cannot clip
(test_zeta_of_an_unbiased_mode_stays_below_the_grid_maximum).
Exact zeros of p - g on a grid point cannot be constructed in double and stay untested."""
import math
from decimal import Context, Decimal, localcontext

import numpy as np
import pytest

import rgb_cases as rc
import rgb_check as chk
import rgb_reference as rr
import table_reference as tr

CASES = rc.all_cases()
GOOD = [c for c in CASES if c.expect.get("status", rr.OK) == rr.OK]


def _dec(v):
    return v if isinstance(v, Decimal) else Decimal(str(v))


def test_series_against_libm():
    with localcontext(Context(prec=rr.PREC)):
        for v in (0.0, 1e-9, 0.3, 0.785, 1.2, 1.5707, 2.0, 31.4, 123.456, -77.7, 412.0):
            s, c = rr.Ex.sincos(Decimal(v))
            assert float(s) == pytest.approx(math.sin(v), abs=2e-14) and float(c) == pytest.approx(math.cos(v), abs=2e-14)
            assert abs(s * s + c * c - 1) < Decimal(10) ** -45
        for v in (0.0, 1e-12, 0.04, 0.5, 1.0, 3.0, 1e6, -2.5, -1e-3):
            a = rr.Ex.atan(Decimal(v))
            assert float(a) == pytest.approx(math.atan(v), rel=1e-15, abs=1e-300)
            if v != 0:
                assert abs(rr.Ex.tan(a) - Decimal(v)) < (1 + Decimal(v) ** 2) * Decimal(10) ** -47      # (tan' = 1 + tan^2 on the 50th digit of a)


def test_any_g_mode_of_the_ladder_gives_the_same_function():
    """1e6 / (nu_g DPl) = n_g + alpha: p - g and the zeta term are the same function for every g mode (to 1e-40 at 50 digits), so the pair
    loop's roots are copies and the inner sum of zeta is L_g times one term -- the double loop as written agrees with the short form."""
    c = rc.by_name("base-b0-m1-app")
    sol = rc.reference(c)
    U = sol["U"]
    with localcontext(Context(prec=rr.PREC)):
        P = rr.Pair(rr.Ex, U, 2)
        for nu in (Decimal("151.2345"), Decimal("170.001"), Decimal(U["fl0"][3])):
            f0 = P.f(nu)
            for ig in (0, 7, U["Lg"] - 1):
                P.nu_g = rr.nu_g_of(rr.Ex, U, ig)
                assert abs(P.f(nu) - f0) < Decimal(10) ** -40, (nu, ig)
            lit, short = rr.zeta_sum(rr.Ex, U, nu, literal=True), rr.zeta_sum(rr.Ex, U, nu)
            assert abs(lit - short) < Decimal(10) ** -38 * abs(short), (nu, lit, short)


def test_base_variants_are_the_synthetic_generator_s(synth):
    for bt, mt, cte in rc.BASE_VARIANTS:
        p, pl = synth.make_params_rgb_model(np.random.default_rng(5), bias_type=bt, model_type=mt, cte_width=cte)
        c = rc.by_name(f"base-b{bt}-m{mt}-{'cte' if cte else 'app'}")
        assert np.array_equal(p, c.params) and np.array_equal(pl, c.plength)


def test_twin_against_definition():
    """r_twin per field over every case, both local grids of every root; the twin takes every decision the definition takes."""
    worst = {f: (0.0, None) for f in chk.K}

    def add(f, tw, ref, scale, where):
        if scale == 0.0:
            assert _dec(tw) == ref or abs(float(_dec(tw) - ref)) < 1e-18 * max(abs(float(ref)), 1e-300), (f, where)
            return
        r = abs(float(_dec(tw) - ref)) / (rr.EPS * scale)
        if r > worst[f][0]:
            worst[f] = (r, where)
    modes = 0
    for c in CASES:
        ref, tw = rc.reference(c), rc.twin(c)
        assert ref["status"] == tw["status"] == c.expect.get("status", rr.OK) or c.expect.get("over_cap"), c
        assert len(ref["cands"]) == len(tw["cands"]) and len(ref["roots"]) == len(tw["roots"]), c
        for a, b in zip(ref["cands"], tw["cands"]):
            assert (a["ip"], a["cell"]) == (b["ip"], b["cell"])
            for k in (0, 1):
                x, y = a["alts"][k], b["alts"][k]
                assert (x["kind"], x["j"], x["accepted"], x["kept"]) == (y["kind"], y["j"], y["accepted"], y["kept"]), (c, a["cell"], k)
                if x["kept"]:
                    add("nu", y["prop"], x["prop"], x["scale"], f"{c} cell {a['cell']}/{k}")
        fr, ft = rc.finished(c), rr.finish_twin(tw)
        assert fr["status"] == ft["status"] == c.expect.get("status", rr.OK), (c, fr["status"])
        for i, (m, t) in enumerate(zip(fr["modes"], ft["modes"])):
            modes += 1
            assert (m["clipped"], m["lifted"], m["branch"]) == (t["clipped"], t["lifted"], t["branch"])
            for f, key in (("nu", "nu"), ("zeta", "zeta"), ("hr", "hr"), ("hv", "H"), ("gamma", "W"), ("nu", "a1")):
                add(f, t[key], m[key], m[key + "_scale"], f"{c} mode {i} {key}")
        for i, (a, b) in enumerate(zip(fr["rows"], ft["rows"])):
            assert (a["l"], a["i0"], a["i1"]) == (b["l"], b["i0"], b["i1"]), (c, i)
            for k in range(2 * a["l"] + 1):
                for f in ("nu", "hv"):
                    add(f, b[f][k], a[f][k], a[f + "_scale"][k], f"{c} row {i} {f}[{k}]")
    print("r_twin", {f: (float(f"{v:.3g}"), w) for f, (v, w) in worst.items()}, "modes", modes)
    assert modes > 1400
    for f, (v, w) in worst.items():
        assert v <= chk.R_TWIN[f], (f, v, w)
        assert chk.K[f] == 4.0


def test_cases_reach_what_they_claim():
    seen = {"fact": set(), "kind": set(), "branch": set(), "model": set()}
    for c in CASES:
        sol, fin, e = rc.reference(c), rc.finished(c), c.expect
        U = sol["U"]
        assert fin["status"] == e.get("status", rr.OK), (c, fin["status"])
        if "modes" in e:
            assert e["modes"][0] <= len(fin["modes"]) <= e["modes"][1], (c, len(fin["modes"]))
        if e.get("over_cap"):
            assert sol["status"] == rr.OK and len(sol["roots"]) > rr.CAP1 and sol["n_raw"] <= 1024, (c, len(sol["roots"]))
        if e.get("few_g"):
            assert U["few_g"] and U["Lg"] < 6 and float(U["zone"]) > 10 and len(fin["modes"]) > 3, c
        if e.get("numin_negative"):
            assert any(n.startswith("numin>=0") and float(U["nu_p"][int(n[9:-1])] - U["zone"] * U["Dnu"]) < 0 for n, _, _ in sol["edges"]), c
        if e.get("no_modes"):
            assert U["no_modes"] and fin["modes"] == [] and len(fin["rows"]) == U["L"].Nfl0 + U["L"].Nfl2 + U["L"].Nfl3, c
        if "fact" in e:
            assert U["fact"] == e["fact"] and len(fin["modes"]) > 10, (c, U["fact"])
        if "branches" in e:
            assert {m["branch"] for m in fin["modes"]} == e["branches"], c
        if "clip" in e:
            # the named modes clip (z > 1 before the clip) and are lifted (hr -> 1e-10), each with margin; every other mode does neither
            edges = {n: (d, sc) for n, d, sc in fin["edges"]}
            for i, m in enumerate(fin["modes"]):
                want = i in e["clip"]
                assert (m["clipped"], m["lifted"]) == (want, want), (c, i)
                for name in (f"z>1 mode {i}", f"|hr|<1e-5 mode {i}"):
                    d, sc = edges[name]
                    assert d > 1000 * chk.K_EDGE * rr.EPS * sc, (c, name, d, sc)
                if want:
                    assert m["zeta"] == 1 and float(m["hr"]) == 1e-10 and float(m["W"]) == 0.0 and float(m["H"]) < 1e-8, (c, i)
            assert len(fin["modes"]) - len(e["clip"]) >= 1
        if "hr_below" in e:
            assert min(float(m["hr"]) for m in fin["modes"]) < e["hr_below"] and not any(m["clipped"] or m["lifted"] for m in fin["modes"]), c
        if e.get("lost"):
            # the g-dominated roots sit on the poles and are lost: what is left is at most two modes per p mode
            assert 0 < len(fin["modes"]) <= 2 * U["Lp"] and U["Lg"] > 5 * len(fin["modes"]), c
        if "gate" in e:
            g = e["gate"]
            hit = [cd for cd in sol["cands"] if cd["ip"] == g["ip"] and cd["alts"][0]["kind"] == g["kind"] and abs(float(cd["alts"][0]["prop"]) - g["prop"]) < 0.01]
            assert len(hit) == 1, (c, len(hit))
            for a in hit[0]["alts"]:
                assert a["accepted"] == g["accepted"] and abs(float(a["ratio"]) - float(g["gate"])) >= 1e-6, (c, float(a["ratio"]))
                assert abs(float(a["ratio"]) - float(g["gate"])) < 1e-4, (c, float(a["ratio"]))
            # accepted, the candidate is a mode of its own (not a copy the unique drops): its partner vector has one mode less
            other = rc.by_name(c.name.replace("accepted", "rejected") if g["accepted"] else c.name.replace("rejected", "accepted"))
            assert len(sol["roots"]) - len(rc.reference(other)["roots"]) == (1 if g["accepted"] else -1), c
            if g["accepted"]:
                assert any(r is hit[0] for r in sol["roots"]), c
        if "above_pole" in e:
            g = e["above_pole"]
            hit = [cd for cd in sol["roots"] if cd["ip"] == g["ip"] and cd["cell"] == g["cell"]]
            assert len(hit) == 1 and hit[0]["alts"][0]["kind"] == "interp" and hit[0]["alts"][1]["kept"], c
            lo, hi = float(U["nu_p"][g["ip"]] - U["zone"] * U["Dnu"]), float(U["nu_p"][g["ip"]] + U["zone"] * U["Dnu"])
            h = (hi - lo) / (int((hi - lo) / U["resol"]) - 1)
            na, ks = U["ng_min"] + U["ig0"][g["ip"]] + U["alpha"], 1e6 / U["DPl"]
            poles = [ks / (k + na + 0.5) for k in range(int(ks / hi - na - 2), int(ks / lo - na + 2))]
            inside = [p for p in poles if math.floor((p - lo) / h) == g["cell"] - 2]
            assert len(inside) == 1 and min(inside[0] - (lo + (g["cell"] - 2) * h), lo + (g["cell"] - 1) * h - inside[0]) > 1e-4, (c, inside)
            assert inside[0] < float(hit[0]["alts"][0]["rmin"]), c          # (the pole lies below the refinement window: the root is not lost)
        if e.get("irregular"):
            d = [float(v) for v in U["dnup"]]
            assert max(d) - min(d) > 0.5, d
        if e.get("runs"):
            runs = rr.unique_runs(sol)
            tol = 2 * U["resol"]
            assert sum(len(r) >= 3 for r in runs) >= 3, [len(r) for r in runs]
            # an element within tol of its left neighbour that is KEPT: it lies beyond tol of the last kept one
            assert sum(1 for r in runs for k in range(1, len(r)) if r[k][1] and abs(r[k][0] - r[k - 1][0]) <= tol) >= 1
        if sol["status"] == rr.OK and not U["no_modes"]:
            seen["fact"].add(U["fact"])
            seen["kind"] |= {a["kind"] for cd in sol["cands"] for a in cd["alts"]}
            seen["branch"] |= {m["branch"] for m in fin["modes"]}
            seen["model"].add((c.model_id, U["model_type"], U["bias_type"]))
    assert seen["fact"] == {"0.04", "0.01", "0.005"} and seen["kind"] == {"interp", "below", "above"}
    assert seen["branch"] == {None, "left", "in", "right"} and len(seen["model"]) >= 8


def test_the_p_mode_refusal_is_the_limit_of_32_and_nothing_else(monkeypatch):
    """refuse-m1-33-p-modes: 32 radial orders (the most a vector may list) give 33 p modes in range; with the limit lifted the same vector
    is solved, so the refusal is Lp > 32 and no other rule.  (28 orders give 29 p modes: accepted.)"""
    c = rc.by_name("refuse-m1-33-p-modes")
    assert int(c.plength[2]) == rr.MAXL and rc.reference(c)["status"] == rr.ERR_BAD_ARG
    monkeypatch.setattr(rr, "MAXP", 64)
    sol = rr.build(c.model_id, c.params, c.plength, c.x, twin=True)
    assert sol["status"] == rr.OK and sol["U"]["Lp"] == 33 and len(sol["roots"]) > 50
    p28, pl28 = rc.make_params(np.random.default_rng(5), model_type=1, nmax=28, dnu=5.0, n_first=20)
    monkeypatch.setattr(rr, "MAXP", 32)
    s28 = rr.build(rr.ID_APP, p28, pl28, c.x, twin=True)
    assert s28["status"] == rr.OK and s28["U"]["Lp"] == 29


def test_zeta_of_an_unbiased_mode_stays_below_the_grid_maximum():
    """A statement about UNBIASED modes only (a bias moves a mode off its zero: tests/rgb_cases.py, clip-on-a-pole).  At a zero of p - g,
    q tan X = tan(down), hence cos^2 X = q^2 cd^2 / (q^2 cd^2 + sd^2) and the zeta term is 1 / (1 + N q / (q^2 cd^2 + sd^2)) <= 1 / (1 + N q) for
    q <= 1, N = 1e-6 nu^2 DPl / Dnu.  On a regular ladder (model_type 0) every p mode gives the same term, so the sum at such a mode is at
    most Lp Lg / (1 + N q), whatever the solver's step, while the maximum over the 4-year grid is within ~1e-5 of Lp Lg (a grid point next
    to a pole of tan X, where the term is 1).  Asserted on every such case: each mode's term obeys the bound, and the bound lies below
    the grid maximum by a margin."""
    seen = 0
    for c in GOOD:
        sol, fin = rc.reference(c), rc.finished(c)
        U = sol["U"]
        if U["no_modes"] or U["model_type"] != 0 or U["bias_type"] != 0 or not fin["modes"] or U["q"] > 1:
            continue
        LpLg = U["Lp"] * U["Lg"]
        top = float(fin["zeta_norm"]) / LpLg
        assert 1 - 1e-3 < top <= 1.0, (c, top)
        for m in fin["modes"]:
            N = 1e-6 * float(m["nu"]) ** 2 * U["DPl"] / float(U["Dnu"])
            bound = 1 / (1 + N * U["q"])
            term = float(m["zeta"]) * top
            assert term <= bound + 1e-4, (c, term, bound)           # (1e-4: an extrapolated root lies up to ~1e-4 muHz from its zero)
            assert bound < top - 1e-4, (c, bound, top)              # no unbiased mode of this vector can clip, at any resol
            seen += 1
    assert seen > 300


def test_no_vector_sits_on_a_knife_edge():
    """Decisions within K_EDGE 2^-52 scale of their decision point, from the reference alone, both choices of local grid: none.  (The
    point count of the local grid is excluded by construction: the reference carries both outcomes.)"""
    hits, decisions = [], 0
    for c in CASES + [s for name in rc.BATCHED for s in rc.perturbed(rc.by_name(name))[2]]:
        sol = rc.reference(c)
        decisions += len(sol["edges"])
        n = len(sol["roots"])
        for ch in ((0,) * n, tuple(1 if r["alts"][1]["kept"] else 0 for r in sol["roots"])):
            fin = rc.finished(c, ch)
            decisions += len(fin["edges"])
            hits += [(c.name,) + h for h in chk.exempt(c, fin)]
    print("decisions", decisions, "knife edges", hits)
    assert decisions > 50000
    assert hits == []


@pytest.mark.parametrize("case", GOOD, ids=str)
def test_solver_roots_are_the_zeros_of_p_minus_g(case):
    """Definition-level layer, independent of the grid method.  Between two poles of tan X, p - g is continuous and increasing: at most one
    zero, found by bisection and polished at 50 digits.  Every root the solver returns (before bias) lies within the interpolation bound of
    one true zero: |chord root - zero| <= (dx^2 / 8) max|f''| / min|f'| on the bracketing cell (f'' sampled at 17 points of the cell, doubled).
    Every true zero inside the keep range and farther than 2 resol + one step of the resol grid + one local step from every pole is
    returned: the refinement window is centred on the LEFT point of the sign-change cell, which lies up to one grid step below the zero,
    so a pole up to three grid steps below a zero still falls into the window.  A zero nearer to a pole may be missing (kept from the
    reference on purpose).  Nothing is returned that is not a zero."""
    sol = rc.reference(case)
    U = sol["U"]
    if U["no_modes"]:
        return
    resol = U["resol"]
    found = [(c["ip"], c["alts"][0]) for c in sol["sorted"]]
    with localcontext(Context(prec=rr.PREC)):
        keep_lo, keep_hi = float(U["keep_lo"]), float(U["keep_hi"])
        total = 0
        for ip in range(U["Lp"]):
            if U["ig0"][ip] < 0:
                continue
            zeros, poles = rr.true_roots(sol, ip)
            P = rr.Pair(rr.Ex, U, ip)
            mine = [a for i, a in found if i == ip]
            for a in mine:
                z = min(zeros, key=lambda v: abs(v - a["prop"]))
                xs = np.linspace(float(a["xa"]), float(a["xb"]), 17).astype(rr.LD)
                f = P.f_bulk(xs)
                h = xs[1] - xs[0]
                d1, d2 = np.diff(f) / h, np.diff(f, 2) / (h * h)
                if a["kind"] == "interp":
                    bound = float((a["xb"] - a["xa"]) ** 2) / 8 * 2 * float(np.max(np.abs(d2))) / float(np.min(d1)) + 8 * rr.EPS * a["scale"]
                    assert float(a["xa"]) - 1e-12 <= float(z) <= float(a["xb"]) + 1e-12
                else:
                    # a pole inside the local window and the zero beyond its last point: the line through the last two points is followed
                    # to zero (a Newton step from the window's end): error <= L^2 / 2 max|f''| / min|f'| over [x_a, zero]
                    span = np.linspace(float(a["xa"]), max(float(z), float(a["prop"])), 33).astype(rr.LD)
                    fs, hs = P.f_bulk(span), span[1] - span[0]
                    bound = float(span[-1] - span[0]) ** 2 / 2 * 2 * float(np.max(np.abs(np.diff(fs, 2) / (hs * hs)))) / float(np.min(np.diff(fs) / hs))
                assert abs(float(z - a["prop"])) <= bound, (case, ip, a["kind"], float(a["prop"]), float(z), bound)
            local = 4 * resol / (round(4 / float(U["fact"])) - 2)
            width = float(2 * U["zone"] * U["Dnu"]) if float(P.nu_p - U["zone"] * U["Dnu"]) >= 0 else float(P.nu_p + U["zone"] * U["Dnu"])
            h_grid = width / (int(width / resol) - 1)                      # the step of the resol grid: a little more than resol
            for z in zeros:
                zf = float(z)
                if not (keep_lo <= zf <= keep_hi):
                    continue
                lo_edge = float(P.nu_p - U["zone"] * U["Dnu"])
                if zf < max(lo_edge, 0.0) + resol or zf > float(P.nu_p + U["zone"] * U["Dnu"]) - resol:
                    continue
                far = min(abs(zf - p) for p in poles) > 2 * resol + h_grid + local if poles else True
                got = any(abs(float(a["prop"]) - zf) < resol for a in mine)
                assert got or not far, (case, ip, zf, min(abs(zf - p) for p in poles))
                total += got
        assert total >= len(sol["roots"])


@pytest.fixture(scope="module")
def unpack_driver(tmp_path_factory):
    """tests/rgb_unpack_driver.cpp: csrc/rgb_unpack.h compiled for the host outside the library's own build (hipcc, no GPU needed to run)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("rgb_unpack") / "driver")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unused-variable", "-o", exe,
                    os.path.join(root, "tests", "rgb_unpack_driver.cpp")], check=True)

    def run(case):
        text = f"{case.model_id} {float(case.x[2] - case.x[1])!r} {case.params.size} " + " ".join(repr(float(v)) for v in case.params) + " " + \
               " ".join(str(int(v)) for v in case.plength) + "\n"
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout
        rec = {}
        for line in out.splitlines():
            k, *v = line.split()
            rec.setdefault(k, []).append(v)
        return rec
    return run


@pytest.mark.parametrize("case", CASES, ids=str)
def test_host_unpack_against_stage_a(unpack_driver, case):
    """Prep and RowIn of unpack_vector<OneThread> (host, long double inside) field by field against stage (a) of the definition: status,
    counts, zone, factor and ig0 exactly; the ladders, widths, heights, spline coefficients and V[l][m] within K 2^-52 scale (V: the K of the
    Wigner sum, tests/table_check.py)."""
    import table_check
    rec = unpack_driver(case)
    U = rc.reference(case)["U"]
    assert int(rec["status"][0][0]) == U["status"], (case, rec["status"], U["status"])
    if U["status"] != rr.OK:
        assert rec["nn"][0] == ["1"] and rec["nh"][0] == ["0"] and float(rec["noise"][0][0]) == 1.0, case
        return
    assert [float(v) for v in rec["noise"][0]] == U["noise"] and int(rec["nh"][0][0]) == U["nharvey"]
    Lp = int(rec["Lp"][0][0])
    assert Lp == U["Lp"], (case, Lp, U["Lp"])
    worst = 0.0

    def near(got, want, scale, K, what):
        nonlocal worst
        if scale == 0.0:
            assert float(got) == float(want), (case, what, got, want)
            return
        r = tr.ratio(float(got), want, scale)
        worst = max(worst, r / K)
        assert r <= K, (case, what, r, got, float(want), scale)
    if not U["no_modes"]:
        assert int(rec["Lg"][0][0]) == U["Lg"] and int(rec["ng_min"][0][0]) == U["ng_min"], case
        prep = [float(v) for v in rec["prep"][0]]
        near(prep[0], U["Dnu"], U["s_Dnu"], chk.K["nu"], "Dnu")
        assert prep[1:4] == [U["DPl"], U["alpha"], U["q"]] and prep[4] == float(U["zone"]) and prep[5] == U["resol"] and prep[6] == float(U["fact"]), (case, prep)
        near(rec["keep"][0][0], U["keep_lo"], U["s_keep_lo"], chk.K["nu"], "keep_lo")
        near(rec["keep_hi"][0][0], U["keep_hi"], U["s_keep_hi"], chk.K["nu"], "keep_hi")
        for i in range(Lp):
            near(rec["nu_p"][0][i], U["nu_p"][i], U["s_nu_p"][i], chk.K["nu"], f"nu_p[{i}]")
            near(rec["dnu_loc"][0][i], U["dnu_loc"][i], U["s_dnu_loc"][i], chk.K["nu"], f"dnu_loc[{i}]")
            near(rec["dnup"][0][i], U["dnup"][i], U["s_dnup"][i], chk.K["nu"], f"dnup[{i}]")
        assert [int(v) for v in rec["ig0"][0]] == U["ig0"], (case, rec["ig0"], U["ig0"])
    L = U["L"]
    assert [int(v) for v in rec["rowin"][0]] == [L.Nfl0, L.Nfl2, L.Nfl3, L.lmax, int(U["do_amp"]), U["spline"]["n"] if U["spline"] else 0, int(U["cte"])]
    for n in range(L.Nfl0):
        near(rec["Wl0"][0][n], U["W0"][n], U["W0s"][n], chk.K["gamma"], f"Wl0[{n}]")
        near(rec["Hl0"][0][n], U["H0"][n], U["H0s"][n], chk.K["hv"], f"Hl0[{n}]")
    assert [float(v) for v in rec["Vl"][0]] == U["Vl"]
    for l in range(1, L.lmax + 1):
        for k in range(2 * l + 1):
            near(rec["V"][l][k], U["V"][l][k], U["Vs"][l][k], table_check.K["hv"], f"V[{l}][{k}]")
    scal = [float(v) for v in rec["scal"][0]]
    near(scal[0], U["eta0"], abs(float(U["eta0"])) * (2 * U["s_Dnu"] / float(U["Dnu"]) + 8), chk.K["nu"], "eta0")
    assert scal[1:] == [U["Hfactor"], U["Wfactor"], U["rot_env"], U["rot_core"], U["trunc_c"]]
    if U["spline"]:
        S = U["spline"]
        for name, key, power in (("sb", "b", 1), ("sc", "c", 2), ("sd", "d", 3)):
            for i in range(S["n"]):
                near(rec[name][0][i], S[key][i], 8 * S["ymax"] / S["hmin"] ** power, chk.K["nu"], f"{name}[{i}]")
        near(rec["sc0"][0][0], S["c0"], 8 * S["ymax"] / S["hmin"] ** 2, chk.K["nu"], "sc0")
    print("host unpack", case, "worst ratio / K", round(worst, 3))


@pytest.mark.parametrize("case", [c for c in CASES if c.name != "over-row-cap"], ids=str)
def test_oracle_against_the_definition(oracle, case):
    """oracle.rgb_modes (frequencies, zeta, widths, heights, splittings of the mixed modes; widths and heights of the radial modes) within
    K 2^-52 scale of the definition, and the status of call_model equal to the definition's, on every case.  near-row-cap: the oracle
    solves every (p, g) pair (8 x 330 grids of 7000 points, half a minute), so its modes are compared and the second solve inside call_model is
    not made.  over-row-cap is left out: 400 rows is a limit of the product, the oracle has none and there is nothing to compare."""
    sol, fin0 = rc.reference(case), rc.finished(case)
    cte = case.model_id == rr.ID_CTE
    step = float(case.x[2] - case.x[1])
    rc_, md = oracle.rgb_modes(case.params, case.plength, step, cte_width=cte)
    st = rc_ if case.name == "near-row-cap" else oracle.call_model(case.model_id, case.params, case.plength, case.x)[0]
    if case.product_limit or case.expect.get("over_cap"):
        assert st == 0 and rc_ == 0          # a stated limit of the product (32 p modes, 400 rows), not of the model: the oracle has none
        return
    assert (st == 0) == (fin0["status"] == rr.OK) and (rc_ == 0) == (sol["status"] == rr.OK), (case, st, rc_, fin0["status"])
    if fin0["status"] != rr.OK:
        return
    tally = chk.Tally()
    fin = chk.check_modes(case, md["fl1"], md["ksi"], None, tally, "oracle")
    U = sol["U"]
    for n in range(U["L"].Nfl0):
        for f, got, want, scale in (("gamma", md["Wl0"][n], U["W0"][n], U["W0s"][n]), ("hv", md["Hl0"][n], U["H0"][n], U["H0s"][n])):
            if scale == 0.0:
                assert float(got) == float(want), (case, f, n)
            else:
                assert tr.ratio(got, want, scale) <= chk.K[f], (case, f, n, got, want)
    for i, m in enumerate(fin["modes"]):
        for f, key, got in (("gamma", "W", md["Wl1"][i]), ("hv", "H", md["Hl1"][i]), ("nu", "a1", md["a1_l1"][i])):
            r = tr.ratio(got, m[key], m[key + "_scale"])
            tally.add(f, r, f"{case} mode {i} {key}")
            assert r <= chk.K[f], (case, i, key, r, got, float(m[key]), m[key + "_scale"])
    print("oracle", case, tally)

"""Red-giant tables and mixed modes against the 50-digit reference (tests/rgb_reference.py): the comparison shared by the CPU module
(oracle) and the GPU module (rgb_mixed_modes, rgb_batch_tables STRICT and FAST).

K per field is max(4, 4 r_twin).  r_twin is the distance of the reference's own longdouble twin from the definition over every case, in
units of 2^-52 scale (asserted by tests/test_rgb_reference.py: below 1e-3 for every field, the twin carrying 11 more bits than a double),
so K = 4 everywhere: the scales count every rounded intermediate of a straightforward double evaluation once, each contributes at most
half an ulp of its magnitude (one or two for tan, atan, cos, log, exp of the device's libm), and 4 leaves room for those.
K_EDGE follows table_check: 4 for the chain of roundings in front of a decision plus the K of the value that enters it.

A vector one of whose decisions lies within K_EDGE 2^-52 scale of its decision point is exempt as a whole (the decisions of the pre-step
feed each other: a grid point's sign decides a cell, the cell a root, the root every later mode's index).  The cases are chosen so that
none is.
"""
import numpy as np

import rgb_cases as rc
import rgb_reference as rr
import table_reference as tr

# measured 2.8e-4 / 3.2e-5 / 3.2e-5 / 1.1e-4 / 1.8e-5 (tests/test_rgb_reference.py prints them), pinned a little above; a twin that drifts shows
R_TWIN = {"nu": 4e-4, "zeta": 5e-5, "hr": 5e-5, "hv": 1.6e-4, "gamma": 3e-5}
K = {f: max(4.0, 4.0 * r) for f, r in R_TWIN.items()}
K_EDGE = 4.0 + K["nu"]


def exempt(case, fin=None):
    """The knife-edge decisions of a case, from the reference alone."""
    sol = rc.reference(case)
    fin = fin if fin is not None else rc.finished(case)
    hits = rr.knife_edges(sol["edges"] + fin["edges"], K_EDGE)
    for i, row in enumerate(fin["rows"]):
        hits += [(f"row {i} {n}", d, s) for n, d, s in rr.knife_edges(row["edges"], K_EDGE)]
    return hits


class Tally:
    def __init__(self):
        self.worst = {f: 0.0 for f in K}
        self.where = {}
        self.modes = self.rows = 0
        self.alt = [0, 0]

    def add(self, field, r, where):
        if r > self.worst[field]:
            self.worst[field], self.where[field] = r, where

    def __str__(self):
        return " ".join(f"{f}={self.worst[f]:.3f}@{self.where.get(f)}" for f in self.worst) + f" modes={self.modes} rows={self.rows} grids={self.alt}"


def choice_for(case, got_nu):
    """Per root: which of the two local grids (rgb_reference: ROUNDING-DECIDED BY CONSTRUCTION) the evaluation used -- the one whose mode
    frequency is nearer to what it delivered."""
    sol = rc.reference(case)
    n = len(sol["roots"])
    if n == 0:
        return ()
    ones = tuple(1 if c["alts"][1]["kept"] else 0 for c in sol["roots"])
    f0, f1 = rc.finished(case, (0,) * n), rc.finished(case, ones)
    ch = []
    for i in range(n):
        d0 = abs(float(got_nu[i]) - float(f0["modes"][i]["nu"]))
        d1 = abs(float(got_nu[i]) - float(f1["modes"][i]["nu"]))
        ch.append(ones[i] if d1 < d0 else 0)
    return tuple(ch)


def check_modes(case, got_nu, got_zeta, got_hr, tally, label=""):
    """(nu_m, zeta, h1_h0) of one vector against the definition; returns the finished reference at the evaluation's choice of local grids."""
    sol = rc.reference(case)
    tag = f"{label} {case.name}"
    assert len(got_nu) == len(sol["roots"]), (tag, len(got_nu), len(sol["roots"]))
    ch = choice_for(case, got_nu)
    fin = rc.finished(case, ch)
    for i, m in enumerate(fin["modes"]):
        at = f"{tag} mode {i}"
        for f, key, got in (("nu", "nu", got_nu[i]), ("zeta", "zeta", None if got_zeta is None else got_zeta[i]), ("hr", "hr", None if got_hr is None else got_hr[i])):
            if got is None:
                continue
            r = tr.ratio(got, m[key], m[key + "_scale"])
            tally.add(f, r, at)
            assert r <= K[f], (at, f, r, float(got), float(m[key]), m[key + "_scale"])
        tally.modes += 1
        tally.alt[ch[i]] += 1
    return fin


def check_rows(case, status, rows, noise, nharvey, nnoise, tally, label="", placeholder=False):
    """One vector's table (status, rows [MULT_DTYPE], |noise| row, nharvey, nnoise) against the definition."""
    sol = rc.reference(case)
    tag = f"{label} {case.name}"
    n1 = len(sol["roots"])
    fin0 = rc.finished(case)
    want_status = fin0["status"]
    assert int(status) == want_status, (tag, status, want_status)
    if want_status != rr.OK:
        assert len(rows) == 0, (tag, len(rows))
        if placeholder:
            assert nharvey == 0 and nnoise == 1 and noise[0] == 1.0, (tag, nharvey, nnoise, noise[:1])
        return None
    L = sol["U"]["L"]
    assert len(rows) == L.Nfl0 + n1 + L.Nfl2 + L.Nfl3, (tag, len(rows), n1)
    got_nu = [rows[L.Nfl0 + i]["fc"] for i in range(n1)]
    ch = choice_for(case, got_nu)
    fin = rc.finished(case, ch)
    assert nharvey == fin["nharvey"] and nnoise == fin["nnoise"], (tag, nharvey, nnoise)
    assert all(np.float64(noise[k]).view(np.int64) == np.float64(fin["noise"][k]).view(np.int64) for k in range(nnoise)), (tag, noise)
    for r, (got, want) in enumerate(zip(rows, fin["rows"])):
        at = f"{tag} row {r}"
        l = want["l"]
        assert int(got["l"]) == l and int(got["flags"]) == 0, (at, got["l"], got["flags"])
        assert np.float64(got["asym"]).view(np.int64) == np.float64(want["asym"]).view(np.int64), (at, got["asym"])
        for f, key, g in (("nu", "fc", got["fc"]), ("gamma", "gamma", got["gamma"])):
            if want[key + "_scale"] == 0.0:
                assert float(g) == float(want[key]), (at, key, g, want[key])
            else:
                rr_ = tr.ratio(g, want[key], want[key + "_scale"])
                tally.add(f, rr_, at)
                assert rr_ <= K[f], (at, key, rr_, float(g), float(want[key]), want[key + "_scale"])
        for k in range(7):
            if k > 2 * l:
                assert got["nu"][k] == 0 and got["hv"][k] == 0, (at, k)
                continue
            for f in ("nu", "hv"):
                if want[f + "_scale"][k] == 0.0:
                    assert float(got[f][k]) == float(want[f][k]), (at, f, k, got[f][k], want[f][k])
                    continue
                rr_ = tr.ratio(got[f][k], want[f][k], want[f + "_scale"][k])
                tally.add(f, rr_, f"{at} k={k}")
                assert rr_ <= K[f], (at, f, k, rr_, float(got[f][k]), float(want[f][k]), want[f + "_scale"][k])
        assert (int(got["i0"]), int(got["i1"])) == (want["i0"], want["i1"]), (at, got["i0"], got["i1"], want["i0"], want["i1"], want["edges"])
        tally.rows += 1
    return fin

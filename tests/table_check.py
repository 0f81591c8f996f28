"""One table against the 50-digit reference (tests/table_reference.py): the comparison shared by the CPU module (host builder) and the GPU
module (the three device builders).

K per field is max(4, 4 r_twin), r_twin being the distance of the reference's OWN double twin from the definition over every case
(R_TWIN below, asserted by tests/test_table_reference.py; measured 1.72 / 5.86 / 0.56 for nu / hv / gamma, pinned just above: K = 7.2 / 24 / 4).  A window is compared exactly;
a row is exempt from that only when one of its deciding quantities (an edge's quotient, a clip test's difference) lies within
K_EDGE 2^-52 scale of its decision point.  K_EDGE: the chain from the inputs to a quotient has six roundings of at most half an ulp of
quantities bounded by the scale (l f_s, + gamma, x c, f_c -+ h, - x_first or +- step, / step): 3, rounded up to 4, plus the K of an
interpolated width, whose own error enters through the half width.
"""
import numpy as np

import table_reference as tr

R_TWIN = {"nu": 1.8, "hv": 6.0, "gamma": 0.6}
K = {f: max(4.0, 4.0 * r) for f, r in R_TWIN.items()}
K_EDGE = 4.0 + K["gamma"]


def bits(v):
    return np.float64(v).view(np.int64)


def same_double(a, b):
    return bits(a) == bits(b)


class Tally:
    """Worst ratio per field, rows compared, rows exempt from the window comparison."""

    def __init__(self):
        self.worst = {"nu": 0.0, "hv": 0.0, "gamma": 0.0}
        self.where = {}
        self.rows = 0
        self.exempt = []

    def add(self, field, r, where):
        if r > self.worst[field]:
            self.worst[field], self.where[field] = r, where

    def __str__(self):
        return " ".join(f"{f}={self.worst[f]:.2f}@{self.where.get(f)}" for f in self.worst) + f" rows={self.rows} exempt={self.exempt}"


def exempt_rows(group, i):
    """Rows of vector i of the group whose window a rounding may decide: from the reference alone."""
    hits = {r for r, name in tr.knife_edges(group.reference(i), K_EDGE) if (i, r, name) not in group.exact_edges}
    return hits


def check_table(group, i, status, rows, noise, nharvey, nnoise, tally, fail_rule="host", label=""):
    """Vector i of the group: (status, rows [MULT_DTYPE], |noise| row, nharvey, nnoise) as a builder left them, against the reference.
    fail_rule: what a failed vector leaves -- "host": the status alone; "placeholder": no rows, nn = 1, noise[0] = 1 (dev_unpack.h, wg_unpack);
    "empty": no rows, nn = 0 (wg_unpack with empty_on_fail)."""
    ref = group.reference(i)
    tag = f"{label} {group.name}[{group.names[i]}]"
    assert status == ref["status"], (tag, status, ref["status"])
    if ref["status"] != tr.OK:
        if fail_rule != "host":
            assert len(rows) == 0 and nharvey == 0, (tag, len(rows), nharvey)
            assert nnoise == (1 if fail_rule == "placeholder" else 0), (tag, nnoise)
            if fail_rule == "placeholder":
                assert noise[0] == 1.0, tag
        return
    p = group.vectors[i]
    assert len(rows) == len(ref["rows"]) == group.per, (tag, len(rows), len(ref["rows"]))
    assert nharvey == ref["nharvey"] and nnoise == ref["nnoise"], (tag, nharvey, nnoise)
    assert len(noise) >= nnoise and all(same_double(noise[k], ref["noise"][k]) for k in range(nnoise)), (tag, noise, ref["noise"])
    exempt = exempt_rows(group, i)
    for r, (got, want) in enumerate(zip(rows, ref["rows"])):
        at = f"{tag} row {r}"
        l = want["l"]
        assert int(got["l"]) == l and int(got["flags"]) == want["flags"], (at, got["l"], got["flags"])
        assert same_double(got["fc"], want["fc"]) and same_double(got["asym"], want["asym"]), (at, got["fc"], got["asym"])
        if want["gamma_scale"] == 0.0:   # the magnitude of an input
            assert same_double(got["gamma"], float(want["gamma"])), (at, got["gamma"], want["gamma"])
        else:
            rg = tr.ratio(got["gamma"], want["gamma"], want["gamma_scale"])
            tally.add("gamma", rg, at)
            assert rg <= K["gamma"], (at, "gamma", rg, got["gamma"], want["gamma"])
        for k in range(7):
            if k > 2 * l:
                assert bits(got["nu"][k]) == 0 and bits(got["hv"][k]) == 0, (at, k, got["nu"][k], got["hv"][k])
                continue
            for f in ("nu", "hv"):
                rr = tr.ratio(got[f][k], want[f][k], want[f + "_scale"][k])
                tally.add(f, rr, f"{at} k={k}")
                assert rr <= K[f], (at, f, k, rr, float(got[f][k]), want[f][k], want[f + "_scale"][k])
        if r in exempt:
            tally.exempt.append(at)
        else:
            assert (int(got["i0"]), int(got["i1"])) == (want["i0"], want["i1"]), (at, got["i0"], got["i1"], want["i0"], want["i1"], want["edges"])
        tally.rows += 1
    assert not (group.directed and exempt), (tag, "a directed case sits on a knife edge", exempt)


def ulp_distance(a, b):
    """Distance of two finite doubles of one sign in units of the last place (0 for equal values, +0 and -0 included)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ia, ib = a.view(np.int64), b.view(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
    return np.abs(ia - ib)

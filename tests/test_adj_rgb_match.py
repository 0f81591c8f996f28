"""The row correspondence rule of the hybrid red-giant adjoint batch (tamcmc-c_amd/csrc/adj_rgb_match.h) on the CPU: a g++ driver
(tests/adj_rgb_match_driver.cpp) classifies hand-made pairs of tables; what each must give is stated here.

A perturbed slot is linearisable when both statuses are TAMCMC_OK, the row counts are equal, every row has the base row's l, and every l=1
row's fc lies within half the distance from the base row's fc to that row's nearest l=1 neighbour in the base table; every other slot with
two valid tables falls back; a failed table is neither."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAILED, LINEARISABLE, FALLBACK, FLAG = 0, 1, 2, 4
OK, ERR_BAD_ARG = 0, -5

L0 = [(0, 99.9), (0, 119.9)]
L1 = [(1, 100.0), (1, 110.0), (1, 130.0), (1, 135.0), (1, 150.0)]     # gaps 10, 20, 5, 15
L23 = [(2, 98.0), (2, 118.0), (3, 104.0)]
BASE = L0 + L1 + L23


def _moved(j, df):
    """BASE with l=1 row j moved by df."""
    l1 = list(L1)
    l1[j] = (1, L1[j][1] + df)
    return L0 + l1 + L23


def _without(j):
    l1 = list(L1)
    del l1[j]
    return L0 + l1 + L23


CASES = [
    ("identical", OK, OK, BASE, BASE, LINEARISABLE),
    # row 110: neighbours at 100 (the nearer, gap 10) and 130 (the farther, gap 20) -- half of the NEAREST gap on either side
    ("0.49 of the gap, nearer side", OK, OK, BASE, _moved(1, -4.9), LINEARISABLE),
    ("0.51 of the gap, nearer side", OK, OK, BASE, _moved(1, -5.1), FALLBACK),
    ("0.49 of the gap, farther side", OK, OK, BASE, _moved(1, +4.9), LINEARISABLE),
    ("0.51 of the gap, farther side", OK, OK, BASE, _moved(1, +5.1), FALLBACK),
    # the first and the last l=1 row have one l=1 neighbour: the l=0 row 0.1 below the first and the l=2 row after the last do not count
    ("first row, 0.49 of its only gap", OK, OK, BASE, _moved(0, -4.9), LINEARISABLE),
    ("first row, 0.51 of its only gap", OK, OK, BASE, _moved(0, +5.1), FALLBACK),
    ("last row, 0.49 of its only gap", OK, OK, BASE, _moved(4, +7.35), LINEARISABLE),
    ("last row, 0.51 of its only gap", OK, OK, BASE, _moved(4, +7.65), FALLBACK),
    # row 135: gaps 5 (below) and 15 (above)
    ("narrow gap below, 0.49", OK, OK, BASE, _moved(3, +2.45), LINEARISABLE),
    ("narrow gap below, 0.51", OK, OK, BASE, _moved(3, +2.55), FALLBACK),
    ("one row fewer, in the middle", OK, OK, BASE, _without(2), FALLBACK),
    ("one row fewer, at the low end", OK, OK, BASE, _without(0), FALLBACK),
    ("one row fewer, at the high end", OK, OK, BASE, _without(4), FALLBACK),
    ("one row more, in the middle", OK, OK, _without(2), BASE, FALLBACK),
    ("one row more, at the low end", OK, OK, _without(0), BASE, FALLBACK),
    ("one row more, at the high end", OK, OK, _without(4), BASE, FALLBACK),
    ("equal count, one lost at the low end and one gained at the high end", OK, OK, BASE, L0 + L1[1:] + [(1, 160.0)] + L23, FALLBACK),
    ("equal count, one gained at the low end and one lost at the high end", OK, OK, BASE, L0 + [(1, 95.0)] + L1[:-1] + L23, FALLBACK),
    ("l mismatch", OK, OK, BASE, L0 + L1 + [(2, 98.0), (3, 118.0), (3, 104.0)], FALLBACK),
    ("l mismatch at the edge of the l=1 block", OK, OK, BASE, L0 + L1[:-1] + [(2, 150.0)] + L23, FALLBACK),
    ("a NaN frequency", OK, OK, BASE, _moved(2, float("nan")), FALLBACK),
    ("failed base table", ERR_BAD_ARG, OK, BASE, BASE, FAILED),
    ("failed perturbed table", OK, ERR_BAD_ARG, BASE, BASE, FAILED),
    ("both failed", ERR_BAD_ARG, ERR_BAD_ARG, [], [], FAILED),
    ("a single l=1 row: no neighbour, nothing to be confused with", OK, OK, L0 + L1[:1] + L23, L0 + [(1, 160.0)] + L23, LINEARISABLE),
    ("no l=1 row", OK, OK, L0 + L23, L0 + L23, LINEARISABLE),
    ("no l=1 row, other rows moved", OK, OK, L0 + L23, [(0, 50.0), (0, 500.0)] + L23, LINEARISABLE),
    ("l=0, 2, 3 rows moved past each other: only the l=1 rows are held to their gaps", OK, OK, BASE, [(0, 150.0), (0, 50.0)] + L1 + L23, LINEARISABLE),
    ("two empty tables", OK, OK, [], [], LINEARISABLE),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("match") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adj_rgb_match_driver.cpp")], check=True)
    return exe


def test_row_correspondence_rule(driver):
    args = []
    for _, st0, st1, base, pert, _ in CASES:
        args += [st0, st1, len(base), len(pert)] + [v for row in base + pert for v in (row[0], repr(float(row[1])))]
    out = subprocess.run([driver] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[len(CASES)] == "classes %d %d %d flag %d" % (FAILED, LINEARISABLE, FALLBACK, FLAG)
    got = [int(v) for v in out[:len(CASES)]]
    for (name, *_, want), g in zip(CASES, got):
        assert g == want, (name, g, want)
    assert {c[-1] for c in CASES} == {FAILED, LINEARISABLE, FALLBACK}

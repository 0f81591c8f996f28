"""The launch plan of a two-group fused stretch (csrc/step_schedule.h: StepPlanner) without a GPU.  Around a swap pair that straddles
the two chain groups the boundary between the groups moves by one chain for the two iterations concerned (a "window") instead of both
groups stopping for a joint launch.  tests/step_hazard_driver.cpp (compiled with g++) replays the plan over every pair sequence of
length 4 (7, 8, 9 and 20 chains, both splits; length 6 for 7 and 8 chains) and over random sequences against a model of every buffer of
the fused step, with two launches ordered only through their stream or a planned wait; the plan itself is restated here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240611
SHAPES = [(C, xs) for C in (7, 8, 9, 20) for xs in (C // 2, C // 2 + 1)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hazards") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "step_hazard_driver.cpp")],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe, str(SEED)], check=True, capture_output=True, text=True, timeout=300).stdout
    rows = {"H": [], "W": []}
    for line in out.splitlines():
        w = line.split()
        rows[w[0]].append(w[1:])
    return rows


def _rows(printed, mode):
    return [(int(r[0]), int(r[1]), r[2], int(r[4]), int(r[5]), int(r[6]), int(r[7]), int(r[8]), r[9]) for r in printed["H"] if int(r[3]) == mode]


def test_the_plan_has_no_hazard_and_splits_no_pair(printed):
    rows = _rows(printed, 0)
    seen = set()
    for C, xs, what, seqs, hazards, unsplit, windows, joints, first in rows:
        assert hazards == 0 and unsplit == 0 and first == "-", (C, xs, what, first)
        assert windows > 0 and joints > 0, (C, xs, what)       # both kinds of iteration were exercised
        if what == "x4":
            assert seqs == C ** 4                               # pairs -1 .. C-2 at each of the four iterations
        if what == "x6":
            assert seqs == C ** 6
        seen.add((C, xs, what))
    assert seen == {(C, xs, w) for C, xs in SHAPES for w in ("x4", "r")} | {(C, xs, "x6") for C, xs in SHAPES if C <= 8}


def test_windows_replace_most_joint_launches(printed):
    """Over every sequence of four pairs: the iterations that joint_launch() names are the windows plus the joint launches of the plan,
    and a window iteration stays joint only for a pair on the moved boundary."""
    for C, xs, what, seqs, hazards, unsplit, windows, joints, first in _rows(printed, 0):
        if what != "x4":
            continue
        # iteration k of 4 is near a straddle: its own pair (1 in C of the values -1 .. C-2), or for k >= 1 the previous one's
        near = C ** 4 // C + 3 * (C ** 4 - (C - 1) ** 2 * C ** 2)
        assert windows + joints == near, (C, xs)
        assert joints * 4 < windows, (C, xs)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_the_model_sees_a_removed_wait(printed, mode):
    """1: s1 does not wait for st after a window; 2: st does not wait for s1 before one; 3, 4: the waits inside a window for the shared
    block of extra candidate slots (of s1 for st before a pair of the second group, of st for s1 before a repeated straddle)."""
    rows = _rows(printed, mode)
    assert {(C, xs) for C, xs, *_ in rows} == set(SHAPES)
    for C, xs, what, seqs, hazards, unsplit, windows, joints, first in rows:
        assert hazards > 0 and first != "-", (C, xs, what, mode)
        assert unsplit == 0


def _plan(C, xs, pairs):
    """Independent restatement of StepPlanner::next over one stretch (the closing launches: a last pair of -1)."""
    out = []
    s1_must_wait = s1_ahead = in_window = False
    for k, A in enumerate(pairs):
        Ap = pairs[k - 1] if k else -1
        near = A == xs - 1 or Ap == xs - 1
        if near and (xs in (A, Ap) or xs + 1 >= C):
            out.append((C, 0, int(s1_ahead), 0))
            s1_ahead, s1_must_wait, in_window = False, True, False
        elif near:
            st_w = s1_ahead and (not in_window or A == xs - 1)
            s1_w = s1_must_wait or (in_window and A > xs)
            out.append((xs + 1, 1, int(st_w), int(s1_w)))
            s1_ahead, s1_must_wait, in_window = True, False, True
        else:
            out.append((xs, 0, 0, int(s1_must_wait or in_window)))
            s1_ahead, s1_must_wait, in_window = True, False, False
    return out


def test_the_plan_is_the_rule_restated(printed):
    by = {}
    for C, xs, k, A, b, window, st_w, s1_w in printed["W"]:
        by.setdefault((int(C), int(xs)), []).append((int(k), int(A), int(b), int(window), int(st_w), int(s1_w)))
    assert set(by) == {(8, 4), (20, 10)}
    for (C, xs), rows in by.items():
        assert [r[0] for r in rows] == list(range(49)) and rows[-1][1] == -1
        pairs = [r[1] for r in rows]
        assert [r[2:] for r in rows] == _plan(C, xs, pairs), (C, xs)
        assert any(r[3] for r in rows) and any(r[2] == C for r in rows)       # a window and a joint launch among them
        for k, r in enumerate(rows):  # the boundary never splits this iteration's pair or the previous one's
            for A in (r[1], rows[k - 1][1] if k else -1):
                assert not (A >= 0 and A + 1 == r[2] and r[2] < C), (C, xs, k)

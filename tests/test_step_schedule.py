"""The host-side schedule of the device engine (csrc/step_schedule.h) without a GPU: the split of a run() call into fused and lockstep
stretches, the swap pair of an iteration, and the rule that makes an iteration of a two-group fused stretch one joint launch.  A small
C++ driver (tests/step_schedule_driver.cpp, compiled with g++) prints what the header computes; the expectations are restated here."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240611
MIN_FUSED = 3
CS, DNS = (1, 2, 3, 8, 20), (0, 1, 3, 7)


def _masks():
    m = ["0" * 40, "null:40", "1" * 40, "0" * 10 + "1" * 15 + "0" * 15,
         "1" + "0" + "11" + "00" + "11" + "000" + "1" + "0000" + "1",   # quiet runs of 1, 2, 3 (the MIN_FUSED edge) and 4 between learning
         "000" + "1" + "00" + "1" + "000",                              # the edge at both ends of a call
         "1" * 5 + "00", "1" * 5 + "000", "0" * 5 + "1" + "00",         # quiet tails of 2 and 3
         "0", "00", "000", "1", "01", "10", "null:1", "null:2", "null:3"]
    rng = np.random.default_rng(5)
    for n in (7, 19, 40):
        for p in (0.15, 0.5):
            m.append("".join("1" if x else "0" for x in rng.random(n) < p))
    return m


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sched") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "step_schedule_driver.cpp")],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe, str(SEED)] + _masks(), check=True, capture_output=True, text=True, timeout=60).stdout
    rows = {"S": [], "P": [], "J": [], "G": []}
    for line in out.splitlines():
        w = line.split()
        rows[w[0]].append(w[1:])
    return rows


def _learn(mask):
    return [0] * int(mask[5:]) if mask.startswith("null:") else [int(ch) for ch in mask]


def _expected_stretches(learn, use_fused):
    """Independent restatement: the maximal quiet runs of at least MIN_FUSED iterations are the fused stretches; what lies between two
    of them (or between one and an end of the call) is one lockstep stretch."""
    n, fused, i = len(learn), [], 0
    while i < n:
        j = i
        while j < n and learn[j] == learn[i]:
            j += 1
        if use_fused and not learn[i] and j - i >= MIN_FUSED:
            fused.append((i, j, 1))
        i = j
    out, at = [], 0
    for s in fused + [(n, n, 1)]:
        if s[0] > at:
            out.append((at, s[0], 0))
        if s[1] > s[0]:
            out.append(s)
        at = s[1]
    return out


def test_stretches_partition_a_call(printed):
    assert len(printed["S"]) == 2 * len(_masks())
    for use_fused, mask, *cells in printed["S"]:
        use_fused, learn = int(use_fused), _learn(mask)
        n = len(learn)
        got = [tuple(int(v) for v in cell.split(":")) for cell in cells]
        at = 0
        for s, e, f in got:  # the stretches tile [0, n) in order
            assert s == at and e > s, (mask, got)
            at = e
        assert at == n, (mask, got)
        # the start of every quiet run that is at least MIN_FUSED long (it reaches a learning iteration or the end of the call)
        long_quiet = [k for k in range(n) if not learn[k] and (k == 0 or learn[k - 1]) and not any(learn[k:k + MIN_FUSED]) and k + MIN_FUSED <= n]
        for s, e, f in got:
            if f:
                assert use_fused and e - s >= MIN_FUSED and not any(learn[s:e]), (mask, got)
                assert e == n or learn[e], (mask, got)  # ... and takes the whole quiet run
            elif use_fused:
                assert not [k for k in long_quiet if s < k < e], (mask, got)
                assert s not in long_quiet, (mask, got)
        assert got == _expected_stretches(learn, use_fused), (mask, use_fused)


def _pairs(printed):
    t = {}
    for C, dN, it, pair, draw in printed["P"]:
        t[(int(C), int(dN), int(it))] = (int(pair), int(draw))
    assert len(t) == len(CS) * len(DNS) * 201
    return t


def test_swap_pair_is_the_draw_on_swap_iterations_only(printed):
    t = _pairs(printed)
    seen = {C: set() for C in CS}
    for (C, dN, it), (pair, draw) in t.items():
        swaps = C >= 2 and dN > 0 and it % dN == 0 and it != 0
        if not swaps:
            assert pair == -1, (C, dN, it)
        else:
            assert 0 <= pair <= C - 2 and pair == draw, (C, dN, it, pair, draw)
            seen[C].add(pair)
        assert draw == t[(C, 1, it)][1]            # the draw does not depend on dN_mixing ...
        assert (draw == -1) == (C == 1) and draw <= C - 2   # ... and a single chain has no pair at any iteration
    assert seen[8] == set(range(7)) and seen[20] == set(range(19))  # 200 draws reach every pair
    assert printed["G"] == [["0", "0", "1", "1", "1", "2", "2"]]


def test_joint_launches_follow_the_straddling_pair(printed):
    t = _pairs(printed)
    n = n_joint_split = 0
    for C, xsplit, dN, split_ok, ia, i, joint in printed["J"]:
        C, xsplit, dN, split_ok, ia, i, joint = int(C), int(xsplit), int(dN), int(split_ok), int(ia), int(i), int(joint)
        straddles = lambda it: t[(C, dN, it)][0] == xsplit - 1
        want = (not split_ok) or straddles(i) or (i != ia and straddles(i - 1))
        assert joint == int(want), (C, xsplit, dN, split_ok, ia, i)
        n += 1
        n_joint_split += joint if split_ok else 0
    assert n == 2 * len(DNS) * 2 * (200 + 195) and n_joint_split > 0

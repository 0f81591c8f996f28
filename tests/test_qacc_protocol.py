"""The tiles' per-chain accumulators of the fused step (FusedArgs::qacc, csrc/dev_step_impl.h) without a GPU: who adds, who reads and who
zeroes each (chain, iteration mod 3) item, replayed over the launch plan of a two-group stretch (csrc/step_schedule.h: StepPlanner) by
tests/qacc_protocol_driver.cpp (compiled with g++).  Launches are ordered only through their stream or a planned wait, and nothing inside
a launch is ordered except one workgroup's own program.  Every sequence of four swap pairs and the closing launches, for 8, 5 and 20
chains; two stretches in a row, the second starting armed where the first ended, at every phase of the three sets."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240611
SHAPES = [(8, 4), (5, 2), (20, 10)]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qacc") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "qacc_protocol_driver.cpp")],
                   check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe, str(SEED)], check=True, capture_output=True, text=True, timeout=300).stdout
    got = []
    for line in out.splitlines():
        w = line.split()
        assert w[0] == "Q" and len(w) == 8, line
        got.append((int(w[1]), int(w[2]), w[3], int(w[4]), int(w[5]), int(w[6]), w[7]))
    return got


def test_every_zero_add_and_read_is_ordered(rows):
    """The zero happens before every add of the next launch that adds, every add before the read by the launch after it, every read
    before the next zero, and the closing launches leave every item zero."""
    seen = set()
    for C, xs, what, mode, seqs, violations, first in rows:
        if mode != 0:
            continue
        assert violations == 0 and first == "-", (C, xs, what, first)
        if what == "x4":
            assert seqs == C ** 4                      # pairs -1 .. C-2 at each of the four iterations
        else:
            assert seqs >= 1000
        seen.add((C, xs, what))
    assert seen == {(C, xs, w) for C, xs in SHAPES for w in ("x4", "two")}


@pytest.mark.parametrize("mode,kind", [(1, "add-on-read-item"), (2, "left-in-use")])
def test_the_model_sees_a_removed_zero(rows, mode, kind):
    """1: the commit workgroups do not zero set (it+1) mod 3 -- the fourth launch of a stretch adds onto what the second one read;
    2: the closing launches do not zero -- the accumulators of the last iterations stay as they are for the next stretch."""
    mine = [r for r in rows if r[3] == mode]
    assert {(C, xs) for C, xs, *_ in mine} == set(SHAPES)
    assert {(C, xs, what) for C, xs, what, *_ in mine} >= {(8, 4, "x4"), (5, 2, "x4")} | {(C, xs, "two") for C, xs in SHAPES}
    for C, xs, what, _, seqs, violations, first in mine:
        assert violations >= seqs and first.startswith(kind + ":"), (C, xs, what, first)

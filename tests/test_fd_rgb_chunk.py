"""The chunk rule of a red-giant finite-difference batch (tamcmc-c_amd/csrc/fd_rgb_chunk.h) on the CPU: a small C++ driver
(tests/fd_rgb_chunk_driver.cpp, compiled with g++) prints what the header computes; the expectations are restated here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, bytes per vector, budget) -> (chunk, number of chunks)
CASES = [
    ((0, 28672, 1 << 28), (1, 0)),            # empty batch: the loop never runs, its step is not zero
    ((1, 28672, 1 << 28), (1, 1)),
    ((2480, 28672, 1 << 28), (2480, 1)),      # the C5 batch fits at once
    ((65535, 28672, 1 << 28), (9362, 8)),     # the largest batch: 256 MiB / 28 KiB = 9362 vectors per pass, last pass 1
    ((10, 1000, 999), (1, 10)),               # one vector is larger than the budget: one at a time
    ((10, 1000, 5000), (5, 2)),               # an exact fit, twice
    ((10, 1000, 5999), (5, 2)),
    ((10, 1000, 10000), (10, 1)),             # the whole batch fits exactly
    ((10, 1000, 3000), (3, 4)),               # ragged last chunk
    ((7, 0, 100), (7, 1)),                    # no workspace per vector
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chunk") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "fd_rgb_chunk_driver.cpp")], check=True)
    return exe


def test_chunk_rule(driver):
    args = [str(v) for case, _ in CASES for v in case]
    out = subprocess.run([driver] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    for (case, want), line in zip(CASES, out):
        chunk, nchunks, covered, worst = (int(v) for v in line.split())
        assert (chunk, nchunks) == want, (case, line)
        assert covered == case[0] and worst <= chunk
        assert chunk >= 1 and (case[1] == 0 or chunk == 1 or chunk * case[1] <= case[2])
    assert out[len(CASES)] == "default_budget %d" % (256 << 20)

"""The form rule of the red-giant Fisher information (tamcmc-c_amd/csrc/fisher_rgb_rule.h, on top of adj_rgb_match.h) and the pass rule of
such a call (fd_rgb_chunk.h: fisher_rgb_chunk), on the CPU: a g++-built stand-alone driver (tests/rgb_fisher_rule_driver.cpp) on hand-made
triples of tables, built and run a second time under -fsanitize=address,undefined.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAILED, CENTRAL, ONE_SIDED, UNFROZEN = 0, 1, 2, 3
RH_CENTRAL, RH_PLUS, RH_MINUS = 0, 1, 2
NONE, PLUS, MINUS = 0, 1, 2

# l=0, three mixed modes 2 and 3 muHz apart, l=2
BASE = [(0, 100.0), (1, 110.0), (1, 112.0), (1, 115.0), (2, 130.0)]


def _moved(d, row=2):
    t = list(BASE)
    t[row] = (t[row][0], t[row][1] + d)
    return t


GAINED = BASE[:4] + [(1, 117.5)] + BASE[4:]          # one more mixed mode: every later row shifts
LOST = BASE[:3] + BASE[4:]
X0, XP, XM = 199.95986434979568, 199.95986434979568 + 2e-5, 199.95986434979568 - 3e-5     # (three different reciprocals)

# name -> ((status base, +, -), base, plus, minus, (form, reciprocal, substituted side, freeze +, freeze -))
CASES = {
    "both sides match": ((0, 0, 0), BASE, _moved(0.3), _moved(-0.3), (CENTRAL, RH_CENTRAL, NONE, 1, 1)),
    "row count changes on +": ((0, 0, 0), BASE, GAINED, _moved(-0.3), (ONE_SIDED, RH_MINUS, PLUS, 0, 1)),
    "row count changes on -": ((0, 0, 0), BASE, _moved(0.3), LOST, (ONE_SIDED, RH_PLUS, MINUS, 1, 0)),
    "same count, a mode past half its gap on both sides": ((0, 0, 0), BASE, _moved(1.2), _moved(-1.2), (UNFROZEN, RH_CENTRAL, NONE, 0, 0)),
    "same count, a mode past half its gap on + only": ((0, 0, 0), BASE, _moved(1.2), _moved(-0.3), (ONE_SIDED, RH_MINUS, PLUS, 0, 1)),
    "exactly half the gap is not a match": ((0, 0, 0), BASE, _moved(0.3), _moved(-1.0), (ONE_SIDED, RH_PLUS, MINUS, 1, 0)),
    "count changes on both sides": ((0, 0, 0), BASE, GAINED, LOST, (UNFROZEN, RH_CENTRAL, NONE, 0, 0)),
    "an l=0 row may move freely": ((0, 0, 0), BASE, _moved(40.0, 0), _moved(-40.0, 0), (CENTRAL, RH_CENTRAL, NONE, 1, 1)),
    "failed base": ((-5, 0, 0), [], _moved(0.3), _moved(-0.3), (FAILED, RH_CENTRAL, NONE, 0, 0)),
    "failed +": ((0, -3, 0), BASE, [], _moved(-0.3), (FAILED, RH_CENTRAL, NONE, 0, 0)),
    "failed -": ((0, 0, -5), BASE, GAINED, [], (FAILED, RH_CENTRAL, NONE, 0, 0)),
}


def _args():
    a = []
    for st, b, p, m, _ in CASES.values():
        a += list(st) + [len(b), len(p), len(m), repr(X0), repr(XP), repr(XM)]
        for t in (b, p, m):
            for l, fc in t:
                a += [l, repr(fc)]
    return [str(v) for v in a]


# (chains, Nvars, Nx, budget MiB, bytes per pre-step vector, pre-step budget) -> (chains per pass, passes)
W = 256 << 20
CHUNKS = [
    ((40, 91, 200000, 2048, 28672, W), (7, 6)),       # the red-giant star of the benchmark: 291.2 MB of rows per chain, 7 fit 2 GiB
    ((100, 91, 4000, 2048, 28672, W), (51, 2)),       # short rows: the pre-step's slice decides, 9362 vectors = 51 chains of 183
    ((1, 91, 200000, 10, 28672, W), (1, 1)),          # a lone chain above the row budget still runs
    ((3, 91, 4000, 2048, 28672, 100 * 28672), (1, 3)),  # ... and one whose 183 vectors exceed the slice (it takes it in chunks)
    ((3, 35, 4000, 1, 28672, W), (1, 3)),             # the small test star under 1 MiB: 2 240 000 B per chain
    ((1000, 91, 10, 2048, 1, 1 << 40), (358, 3)),     # never more vectors than a red-giant batch takes: 65535 // 183
    ((0, 91, 4000, 2048, 28672, W), (1, 0)),
]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rgb_fisher_rule") / ("driver_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "rgb_fisher_rule_driver.cpp")],
                   check=True)
    return exe


def test_form_reciprocal_and_substituted_side(driver):
    out = subprocess.run([driver] + _args(), check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[len(CASES)] == "forms 0 1 2 3 rh 0 1 2 sides 0 1 2"
    rh3 = [1.0 / (XP - XM), 1.0 / (XP - X0), 1.0 / (X0 - XM)]
    assert len(set(rh3)) == 3
    for (name, case), line in zip(CASES.items(), out):
        got = line.split()
        want = case[4]
        assert tuple(int(v) for v in got[:5]) == want, (name, line)
        assert float.fromhex(got[5]) == rh3[want[1]], (name, line)


def test_pass_rule_of_a_red_giant_call(driver):
    args = [str(v) for case, _ in CHUNKS for v in case]
    out = subprocess.run([driver, "chunk"] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    for (case, want), line in zip(CHUNKS, out):
        chunk, passes, covered, per_chain = (int(v) for v in line.split())
        C, Nv, Nx, mb, pv, wsb = case
        assert (chunk, passes) == want, (case, line)
        assert covered == C
        assert per_chain == 2 * Nv * Nx * 8
        assert chunk == 1 or (chunk * per_chain <= mb << 20 and chunk * (2 * Nv + 1) * pv <= wsb and chunk * (2 * Nv + 1) <= 65535)
    assert out[len(CHUNKS)] == "workspace %d" % W

"""The head of a gradient batch's device block (tamcmc-c_amd/csrc/fd_block.h) on the CPU: a small C++ driver (tests/fd_block_driver.cpp,
compiled with g++, and a second time with AddressSanitizer + UBSan as the stand-alone program it is) prints the plan of the head, the
block that stage() leaves and what results() sees; the rule is restated here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(1, 1, 0), (1, 7, 1), (3, 7, 5), (20, 111, 93), (2, 60, 186)]   # (C, Np, Nvars); the last is Fisher's doubled count
NAMES = ["params", "h", "pr", "ex", "pl", "idx", "sw", "lpp", "lpm", "st"]  # the documented order: seven inputs, three results
GUARD = 64


def al16(v):
    return (v + 15) & ~15


def sizes(C, Np, Nv):
    """Bytes of each array, in the documented order."""
    B = C * (Nv + 1)
    return [C * Np * 8, Nv * 8, 4 * Np * 8, 10 * 8, 11 * 4, Nv * 4, Np * 4, B * 8, B * 8, B * 4]


def plan(C, Np, Nv):
    """(offsets by name, in_bytes, out_bytes): every array at the next multiple of 16 behind its predecessor."""
    off, o, in_bytes = {}, 0, None
    for i, (name, n) in enumerate(zip(NAMES, sizes(C, Np, Nv))):
        if i == 7:
            in_bytes = o
        off[name] = o
        o = al16(o + n)
    return off, in_bytes, o - in_bytes


def pattern(j, n):
    """Byte k of input array j as the driver fills it."""
    return bytes(1 + (j * 37 + k * 11) % 250 for k in range(n))


def build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "fd_block_driver.cpp")],
                   check=True, capture_output=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fd_block")
    return [build(tmp, "driver", []), build(tmp, "driver_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def run(exe, case, present):
    r = subprocess.run([exe] + [str(v) for v in case] + [str(present)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (case, present, r.stdout[-500:], r.stderr[-4000:])
    return r.stdout.split("\n")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "C%d-Np%d-Nv%d" % c)
@pytest.mark.parametrize("sanitized", [0, 1], ids=["plain", "asan-ubsan"])
def test_head_plan_stage_and_results(drivers, case, sanitized):
    C, Np, Nv = case
    B = C * (Nv + 1)
    want_off, want_in, want_out = plan(C, Np, Nv)
    size = dict(zip(NAMES, sizes(C, Np, Nv)))
    for present in (1, 0):
        out = run(drivers[sanitized], case, present)
        v = [int(t) for t in out[0].split()]
        assert len(v) == 12
        off = dict(zip(NAMES[:7], v[:7]))
        off.update(zip(NAMES[7:], v[8:11]))
        in_bytes, out_bytes = v[7], v[11]
        # ---- the plan: multiples of 16, the documented order, disjoint regions large enough, the sums
        assert all(o % 16 == 0 for o in off.values()) and in_bytes % 16 == 0 and out_bytes % 16 == 0
        assert [off[n] for n in NAMES] == sorted(off[n] for n in NAMES) and off["params"] == 0
        ends = [off[n] for n in NAMES[1:]] + [in_bytes + out_bytes]
        for name, end in zip(NAMES, ends):
            assert off[name] + size[name] <= end, name          # (with the order: pairwise disjoint, each at least its array)
        assert off["sw"] + size["sw"] <= in_bytes == off["lpp"]  # inputs in front of in_bytes, results from there
        assert (off, in_bytes, out_bytes) == (want_off, want_in, want_out)
        # ---- stage(): given arrays byte-identical at their offsets, zeros elsewhere in [0, in_bytes), the guard untouched
        blk = bytes.fromhex(out[1])
        assert len(blk) == in_bytes + GUARD
        want = bytearray(in_bytes)
        if present:
            for j, name in enumerate(NAMES[:7]):
                want[off[name]:off[name] + size[name]] = pattern(j, size[name])
        assert blk[:in_bytes] == bytes(want)
        assert blk[in_bytes:] == b"\xa5" * GUARD
        # ---- results(): the three arrays of a block holding the counting pattern
        t = out[2].split(" ")
        count = bytes(i & 255 for i in range(in_bytes + out_bytes))
        assert int(t[0]) == B
        for name, got in zip(NAMES[7:], t[1:4]):
            assert bytes.fromhex(got) == count[off[name]:off[name] + size[name]], name
        assert [int(x) for x in out[3].split()] == [0, -5, -4]

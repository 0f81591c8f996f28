"""Known answers of tamcmc-c_amd/csrc/rng.h on the CPU: a small C++ driver (tests/rng_driver.cpp, compiled with g++) prints what the header
computes; Philox4x32-10, the draw addressing, the uniform and Box-Muller are restated in tests/sampler_reference.py (plain integers,
50-digit decimals).

  * the three Random123 known-answer vectors of philox4x32_10 (kat_vectors of the Random123 distribution: zeros, all ones, digits of pi);
  * the addressing (iteration lo, iteration hi, index, purpose << 16 | chain) / (seed lo, seed hi): the uniforms of a list of addresses
    -- iterations >= 2^32, chain 63, index 4096 (the first redraw of a proposal), all four purposes, seeds above 2^32 -- are the
    reference's bit for bit (a uniform holds the upper 53 bits of each word pair);
  * 0 < u < 1 strictly: the all-ones word pair gives the largest double below 1 (it used to round to 1.0), the zero pair 2^-54;
  * the clamp moves nothing else: over 1e6 pseudo-random words and the 2^12 largest 53-bit values exactly one output differs from the
    unclamped formula, the all-ones word's -- seeds chosen for their events elsewhere in the suite keep their walks;
  * the normals against the reference within K_z 2^-52 rho.  Measured here (x86-64, glibc): worst ratio 3.15 over the listed addresses
    and 4000 more -- the product rounds 2 pi u1 before taking the cosine, an error of up to 2 pi 2^-53 ~ 1.6 x 2^-52 in the angle, and
    rounds log, sqrt, cos / sin and the product once each.  K_z = 4 x 3.2, the convention of tests/test_gpu_priors.py."""
import os
import struct
import subprocess

import pytest

import sampler_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
U01 = [(0, 0), (0xffffffff, 0xffffffff), (0x7fffffff, 0xffffffff), (0xffffffff, 0xfffff7ff)]
# (seed, purpose, chain, iteration, index)
ADDRESSES = [(20240229, 1, 0, 0, 0), (20240229, 1, 0, 1, 0), (20240229, 2, 0, 0, 0), (20240229, 3, 0, 0, 0), (20240229, 4, 0, 0, 0),
             (77, 1, 63, 5, 46), (77, 2, 63, 2 ** 32, 0), (77, 1, 19, 2 ** 32 + 5, 4096), (77, 3, 0, 2 ** 40 + 3, 0), (77, 4, 7, 2 ** 32 - 1, 12345),
             (2 ** 32 + 1, 1, 1, 9, 4096 * 15 + 76), (2 ** 63 + 12345, 1, 2, 2 ** 33, 1), (0xfedcba9876543210, 2, 62, 10 ** 12, 0),
             (5, 1, 3, 1000, 4096), (5, 3, 0, 2 ** 32, 0), (5, 4, 63, 2 ** 32, 4096)]
ADDRESSES += [(31, 1 + k % 4, k % 64, 1000 + k, k % 77) for k in range(4000)]
K_Z = 4 * 3.2


def _dbl(hexbits):
    return struct.unpack("<d", struct.pack("<Q", int(hexbits, 16)))[0]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rng") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "rng_driver.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def printed(driver):
    args = []
    for ctr, key, _ in KAT:
        args += ["kat"] + [str(v) for v in ctr + key]
    for hi, lo in U01:
        args += ["u01", str(hi), str(lo)]
    for a in ADDRESSES:
        args += ["addr"] + [str(v) for v in a]
    args += ["clamp", "1000000"]
    out = subprocess.run([driver] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(KAT) + len(U01) + len(ADDRESSES) + 1
    return out


def test_known_answer_vectors(printed):
    for (ctr, key, want), line in zip(KAT, printed):
        assert line == "kat " + want
        assert " ".join("%08x" % w for w in R.philox4x32(ctr, key)) == want      # (the restatement itself)


def test_uniform_is_strictly_inside_the_unit_interval(printed):
    got = [_dbl(line.split()[1]) for line in printed[len(KAT):len(KAT) + len(U01)]]
    assert got[0] == 2.0 ** -54
    assert got[1] == 1.0 - 2.0 ** -53                     # the all-ones word: the largest double below 1, not 1.0
    assert got[2] == 0.5 - 2.0 ** -54                     # b = 2^52 - 1: the last b for which b + 1/2 is exact
    assert got[3] == 1.0 - 2.0 ** -52                     # b = 2^53 - 2: b + 1/2 is a tie as well, and rounds to the even b
    for (hi, lo), g in zip(U01, got):
        assert g == R.u01(hi, lo) and 0.0 < g < 1.0


def test_the_clamp_changes_one_word_in_2_to_the_53(printed):
    f = printed[-1].split()
    assert f[0] == "clamp" and int(f[2]) == 1000000 + 4096 + 1
    assert int(f[4]) == 1 and int(f[6], 16) == 0xffffffffffffffff and int(f[8]) == 0, printed[-1]


def test_addressing_uniforms_and_normals(printed):
    lines = printed[len(KAT) + len(U01):-1]
    worst = 0.0
    purposes = set()
    for a, line in zip(ADDRESSES, lines):
        u0, u1, z0, z1 = (_dbl(h) for h in line.split()[1:])
        ru0, ru1 = R.uniform2(*a)
        assert (u0, u1) == (ru0, ru1), a                   # the integer words (their upper 53 bits) and the addressing
        assert 0.0 < u0 < 1.0 and 0.0 < u1 < 1.0
        rz0, rz1, rho = R.normal2(*a)
        r = max(R.ratio([z0], [rz0], [float(rho)]), R.ratio([z1], [rz1], [float(rho)]))
        worst = max(worst, r)
        assert r <= K_Z, (a, r)
        purposes.add(a[1])
    print("\nBox-Muller: worst |z - ref| / (2^-52 rho) = %.2f over %d addresses (K_z = %.1f)" % (worst, len(ADDRESSES), K_Z))
    assert purposes == set(R.PURPOSE.values())
    # two addresses that differ in one field only draw different numbers (no field is dropped from the counter)
    base = (77, 1, 5, 2 ** 32 + 9, 3)
    seen = {R.words(*base)}
    for k, other in enumerate((78, 2, 6, 9, 4)):
        changed = list(base)
        changed[k] = other
        seen.add(R.words(*changed))
    seen.add(R.words(77 + 2 ** 32, 1, 5, 2 ** 32 + 9, 3))
    assert len(seen) == 7

"""The Gaussian-envelope row builder and the device engine's public surface for ids 0 / 1, without a GPU.

csrc/envelope_row.h holds ONE env_row for host and device.  Here its host build (a plain C++ driver, tests/envelope_row_driver.cpp,
g++ and libm) is held against the long-double restatement tests/envelope_row_reference.py field by field, on the synthetic stars'
vectors, perturbed copies and the edge cases (negative entries: the model takes absolute values; tc = 0: the Harvey term is switched
off and ln(1e-3 tc) = -inf).  Tolerance K 2^-52 |ref|, K = max(4, 4 r): libm's log and pow are within 1 ulp and the worst field, a_0^2 =
(p0 numax^p1)^2, stacks a pow, a product and a square -- r = 1.81 measured here, K = 7.2.  The same restatement holds the device's rows in
tests/test_gpu_envelope_device.py.

Also: the routing constants the sampler reads (tile, chunk, the one-launch step's limits), TAMCMC_OPT_ENVELOPE_DEVICE_ENGINE = 13 in the
header and the package, the audit entry in the header, the library and the Sampler class.  These fail on a tree without the feature."""
import os
import re
import subprocess

import numpy as np
import pytest

from envelope_row_reference import FIELDS, row_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MEASURED = 1.81
K = max(4.0, 4.0 * R_MEASURED)


def _vectors(synth):
    out = []
    rng = np.random.default_rng(17)
    for mid in (0, 1):
        p0 = synth.make_envelope_star(mid, nx=64, seed=3).params
        out.append((mid, p0.copy()))
        for _ in range(40):
            out.append((mid, p0 * (1.0 + 0.2 * rng.standard_normal(p0.size))))
        out.append((mid, -p0))
    p = synth.make_envelope_star(1, nx=64, seed=3).params
    for i in (1, 4):
        q = p.copy()
        q[i] = 0.0          # |tc| = 0
        out.append((1, q))
    q = p.copy()
    q[[2, 5]] = 0.0         # exponents 0
    out.append((1, q))
    return out


@pytest.fixture(scope="module")
def printed(synth, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("envrow") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "envelope_row_driver.cpp")],
                   check=True, capture_output=True, timeout=300)
    vec = _vectors(synth)
    text = "".join("%d %d %s\n" % (mid, p.size, " ".join(float(v).hex() for v in p)) for mid, p in vec)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    consts = [int(w) for w in out[0].split()[1:]]
    rows = [[float.fromhex(w) for w in line.split()[1:]] for line in out[1:]]
    assert out[0].startswith("C ") and len(rows) == len(vec)
    return consts, vec, np.array(rows)


def test_routing_constants(printed):
    consts, _, _ = printed
    tile, chunk, max_bins, max_bins_ksi, max_chunks, lim0, lim1 = consts
    assert (tile, chunk) == (1024, 4096)                      # envelope.hip's geometry, whatever the context's options say
    assert max_bins == 32768 and lim1 == max_bins             # id 1
    assert max_bins_ksi == 6144 and lim0 == max_bins_ksi      # id 0: the measured crossover
    assert max_chunks * chunk >= max_bins_ksi > (max_chunks - 1) * chunk   # k_env_step keeps id 0's chunk partials in LDS


def test_host_rows_match_the_restatement(printed):
    _, vec, rows = printed
    worst = 0.0
    for (mid, p), got in zip(vec, rows):
        want = row_reference(mid, p)
        for f, name in enumerate(FIELDS):
            w = want[f]
            if name.startswith("hon") or w == 0 or not np.isfinite(w):
                assert got[f] == float(w), (mid, name, got[f], w)
                continue
            ratio = float(abs(np.longdouble(got[f]) - w) / (np.longdouble(2.0) ** -52 * abs(w)))
            worst = max(worst, ratio)
            assert ratio <= K, (mid, name, got[f], float(w), ratio)
    print("\nworst host row field ratio r = %.2f (K = %.1f)" % (worst, K))


def test_public_surface(pkg):
    hip_h = open(os.path.join(ROOT, "include", "tamcmc_hip.h")).read()
    smp_h = open(os.path.join(ROOT, "include", "tamcmc_sampler.h")).read()
    assert re.search(r"#define\s+TAMCMC_OPT_ENVELOPE_DEVICE_ENGINE\s+13\b", hip_h)
    assert pkg.OPT_ENVELOPE_DEVICE_ENGINE == 13
    assert re.search(r"#define\s+TAMCMC_ENVELOPE_ROW_N\s+24\b", smp_h) and "tamcmc_sampler_get_envelope_rows(" in smp_h
    assert hasattr(pkg.lib(), "tamcmc_sampler_get_envelope_rows")
    assert len(pkg.Sampler.ENVELOPE_ROW_FIELDS) == 24 and tuple(pkg.Sampler.ENVELOPE_ROW_FIELDS) == FIELDS
    others = {int(m.group(1)) for m in re.finditer(r"#define\s+TAMCMC_OPT_(?!ENVELOPE_DEVICE_ENGINE)\w+\s+(\d+)\b", hip_h)}
    assert 13 not in others

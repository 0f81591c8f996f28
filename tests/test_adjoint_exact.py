"""The 50-digit definition of the table-space adjoint (tests/adjoint_reference.py) checked against itself, the numpy yardstick
(adjoint_numpy.table_adjoint, which shares its closed forms with csrc/adjoint.hip) checked against it, and the exact replay of the
contraction checked against adjoint_numpy.contract -- on the CPU, on tables of the host builder (no device code).

Measured: the yardstick's worst entry lies at 3.9e-15 (corner) / 6.6e-15 (corner_neg) of the entry's absolute sum, against the cap of
1e-13 that keeps it two orders under the device tolerance of 1e-11; halving the reference's step moves no entry by more than 1.3e-43
of its absolute sum."""
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np
import pytest

import adjoint_cases as ac
import adjoint_numpy as an
import adjoint_reference as ar

U = 2.0 ** -53


def _host_table(pkg, c, ch=0):
    s = c.star
    st, m, nz, nh = pkg.build_mode_table(s.model_id, c.P[ch], s.plength, s.x)
    assert st == 0
    return m, nz, nh


@pytest.mark.parametrize("name", ac.NAMES)
def test_cases_have_their_properties(pkg, synth, name):
    """Row counts (64, 68, 132: one, one-and-a-bit, two-and-a-bit lane passes of k_adj_contract), windows, asymmetry, |noise|: each case's
    own check; the large steps do move a window on the host builder's tables (the GPU test asserts it on the exported ones)."""
    c = ac.case(synth, name)
    base = c.check(pkg)
    assert np.all(c.h != 0) and (np.all(c.h < 0) if c.step_kind == "negative" else np.all(c.h > 0))
    if c.step_kind == "large":
        base, _, _ = _host_table(pkg, c)
        moved = 0
        for k, ip in enumerate(c.idx):
            P = c.P[0].copy()
            P[ip] += c.h[k]
            st, m, _, _ = pkg.build_mode_table(c.star.model_id, P, c.star.plength, c.star.x)
            assert st == 0 and m.size == base.size
            moved += int(np.any((m["i0"] != base["i0"]) | (m["i1"] != base["i1"])))
        assert moved >= 1
    if name == "corner_negnoise":
        assert np.sum(c.P[0][c.noise_index] < 0) == 2


def test_rows_cases_cross_the_lane_pass():
    assert [ac.ROWS[n][3] for n in ("rows64", "rows68", "rows132")] == [64, 68, 132]


@pytest.fixture(scope="module")
def corner_ref(pkg, synth):
    """(table, noise, nh, x, y, (G, Gabs, Gn, Gnabs) as Decimals) of the corner case's own vector."""
    c = ac.case(synth, "corner")
    m, nz, nh = _host_table(pkg, c)
    y = ac.spectrum(pkg, c)
    return m, nz, nh, c.star.x, y, ar.table_adjoint_exact(m, nz, nh, c.star.x, y)


def test_reference_holds_to_25_digits_under_step_halving(corner_ref):
    """Central differences at REL and REL / 2: every entry moves by less than 1e-25 of its absolute sum (the O(h^2) term is ~1e-43)."""
    m, nz, nh, x, y, (G, Ga, Gn, Gna) = corner_ref
    G2, _, Gn2, _ = ar.table_adjoint_exact(m, nz, nh, x, y, rel=ar.REL / 2)
    worst = Decimal(0)
    for a, b, s in [(G[j][f], G2[j][f], Ga[j][f]) for j in range(len(G)) for f in range(ar.NF)] + list(zip(Gn, Gn2, Gna)):
        assert (s == 0) == (a == 0) and (a == 0) == (b == 0)
        if s != 0:
            worst = max(worst, abs(a - b) / s)
    print("\nstep halving: worst move %.2e of the entry's absolute sum" % worst)
    assert worst <= Decimal("1e-25")
    assert sum(1 for row in G for v in row if v != 0) >= 3 * len(G)


def test_height_entries_are_the_direct_sums(corner_ref):
    """M is linear in hv_m, so the central difference is exact: G[row][7+m] = sum_i r_i A_i / q_i evaluated directly at 100 digits; and the
    last noise entry is sum_i r_i."""
    m, nz, nh, x, y, (G, Ga, Gn, Gna) = corner_ref
    import tile_reference as tr
    M = tr.model_row_exact(m, nz, nh, len(nz), x)
    with localcontext() as ctx:
        ctx.prec = ar.WORK
        r = [(1 - Decimal(float(y[i])) / M[i]) / M[i] for i in range(len(x))]
        for j, row in enumerate(m):
            g, a, fc = Decimal(float(row["gamma"])), Decimal(float(row["asym"])), Decimal(float(row["fc"]))
            for k in range(2 * int(row["l"]) + 1):
                s = Decimal(0)
                for i in range(max(int(row["i0"]), 0), min(int(row["i1"]), len(x))):
                    xi = Decimal(float(x[i]))
                    t = 2 * (xi - Decimal(float(row["nu"][k]))) / g
                    A = (1 + a * (xi / fc - 1)) ** 2 + (g * a / (2 * fc)) ** 2
                    s += r[i] * A / (1 + t * t)
                assert abs(s - G[j][7 + k]) <= Decimal("1e-60") * Ga[j][7 + k], (j, k)
        assert abs(sum(r) - Gn[-1]) <= Decimal("1e-90") * Gna[-1]


def test_zeros_where_the_rules_say_zero(pkg, synth, corner_ref):
    """Components m >= 2l+1; the three entries of a Harvey term with tau = 0; asym and fc where the row's asym is 0 (the id 14 star)."""
    m, nz, nh, x, y, (G, Ga, Gn, Gna) = corner_ref
    for j, row in enumerate(m):
        nc = 2 * int(row["l"]) + 1
        assert all(G[j][f] == 0 and Ga[j][f] == 0 for f in list(range(nc, 7)) + list(range(7 + nc, 14)))
        assert all(G[j][f] != 0 for f in list(range(nc)) + list(range(7, 7 + nc)) + [14, 15, 16])
    assert nz[4] == 0.0 and all(Gn[3 + f] == 0 and Gna[3 + f] == 0 for f in range(3)) and all(Gn[f] != 0 for f in (0, 1, 2, 6))
    c = ac.case(synth, "id14")
    t, nzz, nhh = _host_table(pkg, c)
    assert np.all(t["asym"] == 0.0)
    G0, _, Gn0, _ = ar.cached_table_adjoint(t, nzz, nhh, c.star.x, ac.spectrum(pkg, c))
    assert not G0[:, 15:].any() and np.all(G0[:, 14] != 0) and Gn0.size == 1 and Gn0[0] != 0


@pytest.mark.parametrize("name", ac.FIELD_CASES)
def test_numpy_yardstick_within_1e13_of_the_definition(pkg, synth, name):
    """adjoint_numpy.table_adjoint -- the closed forms k_adj_rows shares -- against the field-space differences: every entry within
    1e-13 of the entry's absolute sum (two orders under the device tolerance).  The (gamma asym / (2 fc))^2 terms are ~1e-5 of A: a
    sign or factor slip in their derivatives would stand at 1e-5 here."""
    c = ac.case(synth, name)
    m, nz, nh = _host_table(pkg, c)
    y = ac.spectrum(pkg, c)
    G, Ga, Gn, Gna = ar.cached_table_adjoint(m, nz, nh, c.star.x, y)
    Gw, Gaw, Gnw, Gnaw = an.table_adjoint(m, nz, nh, c.star.x, y)
    assert np.count_nonzero(G) >= 3 * m.size and np.all((G == 0) == (Gw == 0)) and np.all((Gn == 0) == (Gnw == 0))
    rG = np.abs(Gw - G) / np.where(Ga > 0, Ga, 1.0)
    rN = np.abs(Gnw - Gn) / np.where(Gna > 0, Gna, 1.0)
    print("\n%s: numpy yardstick, worst entry at %.2e of its absolute sum (fields), %.2e (noise)" % (name, rG.max(), rN.max()))
    assert np.all(np.abs(Gw - G) <= 1e-13 * Ga) and np.all(np.abs(Gnw - Gn) <= 1e-13 * Gna)
    assert np.all(np.abs(Gaw - Ga) <= 1e-12 * Ga) and np.all(np.abs(Gnaw - Gna) <= 1e-12 * Gna)   # (the scales agree too)


@pytest.mark.parametrize("name", ["corner", "rows68_asym", "rows64"])
def test_exact_contraction_against_the_numpy_contraction(pkg, synth, name):
    """contract_exact against adjoint_numpy.contract (products of doubles rounded, then summed in long double) on host tables, every
    component: within (3 + n 2^-11) 2^-53 abs_sum, n the terms -- a term's difference and product are rounded to double, the result is
    rounded to double once more for the comparison, and the long-double sum adds 2^-64 per term.  The
    asymmetry component contracts G[15] when the base asymmetry is not 0 and is exactly 0 when it is; and dS_from_gradient inverts a
    re-statement of assemble_gradient's two roundings within 3 x 2^-53 |dS|."""
    c = ac.case(synth, name)
    m, nz, nh = _host_table(pkg, c)
    G, _, Gn, _ = an.table_adjoint(m, nz, nh, c.star.x, ac.spectrum(pkg, c))
    nterms = m.size * 17 + nz.size
    seen = set()
    for k, ip in enumerate(c.idx):
        P = c.P[0].copy()
        P[ip] += c.h[k]
        st, t, nzz, _ = pkg.build_mode_table(c.star.model_id, P, c.star.plength, c.star.x)
        assert st == 0
        fields = set()
        dS, ab = ar.contract_exact(G, Gn, m, nz, t, nzz, nz.size, fields)
        seen |= fields
        want = an.contract(G, Gn, m, nz, t, nzz)
        assert abs(Fraction(float(want)) - dS) <= Fraction((3 + nterms * 2.0 ** -11) * U) * ab, (k, float(dS), float(want))
        if k == c.k_asym:
            assert (fields == {15} and dS != 0) if c.asym != 0 else (dS == 0 and ab == 0 and not fields)
        for T in ac.TEMPS:   # assemble_gradient: (double)((long double)(-(long)p dS) / T) / happ
            dSf = float(dS)
            happ = (P[ip] - c.P[0][ip])
            g = float(np.longdouble(-int(ac.P_EXP)) * np.longdouble(dSf) / np.longdouble(T)) / happ
            back = ar.dS_from_gradient(g, c.P[0][ip], c.h[k], T, ac.P_EXP)
            assert abs(back - Fraction(dSf)) <= 3 * Fraction(U) * abs(Fraction(dSf))
    assert len(seen) >= 3 and 17 in seen

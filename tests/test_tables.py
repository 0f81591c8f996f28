"""Host table builder (tamcmc_build_mode_table, no GPU) against the 50-digit table reference, row by row and field by field, on every
case of tests/table_cases.py: ids 3, 11, 12, 13, 14, 23.

Exactly: status, row count and order, l, flags, nharvey, nnoise; bit for bit the input: fc, asym, gamma of an l = 0 row, the |noise| row;
unused nu / hv entries exactly 0; windows equal to the reference's outside the knife-edge rows (none in these cases);
nu, hv and interpolated gamma within K 2^-52 scale (tests/table_check.py).

Worst ratios measured for the host builder: DESIGN.md section 5.
"""
import pytest

import table_cases as tc
import table_check as chk
import table_reference as tr


@pytest.mark.parametrize("model_id", tc.IDS)
def test_host_builder_against_reference(pkg, model_id):
    tally = chk.Tally()
    for g in tc.groups(model_id):
        for i, p in enumerate(g.vectors):
            st, mults, noise, nh = pkg.build_mode_table(model_id, p, g.plength, g.x)
            chk.check_table(g, i, st, mults, noise, nh, len(noise), tally, fail_rule="host", label="host")
    print(f"host id {model_id}: {tally}")
    assert tally.rows > 1000 and tally.exempt == []


def test_row_count_rule_matches_the_library(pkg):
    """count_rows of the reference is what the builder reports for a capacity of zero rows."""
    for model_id in tc.IDS:
        for g in tc.groups(model_id)[:5]:
            st, mults, _, _ = pkg.build_mode_table(model_id, g.vectors[0], g.plength, g.x)
            assert st == tr.OK and len(mults) == g.per == len(g.reference(0)["rows"])

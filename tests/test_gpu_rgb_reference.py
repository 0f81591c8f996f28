"""The red-giant pre-step on the device against its 50-digit definition (tests/rgb_reference.py), on the cases of tests/rgb_cases.py.

Paths: tamcmc_hip_rgb_mixed_modes (host unpack, device solver, sort / unique / bias / zeta kernels) with the structured scan and with the
dense walk, and tamcmc_hip_rgb_batch_tables in STRICT (host unpack in long double) and FAST (device unpack, one thread per vector).
Every value is held to K 2^-52 scale with K = 4 (tests/rgb_check.py); l, flags, row count and order, nharvey, nnoise, status and the
windows are compared exactly.  No case sits on a knife edge (asserted from the reference alone in tests/test_rgb_reference.py), so nothing
is exempt.  The worst ratios per field and path are printed.

The device-resident sampler (proposal-kernel unpack by one wave with amplitude_ratios_lanes, the pre-step per chain group, b0 > 0) is held
through tamcmc_sampler_get_tables, which accepts ids 25 and 27 on the random-walk engine."""
import numpy as np
import pytest

import rgb_cases as rc
import rgb_check as chk
import rgb_reference as rr

pytestmark = pytest.mark.gpu

CASES = rc.all_cases()
GOOD = [c for c in CASES if c.expect.get("status", rr.OK) == rr.OK]
REFUSED = [c for c in CASES if c.expect.get("status", rr.OK) != rr.OK]
BATCHED = rc.BATCHED


def _ctx(pkg, case, precision=None):
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST if precision is None else precision)
    ctx.set_spectrum(case.x, np.ones_like(case.x))
    return ctx


@pytest.mark.parametrize("case", GOOD, ids=str)
def test_mixed_modes_match_the_definition_on_both_scans(pkg, case):
    """nu_m, zeta and h1_h0 of every case within K 2^-52 scale of the definition; the structured scan and the dense walk agree bit for bit."""
    ctx = _ctx(pkg, case)
    try:
        out = {}
        for dense in (0, 1):
            ctx.set_option(pkg.OPT_ARMM_DENSE_SCAN, dense)
            out[dense] = ctx.rgb_mixed_modes(case.model_id, case.params, case.plength)
        for a, b in zip(out[0], out[1]):
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), case
        tally = chk.Tally()
        nu, z, h = out[0]
        chk.check_modes(case, nu, z, h, tally, "rgb_mixed_modes")
        print("rgb_mixed_modes", case, tally)
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["STRICT", "FAST"])
@pytest.mark.parametrize("case", GOOD + [c for c in REFUSED if c.expect.get("over_cap")], ids=str)
def test_batch_table_of_every_case(pkg, case, prec):
    """The case's vector as a one-slot batch: every row field against the definition, the windows exactly; a second call gives the same bits."""
    ctx = _ctx(pkg, case, getattr(pkg, "PRECISION_" + prec))
    try:
        none = np.zeros(0, dtype=np.int32)
        tabs, noise, nh, status = ctx.rgb_batch_tables(case.model_id, case.params, case.plength, none, np.zeros(0))
        tally = chk.Tally()
        # (more than 400 mixed modes is found out by the row kernel, after the unpack has left the vector's own noise row: no placeholder)
        chk.check_rows(case, status[0], tabs[0], noise[0], int(nh[0]), len(noise[0]), tally, prec, placeholder=not case.expect.get("over_cap"))
        tabs2, noise2, nh2, status2 = ctx.rgb_batch_tables(case.model_id, case.params, case.plength, none, np.zeros(0))
        assert tabs[0].tobytes() == tabs2[0].tobytes() and np.array_equal(status, status2) and np.array_equal(noise[0], noise2[0])
        print("rgb_batch_tables", prec, case, tally)
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["STRICT", "FAST"])
@pytest.mark.parametrize("name", BATCHED)
def test_batch_with_perturbed_slots_and_a_refused_vector(pkg, name, prec):
    """Three chains -- the case, the same vector with its radial ladder reversed (refused), the case again -- each with six perturbed
    slots (period spacing, coupling, delta0l, one radial frequency, inclination, Hfactor): every slot of the good chains against its own
    reference, the two good chains bit-identical, every slot of the refused chain empty with the placeholder noise row and its status."""
    case = rc.by_name(name)
    idx, h, slots = rc.perturbed(case)
    L = rr.Layout(case.plength)
    bad = case.params.copy()
    bad[L.o0:L.o0 + L.Nfl0] = bad[L.o0:L.o0 + L.Nfl0][::-1]
    P = np.stack([case.params, bad, case.params])
    ctx = _ctx(pkg, case, getattr(pkg, "PRECISION_" + prec))
    try:
        tabs, noise, nh, status = ctx.rgb_batch_tables(case.model_id, P, case.plength, idx, h)
        n = idx.size + 1
        tally = chk.Tally()
        for k, c in enumerate([case] + slots):
            chk.check_rows(c, status[k], tabs[k], noise[k], int(nh[k]), len(noise[k]), tally, f"{prec} slot {k}", placeholder=True)
            assert tabs[k].tobytes() == tabs[2 * n + k].tobytes() and status[2 * n + k] == status[k], (name, k)
        for k in range(n, 2 * n):
            # (the slot that perturbs the radial frequency of a reversed ladder is still a decreasing ladder)
            assert status[k] == rr.ERR_BAD_ARG and len(tabs[k]) == 0 and nh[k] == 0 and len(noise[k]) == 1 and noise[k][0] == 1.0, (name, k, status[k])
        print("rgb_batch_tables slots", prec, name, tally)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", [c for c in REFUSED if not c.expect.get("over_cap")], ids=str)
def test_refusals_carry_their_status_on_every_path(pkg, case):
    ctx = _ctx(pkg, case)
    try:
        with pytest.raises(pkg.TamcmcError) as e:
            ctx.rgb_mixed_modes(case.model_id, case.params, case.plength)
        assert e.value.code == case.expect["status"]
        for prec in (pkg.PRECISION_STRICT, pkg.PRECISION_FAST):
            ctx.set_option(pkg.OPT_PRECISION, prec)
            try:
                tabs, noise, nh, status = ctx.rgb_batch_tables(case.model_id, case.params, case.plength, np.zeros(0, dtype=np.int32), np.zeros(0))
            except pkg.TamcmcError as err:       # a layout the entry refuses as a whole, before any slot is looked at
                assert err.code == case.expect["status"], (case, prec, err.code)
                continue
            assert status[0] == case.expect["status"] and len(tabs[0]) == 0, (case, prec, status)
    finally:
        ctx.close()


def _sampler_tables(pkg, star, ctx, nchains, iterations):
    from tamcmc_c_amd.sampler import default_errors
    s = pkg.Sampler(ctx, star, nchains=nchains, lambda_temp=1.3, seed=17, engine="device", Nt_learn=(10 ** 9, 10 ** 9 + 1), periods_learn=(1,),
                    init_errors=6.0 * default_errors(star))
    try:
        assert s.tables()["scheme"] == 0
        s.run(iterations)
        return s.tables()
    finally:
        s.close()


@pytest.mark.parametrize("cte", [False, True], ids=["id25", "id27"])
def test_sampler_tables_match_the_definition(pkg, oracle, synth, cte):
    """The device-resident random-walk engine (proposal-kernel unpack by one wave, amplitude_ratios_lanes, the pre-step per chain group):
    after 12 iterations with wide proposals, every chain's table as tamcmc_sampler_get_tables returns it against the definition built
    from the engine's own params_prop -- 4 chains (one group) and 16 chains (four groups, b0 > 0).  A proposal the prior rejects holds the
    placeholder.  After ONE iteration the first four chains of both samplers have drawn the same proposals (same seed, same streams):
    their tables must be bit-identical between one group and four."""
    star = synth.make_c5_star(nx=3000, nmax=5, nferr=4, cte_width=cte)
    st, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    assert st == 0
    star.set_spectrum_from_model(m0, 4)
    ctx = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    ctx.set_spectrum(star.x, star.y)
    try:
        first = {n: _sampler_tables(pkg, star, ctx, n, 1) for n in (4, 16)}
        same = [m for m in range(4) if first[4]["params"][m].tobytes() == first[16]["params"][m].tobytes()]
        assert same, "the first four chains of the two samplers drew different first proposals"
        for m in same:
            assert first[4]["tables"][m].tobytes() == first[16]["tables"][m].tobytes() and first[4]["status"][m] == first[16]["status"][m], m
            assert first[4]["noise"][m].tobytes() == first[16]["noise"][m].tobytes(), m
        tally, held, moved, exempt = chk.Tally(), 0, 0, []
        for n in (4, 16):
            t = _sampler_tables(pkg, star, ctx, n, 12)
            assert t["scheme"] == 1 and len(t["tables"]) == n
            o1 = rr.Layout(star.plength).o1
            for m in range(n):
                tag = f"sampler-{'cte' if cte else 'app'}-{n}-{m}"
                if not np.isfinite(t["logprior"][m]):
                    assert len(t["tables"][m]) == 0 and t["nnoise"][m] == 1 and t["nharvey"][m] == 0 and t["noise"][m][0] == 1.0 and t["status"][m] != 0, tag
                    continue
                case = rc.adhoc(tag, star.model_id, t["params"][m], star.plength, star.x)
                if chk.exempt(case):
                    exempt.append(tag)
                    continue
                chk.check_rows(case, t["status"][m], t["tables"][m], t["noise"][m], int(t["nharvey"][m]), int(t["nnoise"][m]), tally, tag, placeholder=True)
                held += 1
                moved += (t["params"][m][o1 + 1] != star.params[o1 + 1]) and (t["params"][m][o1 + 3] != star.params[o1 + 3])
        print("sampler", "id27" if cte else "id25", tally, "held", held, "moved", moved, "exempt", exempt)
        assert exempt == [], exempt          # (fixed seed: no chain's proposal sits on a knife edge)
        assert held >= 12 and moved >= 10
    finally:
        ctx.close()


def test_over_the_row_cap_is_refused_by_mixed_modes_too(pkg):
    case = rc.by_name("over-row-cap")
    ctx = _ctx(pkg, case)
    try:
        with pytest.raises(pkg.TamcmcError) as e:
            ctx.rgb_mixed_modes(case.model_id, case.params, case.plength)
        assert e.value.code == rr.ERR_BAD_ARG
    finally:
        ctx.close()

"""The three device table builders against the 50-digit table reference (-m gpu), row by row and field by field.

    gradient batch    k_fd_unpack -> wg_unpack(live): HipContext.fd_batch_tables, with a prior class (the log-prior's last lane prepares the
                      unpack) and with none, every case of tests/table_cases.py plus each vector with one parameter perturbed
    lockstep step     k_iterate -> wg_log_prior(vis_in_prior, early_rows) -> wg_unpack(vis_done, rows_done): Sampler.tables() after
                      random-walk iterations under TAMCMC_OPT_STEP_SCHEME = 1.  The ONLY path on which the rows are written with hv = H
                      and multiplied by the visibilities afterwards (e / 7, e % 7)
    fused step        role_rows -> wg_unpack(empty_on_fail): Sampler.tables() after a fused stretch (info() says fused iterations ran),
                      every candidate slot a launch has written, against the candidate vector stored for the same slot

Every slot is compared with the reference evaluated on the vector that slot was built from: the batch's own rule for the gradient batch
(theta, theta + h e_k in double), the engine's own buffers for the sampler (tamcmc_sampler_get_tables).  What is asserted: tests/table_check.py.
A failed slot: the placeholder (no rows, nn = 1, noise[0] = 1) for the batch and the lockstep step, the empty slot (nn = 0) for the fused
step; its neighbours are compared like every other slot.

Host against device (the claim at the head of csrc/mode_tables_impl.h): i0 and i1 equal on every row, no exemption; nu, and hv where the
heights do not pass through the Wigner sum (ids 12, 13, 14), within HOST_DEV_ULP units of the last place of the row's largest component.
Where they do (ids 3, 11, 23) the two builders evaluate different formulas, and the distance is bounded in the reference's scale:
|hv_host - hv_dev| <= K_WIGNER_HD 2^-52 hv_scale.  Per Wigner term, in units of 2^-52 of the term: the device's repeated multiplication
rounds 2l = 6 times (3), the host's two pow() and two products 3; the two libraries' sine and cosine are each within an ulp of the true
value, so within 2 of each other, and enter with the exponents a + b = 2l: 12; summing and normalising (at most four additions, two
square roots, a product and a quotient on either side, half an ulp each): 8.  Together 26 of norm x sum |terms|; squaring doubles it, the
product with H adds 1: K_WIGNER_HD = 53.  Measured figures: DESIGN.md section 5 (13 ulp of the largest component, 9.9 of the scale).
"""
import numpy as np
import pytest

import table_cases as tc
import table_check as chk
import table_reference as tr
from strict_numpy import eval_table

pytestmark = pytest.mark.gpu

HOST_DEV_ULP = {"nu": 2, "hv": 2}
K_WIGNER_HD = 53.0
WIGNER_IDS = (tr.CLASSIC, tr.LOCAL, tr.AJ)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
    yield c
    c.close()


class _Prior:
    """A prior of the model's class that every vector passes through: no primitive (every switch 0), the extra block of the model's
    loader.  The table does not depend on what the prior says; the path in front of the unpack does."""

    def __init__(self, model_id, n):
        self.prior_class = 3 if model_id in (tr.LOCAL, tr.HNLM) else 2
        self.priors = np.full((4, n), -9999.0)
        self.priors_switch = np.zeros(n, dtype=np.int32)
        self.extra_priors = {tr.AJ: [0, 2, 0, .2, .2, .2, .2, .2, 0, 9], tr.CLASSIC: [0, 2, 0, .2, .2, .2, .2, .2, 0, -1],
                             tr.V2: [0, 2, 0, .2, .2, .2, .2, .2, 1, -1], tr.LOCAL: [0, 0, .2, 0, 0, 0, 0, 0, 0, 0],
                             tr.HNLM: [0, 0, .2, 2, 0, 0, 0, 0, 0, 0]}[model_id]


def _host_vs_device(pkg, g, i, dev_rows, worst):
    """i0, i1 bit for bit; nu and hv in units of the last place of the row's largest magnitude of that field."""
    st, host, _, _ = pkg.build_mode_table(g.model_id, g.vectors[i], g.plength, g.x)
    if st != tr.OK:
        return
    assert np.array_equal(host["i0"], dev_rows["i0"]) and np.array_equal(host["i1"], dev_rows["i1"]), (g.name, g.names[i])
    for f in ("nu", "hv"):
        ulp = np.spacing(np.maximum(np.abs(host[f]).max(axis=1), np.abs(dev_rows[f]).max(axis=1)))
        d = np.abs(host[f] - dev_rows[f]).max(axis=1)
        r = np.where(d > 0, d / np.where(ulp > 0, ulp, 1.0), 0.0)
        k = int(np.argmax(r))
        if r[k] > worst[f][0]:
            worst[f] = (float(r[k]), f"{g.name}[{g.names[i]}] row {k}")
    if g.model_id in WIGNER_IDS:
        for k, want in enumerate(g.reference(i)["rows"]):
            for c in range(2 * want["l"] + 1):
                r = tr.ratio(dev_rows["hv"][k][c], float(host["hv"][k][c]), want["hv_scale"][c])
                if r > worst["hv_scale"][0]:
                    worst["hv_scale"] = (r, f"{g.name}[{g.names[i]}] row {k} k={c}")


def _perturbed(g):
    """The group with one more vector per vector: the last frequency of the table moved by 2^-20 of its value (the batch's slot 1)."""
    L = tr.Layout(g.plength)
    idx = L.o_split - 1
    h = np.array([g.vectors[0][idx] * 2.0 ** -20])
    q = tc.Group(g.name + "+h", g.model_id, g.plength, g.x, g.directed)
    for i, p in enumerate(g.vectors):
        q.add(g.names[i], p)
        pp = p.copy()
        pp[idx] = p[idx] + h[0]
        q.add(g.names[i] + "+h", pp)
    # (the exact decisions of the unperturbed vectors; a clipped lower edge x_last - c stays on the grid wherever the mode moves to)
    q.exact_edges = {(2 * i, r, n) for i, r, n in g.exact_edges} | {(2 * i + 1, r, n) for i, r, n in g.exact_edges if n == "i0"}
    return q, np.array([idx], dtype=np.int32), h


@pytest.mark.parametrize("model_id", tc.IDS)
def test_gradient_batch_tables(pkg, ctx, model_id):
    """Slots [0, C (Nvars + 1)) of a gradient batch as k_fd_unpack leaves them: no prior class (Nvars = 1: base and perturbed vector) and,
    where the model has a prior, its class (Nvars = 0)."""
    tally, tally_p, worst = chk.Tally(), chk.Tally(), {k: (0.0, None) for k in ("nu", "hv", "hv_scale")}
    none = np.zeros(0, dtype=np.int32)
    for g in tc.groups(model_id):
        ctx.set_spectrum(g.x, np.ones(g.x.size))
        q, idx, h = _perturbed(g)
        tabs, noise, nh, nn, status = ctx.fd_batch_tables(model_id, g.params, g.plength, idx, h)
        assert len(tabs) == 2 * len(g.vectors)
        for s in range(len(tabs)):
            chk.check_table(q, s, int(status[s]), tabs[s], noise[s], int(nh[s]), int(nn[s]), tally, fail_rule="placeholder", label="batch")
            if status[s] == tr.OK:
                _host_vs_device(pkg, q, s, tabs[s], worst)
        if model_id == tr.V3:
            continue  # (id 13 has no prior the reference can run: include/tamcmc_hip.h)
        tabs, noise, nh, nn, status = ctx.fd_batch_tables(model_id, g.params, g.plength, none, np.zeros(0), star=_Prior(model_id, g.params.shape[1]))
        assert len(tabs) == len(g.vectors)
        for s in range(len(tabs)):
            chk.check_table(g, s, int(status[s]), tabs[s], noise[s], int(nh[s]), int(nn[s]), tally_p, fail_rule="placeholder", label="batch+prior")
    print(f"batch id {model_id}: {tally}")
    print(f"batch+prior id {model_id}: {tally_p}")
    print(f"host-device ulp id {model_id}: {worst}")
    assert tally.rows > 2000 and tally.exempt == [] and tally_p.exempt == []
    assert worst["nu"][0] <= HOST_DEV_ULP["nu"], worst["nu"]
    if model_id in WIGNER_IDS:
        assert worst["hv_scale"][0] <= K_WIGNER_HD, worst["hv_scale"]
    else:
        assert worst["hv"][0] <= HOST_DEV_ULP["hv"], worst["hv"]


# ---- the sampler's two schemes: stars of tamcmc_c_amd.synth with their own priors, small grids

def _star(pkg, synth, model_id, variant):
    if model_id == tr.AJ:
        nmax, lmax = ((16, 3), (17, 2), (3, 1))[variant]
        s = synth.make_c3_star(nx=2600, nmax=nmax, lmax=lmax, step=1.0, fmin=1950.0)
    elif model_id == tr.CLASSIC:
        s = synth.make_classic_star(nx=2600, nmax=(16, 5, 2)[variant], lmax=(3, 2, 1)[variant], step=1.0, fmin=1950.0)
    elif model_id == tr.V2:
        s = synth.make_v2_star(nx=2600, nmax=(16, 5, 2)[variant], lmax=(3, 2, 1)[variant], step=1.0, fmin=1950.0)
    elif model_id == tr.LOCAL:
        s = synth.make_c2_star(nx=(1500, 4097, 700)[variant])
    else:
        s = synth.make_hnlm_star(nx=(1500, 4097, 700)[variant])
    if model_id == tr.V2:
        # (the star's ratios sum to exactly 1, the edge of their prior's support: two proposals in three would leave it and the lockstep
        # step would not unpack them)
        o_inc = int(s.plength[:9].sum())
        s.params[o_inc:o_inc + 9] *= 0.9
    if variant == 2:
        # the truncation parameter free and small: about half of the proposals have c < 0, whose windows are empty -- failed tables
        # between good ones
        o_cfg = int(s.plength[:10].sum())
        s.params[o_cfg] = 0.002
        s.relax[o_cfg] = 1
        s.priors[:2, o_cfg] = (-100.0, 100.0)
        s.priors_switch[o_cfg] = synth.P_UNIFORM
    st, mults, noise, nh = pkg.build_mode_table(s.model_id, s.params, s.plength, s.x)
    assert st == tr.OK
    s.set_spectrum_from_model(eval_table(mults, noise, nh, s.x), seed=7)
    return s


def _errors(pkg, star):
    err = pkg.sampler.default_errors(star)
    o_cfg = int(star.plength[:10].sum())
    free = np.flatnonzero(star.relax == 1)
    err[free == o_cfg] = 0.5
    return err


def _check_sampler_slots(pkg, g_name, star, t, tally, fail_rule, label):
    """Every written slot of Sampler.tables() against the reference on the vector the engine stored for it, and its windows against the
    host builder's on the same vector."""
    hd = {k: (0.0, None) for k in ("nu", "hv", "hv_scale")}
    g = tc.Group(g_name, star.model_id, star.plength, star.x, False)
    failed = notlive = 0
    for s in range(len(t["tables"])):
        if not t["written"][s]:
            assert len(t["tables"][s]) == 0
            continue
        i = g.add(f"slot{s}", t["params"][s])
        if fail_rule == "placeholder" and not np.isfinite(t["logprior"][s]):
            # lockstep: a proposal outside the prior's support is not unpacked (model_def.cpp:472): the placeholder
            assert len(t["tables"][s]) == 0 and t["nnoise"][s] == 1 and t["noise"][s][0] == 1.0 and t["nharvey"][s] == 0, (label, s)
            notlive += 1
            continue
        failed += t["status"][s] != tr.OK
        chk.check_table(g, i, int(t["status"][s]), t["tables"][s], t["noise"][s], int(t["nharvey"][s]), int(t["nnoise"][s]), tally,
                        fail_rule=fail_rule, label=label)
        if t["status"][s] == tr.OK:
            _host_vs_device(pkg, g, i, t["tables"][s], hd)
    return np.array([failed, notlive])


SAMPLER_IDS = (tr.AJ, tr.CLASSIC, tr.V2, tr.LOCAL, tr.HNLM)   # (id 13 has no sampler: include/tamcmc_hip.h)


@pytest.mark.parametrize("model_id", SAMPLER_IDS)
def test_lockstep_iteration_tables(pkg, synth, model_id):
    """The tables of the last lockstep random-walk iteration against the reference on params_prop.  The visibility product of this path is
    applied to finished rows afterwards (wg_unpack, rows_done): a component it leaves out keeps hv = H and shows in hv here alone.
    Slots that hold the placeholder: a table that failed (io_local: a negative truncation parameter passes the prior and its windows are
    empty) or a proposal outside the prior's support, which this path does not unpack (io_MS_Global rejects that parameter)."""
    tally, failed, slots = chk.Tally(), np.zeros(2, dtype=int), 0
    for variant in range(3):
        star = _star(pkg, synth, model_id, variant)
        c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
        c.set_spectrum(star.x, star.y)
        c.set_option(pkg.OPT_STEP_SCHEME, 1)
        smp = pkg.Sampler(c, star, engine="device", nchains=5, lambda_temp=1.4, seed=11 + variant, Nt_learn=(10 ** 9, 10 ** 9 + 1),
                          periods_learn=(1,), init_errors=_errors(pkg, star))
        assert smp.tables()["scheme"] == 0
        for n in (1, 2, 3):
            smp.run(n, record=False)
            t = smp.tables()
            assert t["scheme"] == 1 and len(t["tables"]) == 5 and t["written"].all()
            failed += _check_sampler_slots(pkg, f"lockstep-id{model_id}-v{variant}-n{n}", star, t, tally, "placeholder", "lockstep")
            slots += 5
        info = smp.info()
        assert info["iter_lockstep"] == 6 and info["iter_fused"] == 0
        smp.close()
        c.close()
    print(f"lockstep id {model_id}: {tally} slots={slots} failed, not live={failed}")
    assert tally.rows > 50 and tally.exempt == [] and failed.sum() >= 1 and (failed[0] >= 1 or model_id not in (tr.LOCAL, tr.HNLM))


@pytest.mark.parametrize("model_id", SAMPLER_IDS)
def test_fused_stretch_tables(pkg, synth, model_id):
    """Every candidate slot a fused stretch has written against the reference on cand_params of the same slot; a failed table leaves an
    empty slot (nn = 0)."""
    tally, failed, slots = chk.Tally(), 0, 0
    for variant in range(3):
        star = _star(pkg, synth, model_id, variant)
        c = pkg.HipContext(0, precision=pkg.PRECISION_FAST)
        c.set_spectrum(star.x, star.y)
        nch = (7, 9, 7)[variant]
        c.set_option(pkg.OPT_STEP_SCHEME, 3 if nch >= 8 else 0)
        smp = pkg.Sampler(c, star, engine="device", nchains=nch, lambda_temp=1.4, seed=21 + variant, Nt_learn=(10 ** 9, 10 ** 9 + 1),
                          periods_learn=(1,), init_errors=_errors(pkg, star))
        smp.run(12, record=False)
        info = smp.info()
        assert info["fused_available"] == 1 and info["iter_fused"] == 12 and info["iter_lockstep"] == 0, info
        t = smp.tables()
        assert t["scheme"] == 2 and len(t["tables"]) == 3 * (2 * nch + 8)
        assert t["written"].sum() >= 2 * nch
        failed += _check_sampler_slots(pkg, f"fused-id{model_id}-v{variant}", star, t, tally, "empty", "fused")[0]
        slots += int(t["written"].sum())
        smp.close()
        c.close()
    print(f"fused id {model_id}: {tally} slots={slots} failed={failed}")
    assert tally.rows > 300 and tally.exempt == [] and failed >= 1

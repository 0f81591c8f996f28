"""Height-per-m models without a GPU: host table rows of ids 12, 13, 14 (model_MS_Global_a1etaa3_HarveyLike_Classic_v2 / _v3,
model_MS_local_Hnlm) against the inclination models the oracle knows (by conversion) and against the independent numpy restatement
tests/hnlm_numpy.py; the prior that goes with id 12; the two loaders.

Bounds.  Id 12 with ratios = amplitude_ratio(l, i) performs the operations of id 3: rows bit-identical.  Ids 13, 14 form a height as
|p / (pi W)| with p = H V r rounded twice, id 3 / 11 as |H / (pi W)| V r (or |H V| r): at most four roundings apart, asserted at 8 ulp.
Models (rows evaluated by strict_numpy.eval_table) against the oracle at 1e-12, the tolerance of smoke()."""
import os

import numpy as np
import pytest

import hnlm_numpy
from strict_numpy import eval_table

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = np.finfo(np.float64).eps


def _classic(synth, rng, lmax, nfreqs=6, do_amp=0.0, asym=-30.0):
    p, pl = synth.make_params_aj_model(rng, lmax=lmax, nfreqs=nfreqs, asym=asym, n_first=12)
    pc, plc = synth.aj_to_classic(p, pl)
    pc[plc[0] + plc[1] + plc[2:6].sum() + 2] = 0.01  # a3
    pc[-1] = do_amp
    return pc, plc


def _rows_equal_but_heights(a, b, hv_ulp):
    assert len(a) == len(b)
    for k in ("l", "i0", "i1", "fc", "gamma", "asym", "nu"):
        assert np.array_equal(a[k], b[k]), k
    err = np.abs(a["hv"] - b["hv"]) / np.maximum(np.abs(b["hv"]), 1e-300)
    assert err.max() <= hv_ulp * ULP, err.max() / ULP


@pytest.mark.parametrize("lmax,do_amp", [(1, 0.0), (2, 1.0), (3, 0.0), (3, 1.0)])
def test_v2_rows_are_bitwise_the_classic_rows(pkg, oracle, synth, lmax, do_amp):
    rng = np.random.default_rng(40 + lmax)
    pc, plc = _classic(synth, rng, lmax, do_amp=do_amp)
    x = synth.grid(50000, 1400.0, 0.02)
    st3, m3, nz3, nh3 = pkg.build_mode_table(3, pc, plc, x)
    p12, pl12 = synth.classic_to_v2(pc, plc, oracle.amplitude_ratio)
    assert pl12[9] == 9 and p12.size == pc.size + 8
    st, m12, nz, nh = pkg.build_mode_table(12, p12, pl12, x)
    assert st == st3 == 0 and nh == nh3
    assert m12.tobytes() == m3.tobytes() and np.array_equal(nz, nz3)
    _, ref = oracle.call_model(3, pc, plc, x)
    assert np.array_equal(eval_table(m12, nz, nh, x), ref)


@pytest.mark.parametrize("do_amp", [0.0, 1.0])
def test_v3_rows_follow_classic_where_the_offsets_do_not_bite(pkg, oracle, synth, do_amp):
    rng = np.random.default_rng(51)
    pc, plc = _classic(synth, rng, 1, do_amp=do_amp)
    x = synth.grid(50000, 1400.0, 0.02)
    _, m3, nz3, nh3 = pkg.build_mode_table(3, pc, plc, x)
    p13, pl13 = synth.classic_to_v3(pc, plc, oracle.amplitude_ratio)
    assert pl13[9] == 2 * plc[3]
    st, m13, nz, nh = pkg.build_mode_table(13, p13, pl13, x)
    assert st == 0 and nh == nh3
    _rows_equal_but_heights(m13, m3, 8)
    _, ref = oracle.call_model(3, pc, plc, x)
    assert np.max(np.abs(eval_table(m13, nz, nh, x) - ref) / ref) < 1e-12


def test_v3_reads_every_degree_from_the_start_of_the_block(pkg, oracle, synth):
    """The quirk kept from the reference (models.cpp:2427-2477): the heights of (n, l) are read at o_inc + (l+1) n, inside the l = 1
    heights for l >= 2.  Fails for the 'corrected' offsets o_inc + 2 Nfl1 (+ 3 Nfl2) + (l+1) n."""
    rng = np.random.default_rng(52)
    pc, plc = _classic(synth, rng, 3, nfreqs=5)
    p13, pl13 = synth.classic_to_v3(pc, plc, oracle.amplitude_ratio)
    o_inc = int(pl13[:9].sum())
    p13[o_inc:o_inc + pl13[9]] = 1.0 + np.arange(pl13[9])  # every slot its own value
    x = synth.grid(50000, 1400.0, 0.02)
    st, m, _, _ = pkg.build_mode_table(13, p13, pl13, x)
    assert st == 0 and len(m) == 20
    for n in range(5):
        for l in range(1, 4):
            r = m[4 * n + l]
            assert r["l"] == l
            want = [1.0 + (l + 1) * n + abs(k - l) for k in range(2 * l + 1)]
            assert np.array_equal(r["hv"][:2 * l + 1], want), (n, l)
    ref, nz, nh = hnlm_numpy.rows(13, p13, pl13, x)
    assert np.array_equal(ref["hv"], m["hv"])


def test_local_hnlm_rows_follow_local_basic(pkg, oracle, synth):
    """l <= 1 slice: same spectrum as model_MS_local_basic.  The stock C2 slice (l = 0, 1, 2): the l = 2 rows read at Nfl0 + Nfl1 + 3 n
    (models.cpp:3288-3293), inside the l = 1 heights -- pinned against the values by hand."""
    star = synth.make_c2_star()
    pl = star.plength.copy()
    keep = np.r_[0:4, 6:10, 12:18, 18:22, 24:28]  # drop the two l = 2 modes (heights, frequencies, widths)
    p01 = star.params[keep]
    pl01 = np.array([4, 0, 2, 2, 0, 0, 6, 4, 1, 1, 2], dtype=np.int32)
    for do_amp in (0.0, 1.0):
        p01[-1] = do_amp
        _, m11, nz11, nh11 = pkg.build_mode_table(11, p01, pl01, star.x)
        ph, plh = synth.local_to_hnlm(p01, pl01, oracle.amplitude_ratio)
        assert plh[0] == 2 + 2 * 2 and ph.size == p01.size + 2
        st, m14, nz, nh = pkg.build_mode_table(14, ph, plh, star.x)
        assert st == 0 and nh == 0
        _rows_equal_but_heights(m14, m11, 8)
        _, ref = oracle.call_model(11, p01, pl01, star.x)
        assert np.max(np.abs(eval_table(m14, nz, nh, star.x) - ref) / ref) < 1e-12
    ph, plh = synth.local_to_hnlm(star.params, pl, oracle.amplitude_ratio)
    assert plh[0] == 2 + 4 + 6
    ph[:12] = 1.0 + np.arange(12)
    st, m, _, _ = pkg.build_mode_table(14, ph, plh, star.x)
    assert st == 0 and [int(v) for v in m["l"]] == [0, 0, 1, 1, 2, 2]
    assert np.array_equal(m["hv"][2][:3], [4, 3, 4]) and np.array_equal(m["hv"][3][:3], [6, 5, 6])
    assert np.array_equal(m["hv"][4][:5], [7, 6, 5, 6, 7])     # from Nfl0 + Nfl1 = 4: slots 4, 5, 6 (the loader wrote them at 6, 7, 8)
    assert np.array_equal(m["hv"][5][:5], [10, 9, 8, 9, 10])   # 4 + 3: slots 7, 8, 9


@pytest.mark.parametrize("model_id,lmax,do_amp", [(12, 1, 0), (12, 3, 1), (13, 1, 1), (13, 2, 0), (13, 3, 1), (14, 1, 0), (14, 3, 1), (14, 2, 0)])
def test_host_rows_against_the_numpy_restatement(pkg, synth, model_id, lmax, do_amp):
    """Vectors that are NOT images of an inclination: asymmetric height patterns, one zero height."""
    rng = np.random.default_rng(1000 * model_id + 10 * lmax + do_amp)
    p, pl, x = random_vector(synth, rng, model_id, lmax, do_amp)
    st, m, nz, nh = pkg.build_mode_table(model_id, p, pl, x)
    assert st == 0
    ref, rnz, rnh = hnlm_numpy.rows(model_id, p, pl, x)
    assert nh == rnh and np.array_equal(nz, rnz) and len(m) == len(ref)
    for k in ("l", "i0", "i1", "fc", "gamma", "asym"):
        assert np.array_equal(m[k], ref[k]), k
    assert np.max(np.abs(m["nu"] - ref["nu"])) <= 4 * ULP * 4000.0
    assert np.max(np.abs(m["hv"] - ref["hv"]) / np.maximum(ref["hv"], 1e-300)) <= 4 * ULP
    a, b = eval_table(m, nz, nh, x), eval_table(ref, rnz, rnh, x)
    assert np.max(np.abs(a - b) / b) < 1e-12


def random_vector(synth, rng, model_id, lmax, do_amp, nfreqs=5):
    """A random vector of id 12 / 13 / 14 whose heights follow no inclination (also used by the GPU tests)."""
    if model_id in (12, 13):
        pc, plc = _classic(synth, rng, lmax, nfreqs=nfreqs, do_amp=float(do_amp), asym=float(rng.choice([0.0, 12.5])))
        conv = synth.classic_to_v2 if model_id == 12 else synth.classic_to_v3
        p, pl = conv(pc, plc)
        o = int(pl[:9].sum())
        if model_id == 12:
            p[o:o + 9] = rng.uniform(0.0, 0.6, 9) * rng.choice([1.0, -1.0], 9)  # the model takes |ratio|
        else:
            p[o:o + pl[9]] *= rng.uniform(0.2, 3.0, pl[9])
            p[o + 1] = 0.0
        x = synth.grid(40000, 1450.0, 0.02)
        return p, pl, x
    nfl = [3, 3, 2 if lmax >= 2 else 0, 2 if lmax >= 3 else 0]
    step = 1e6 / (365.0 * 86400.0)
    f = np.concatenate([(20 + np.arange(nfl[l]) + 0.45 + l / 2.0 - (l >= 2)) * 135.1 + rng.uniform(-0.5, 0.5, nfl[l]) for l in range(4)])
    ntot = sum(nfl)
    nh = nfl[0] + 2 * nfl[1] + 3 * nfl[2] + 4 * nfl[3]
    heights = rng.uniform(0.5, 20.0, nh) * (30.0 if do_amp else 1.0)
    heights[nfl[0] + 1] = 0.0
    split = [rng.uniform(0.3, 2.0), 3e-5, 0.01, 0.0, 0.0, float(rng.choice([0.0, 8.0]))]
    p = np.concatenate([heights, f, split, rng.uniform(0.5, 2.0, ntot), [0.1], [0.0], [30.0, float(do_amp)]])
    pl = np.array([nh, 0] + nfl + [6, ntot, 1, 1, 2], dtype=np.int32)
    x = synth.grid(12000, 2800.0, step)
    return p, pl, x


def test_short_height_blocks_are_refused(pkg, synth):
    """A height block one element shorter than what the model function reads is refused; the exact length is accepted."""
    rng = np.random.default_rng(5)
    pc, plc = _classic(synth, rng, 2)
    x = synth.grid(20000, 1400.0, 0.02)
    assert pkg.build_mode_table(12, pc, plc, x)[0] == pkg.ERR_BAD_MODEL   # Ninc = 1, nine ratios needed
    assert pkg.build_mode_table(13, pc, plc, x)[0] == pkg.ERR_BAD_MODEL
    o = int(plc[:9].sum())
    for model_id, need in ((12, 9), (13, 3 * plc[0])):   # id 13 reads up to o_inc + (lmax + 1) Nmax - 1
        for n, want in ((need - 1, pkg.ERR_BAD_MODEL), (need, 0)):
            p = np.concatenate([pc[:o], np.full(n, 0.3), pc[o + 1:]])
            pl = plc.copy()
            pl[9] = n
            assert pkg.build_mode_table(model_id, p, pl, x)[0] == want, (model_id, n)
    star = synth.make_c2_star()
    assert pkg.build_mode_table(14, star.params, star.plength, star.x)[0] == pkg.ERR_BAD_MODEL  # plength[0] = Nf
    ph, plh = synth.local_to_hnlm(star.params, star.plength)
    assert pkg.build_mode_table(14, ph, plh, star.x)[0] == 0
    short = plh.copy()
    short[0] -= 1                                          # (the vector keeps its length: only the declared block shrinks)
    assert pkg.build_mode_table(14, ph, short, star.x)[0] == pkg.ERR_BAD_MODEL


def test_v2_prior_needs_the_nine_ratios(pkg, synth):
    """extra_priors[8] = 1 on a layout whose inclination block is shorter than nine (an id-3 star): refused, nothing read past the end."""
    from tamcmc_c_amd import sampler
    s3 = synth.make_classic_star(nx=2000, nmax=6)
    s3.extra_priors[8] = 1
    v, st = sampler.log_prior(s3)
    assert st == pkg.ERR_BAD_MODEL and v == -np.inf


@pytest.mark.parametrize("lmax", [1, 2])
def test_v2_prior_below_lmax_3(pkg, oracle, synth, lmax):
    """The slots of the degrees above lmax are empty (0, fixed): their sums are 0, inside the support, and all three constants are added."""
    from tamcmc_c_amd import sampler
    star = synth.make_v2_star(oracle.amplitude_ratio, nx=2000, nmax=6, lmax=lmax)
    o = int(star.plength[:9].sum())
    used = {1: 2, 2: 5}[lmax]
    assert np.all(star.params[o + used:o + 9] == 0) and np.all(star.relax[o + used:o + 9] == 0) and np.all(star.relax[o:o + used] == 1)
    v, st = sampler.log_prior(star)
    want = hnlm_numpy.log_prior_v2(star, star.params)
    assert st == 0 and np.isfinite(v) and abs(v - want) <= 1e-15 * abs(want)
    s3 = synth.make_classic_star(nx=2000, nmax=6, lmax=lmax)
    v3, _ = sampler.log_prior(s3)
    assert abs((v - v3) - (np.log(90.0) - 3 * np.log1p(1e-10))) < 1e-11
    p = star.params.copy()
    p[o + 8] = 0.5 + 1e-9                                  # an unused l = 3 slot pushed over the edge still counts: 2 x that > 1 + 1e-10
    assert sampler.log_prior(star, p)[0] == -np.inf and hnlm_numpy.log_prior_v2(star, p) == -np.inf


# ---------------------------------------------------------------- prior of id 12
def test_v2_prior_against_long_double_numpy_at_the_edges_of_the_sums(pkg, oracle, synth):
    from tamcmc_c_amd import sampler
    star = synth.make_v2_star(oracle.amplitude_ratio, nx=2000, nmax=6)
    o = int(star.plength[:9].sum())
    v, st = sampler.log_prior(star)
    assert st == 0 and np.isfinite(v)                      # amplitude_ratio sums to 1 only to rounding: inside thanks to the 1e-10
    assert abs(v - hnlm_numpy.log_prior_v2(star, star.params)) <= 1e-15 * abs(v) + 1e-15
    s3 = synth.make_classic_star(nx=2000, nmax=6)
    v3, _ = sampler.log_prior(s3)
    # against the inclination star: the inclination's Uniform(0, 90) replaced by nine Uniform(0, 1) and three Uniform(0, 1 + 1e-10)
    assert abs((v - v3) - (np.log(90.0) - 3 * np.log1p(1e-10))) < 1e-11
    groups = {1: ([0, 1], [1, 2]), 2: ([2, 3, 4], [1, 2, 2]), 3: ([5, 6, 7, 8], [1, 2, 2, 2])}
    for l, (idx, w) in groups.items():
        for total, inside in ((0.5, True), (1.0, True), (1.0 + 0.5e-10, True), (1.0 + 2e-10, False), (0.0, True)):
            p = star.params.copy()
            p[[o + i for i in idx]] = 0.0
            p[o + idx[1]] = total / w[1]
            s = sum(wi * p[o + i] for i, wi in zip(idx, w))
            want = hnlm_numpy.log_prior_v2(star, p)
            got, st = sampler.log_prior(star, p)
            assert st == 0
            assert np.isfinite(want) == inside == np.isfinite(got), (l, total, s, got, want)
            if inside:
                assert abs(got - want) <= 1e-15 * abs(want)
        p = star.params.copy()                               # a negative sum with every ratio inside its own Uniform(0, 1)? impossible:
        p[[o + i for i in idx]] = 0.0
        p[o + idx[1]] = -1e-3                                # the generic prior rejects the negative ratio as well
        assert sampler.log_prior(star, p)[0] == -np.inf and hnlm_numpy.log_prior_v2(star, p) == -np.inf
        sw = star.priors_switch.copy()                       # ... so switch that ratio's own prior off: the sum alone decides
        star.priors_switch[o + idx[1]] = 0
        assert sampler.log_prior(star, p)[0] == -np.inf and hnlm_numpy.log_prior_v2(star, p) == -np.inf
        star.priors_switch[:] = sw
    star.extra_priors[8] = 2                                 # the reference exits there
    v, st = sampler.log_prior(star)
    assert st == pkg.ERR_BAD_MODEL and v == -np.inf


# ---------------------------------------------------------------- loaders
def _variant(tmp_path, src, name, edit):
    lines = open(os.path.join(GOLDEN, src)).read().split("\n")
    out = tmp_path / name
    out.write_text("\n".join(edit(lines)))
    return str(out)


def _fields(inp):
    return dict(params=np.array(inp.params), relax=np.array(inp.relax), priors=np.array(inp.priors), sw=np.array(inp.priors_switch),
                names=list(inp.names), prior_names=list(inp.prior_names), plength=np.array(inp.plength), extra=np.array(inp.extra_priors))


def test_local_hnlm_loader(pkg, oracle, tmp_path):
    from tamcmc_c_amd import inputs
    def rename(lines):
        return [ln.replace("model_MS_local_basic", "model_MS_local_Hnlm") if "model_fullname" in ln else ln for ln in lines]
    path = _variant(tmp_path, "TF_3443483_local-v3.model", "hnlm.model", rename)
    basic = _fields(inputs.LocalInputs(os.path.join(GOLDEN, "TF_3443483_local-v3.model"), 0, 0.008))
    hn = inputs.LocalInputs(path, 0, 0.008)
    assert hn.model_name == "model_MS_local_Hnlm" and hn.model_id == pkg.MODEL_MS_LOCAL_HNLM == 14 and hn.prior_class == 3
    h = _fields(hn)
    nfl = [int(v) for v in basic["plength"][2:6]]
    ntot, nh = sum(nfl), nfl[0] + 2 * nfl[1] + 3 * nfl[2] + 4 * nfl[3]
    assert basic["plength"][0] == ntot and h["plength"][0] == nh and np.array_equal(h["plength"][1:], basic["plength"][1:])
    assert h["extra"][3] == 2 and np.array_equal(np.delete(h["extra"], 3), np.delete(basic["extra"], 3))
    o_b, o_h = ntot + sum(nfl), nh + sum(nfl)   # first index of the splitting block
    # everything outside the height block, the inclination slot -- and Splitting_a1, which Hnlm keeps where basic rewrites the
    # block to sqrt(a1) cos i / sin i (slots 0, 3, 4)
    same = [k for k in range(ntot, basic["params"].size) if k - o_b not in (0, 3, 4)]
    for key in ("params", "relax", "sw"):
        assert np.array_equal(h[key][[k - ntot + nh for k in same]], basic[key][same]), key
    assert np.array_equal(h["priors"][:, [k - ntot + nh for k in same]], basic["priors"][:, same])
    assert h["names"][o_h] == "Splitting_a1" and h["params"][o_h] == 0.4 and h["prior_names"][o_h] == "Uniform"
    assert tuple(h["priors"][:2, o_h]) == (0.0, 1.5) and h["params"][o_h + 3] == 0 and h["params"][o_h + 4] == 0
    o_inc = int(h["plength"][:9].sum())
    assert h["names"][o_inc] == "Empty" and h["params"][o_inc] == 0 and h["relax"][o_inc] == 0
    # the height block by hand: l = 0 as in basic, then h_l[n] * amplitude_ratio(l, 45 deg)[l + m], l-major
    assert np.array_equal(h["params"][:nfl[0]], basic["params"][:nfl[0]])
    want, names, src = [], [], nfl[0]
    for l in (1, 2, 3):
        V = oracle.amplitude_ratio(l, 45.0)
        for n in range(nfl[l]):
            want += [basic["params"][src] * V[l + m] for m in range(l + 1)]
            names += ["H(%d,%d,%d)" % (n, l, m) for m in range(l + 1)]
            src += 1
    assert np.array_equal(h["params"][nfl[0]:nh], want) and h["names"][nfl[0]:nh] == names
    assert (h["relax"][nfl[0]:nh] == 1).all() and set(h["prior_names"][nfl[0]:nh]) == {"Jeffreys"}
    # the height keyword's numbers are taken from the FIRST one on this path (io_local.cpp:809, :1028): "1.0 1 10000" -> (1, 1, 1e4)
    assert np.array_equal(h["priors"][:, nfl[0]:nh], np.tile([[1.0], [1.0], [10000.0], [-9999.0]], nh - nfl[0]))
    st, m, _, _ = pkg.build_mode_table(14, h["params"], h["plength"], 94.3 + 0.01 * np.arange(800))
    assert st == 0 and len(m) == ntot


def _classic_dialect(lines, model):
    """The Sun sample (an a_j file) in the Classic dialect: model name replaced, the a-coefficient keyword lines replaced by the
    Splitting_a1 / Asphericity_eta / Splitting_a3 lines the Classic path reads (Inclination, Asymetry, Visibility_l* are there)."""
    out, done = [], False
    for ln in lines:
        w = ln.split()
        if w and w[0] == "model_fullname":
            out.append("model_fullname   %s" % model)
        elif w and w[0] in ("a1_0", "a1_1", "a2_0", "a2_1", "a3_0", "a3_1", "a4_0", "a4_1", "a5_0", "a5_1", "a6_0", "a6_1"):
            if not done:
                out += ["Splitting_a1   Uniform   0.45   0.0   2.0", "Asphericity_eta   Fix   0.0", "Splitting_a3   Fix   0.0"]
                done = True
        else:
            out.append(ln)
    assert done
    return out


def test_global_v2_loader(pkg, oracle, tmp_path):
    from tamcmc_c_amd import inputs, sampler
    src = "Sun_19992002_incfix_fast_Priorevalrange.model"
    pc = _variant(tmp_path, src, "classic.model", lambda L: _classic_dialect(L, "model_MS_Global_a1etaa3_HarveyLike_Classic"))
    p2 = _variant(tmp_path, src, "v2.model", lambda L: _classic_dialect(L, "model_MS_Global_a1etaa3_HarveyLike_Classic_v2"))
    p3 = _variant(tmp_path, src, "v3.model", lambda L: _classic_dialect(L, "model_MS_Global_a1etaa3_HarveyLike_Classic_v3"))
    ci = inputs.GlobalInputs(pc, 0.01)
    assert ci.model_id == 3 and ci.prior_class == 2 and ci.plength[6] == 6 and ci.plength[9] == 1
    c = _fields(ci)
    o = int(c["plength"][:9].sum())
    o_split = int(c["plength"][:6].sum())
    assert c["names"][o_split] == "Splitting_a1" and c["params"][o_split] == 0.45 and tuple(c["priors"][:2, o_split]) == (0.0, 2.0)
    assert c["names"][o] == "Inclination" and c["extra"][8] == 0 and c["extra"][9] == -1
    vi = inputs.GlobalInputs(p2, 0.01)
    assert vi.model_id == pkg.MODEL_MS_GLOBAL_A1ETAA3_CLASSIC_V2 == 12 and vi.prior_class == 2
    v = _fields(vi)
    assert v["plength"][9] == 9 and np.array_equal(np.delete(v["plength"], 9), np.delete(c["plength"], 9))
    assert v["extra"][8] == 1 and np.array_equal(np.delete(v["extra"], 8), np.delete(c["extra"], 8))
    for key in ("params", "relax", "sw"):
        assert np.array_equal(v[key][:o], c[key][:o]) and np.array_equal(v[key][o + 9:], c[key][o + 1:]), key
    assert np.array_equal(v["priors"][:, :o], c["priors"][:, :o]) and np.array_equal(v["priors"][:, o + 9:], c["priors"][:, o + 1:])
    assert v["names"][:o] == c["names"][:o] and v["names"][o + 9:] == c["names"][o + 1:]
    lmax, inc0 = int(c["plength"][1]), c["params"][o]
    k = 0
    for l in (1, 2, 3):
        V = oracle.amplitude_ratio(l, inc0)
        for m in range(l + 1):
            if l <= lmax:
                assert v["names"][o + k] == "Inc:H%d,%d" % (l, m) and v["prior_names"][o + k] == "Uniform" and v["relax"][o + k] == 1
                assert v["params"][o + k] == V[l + m] and tuple(v["priors"][:, o + k]) == (0.0, 1.0, -9999.0, -9999.0)
            else:
                assert v["names"][o + k] == "Empty" and v["params"][o + k] == 0 and v["relax"][o + k] == 0
            k += 1
    # the start vector is inside the prior of the three sums, and the model rows are those of the Classic file
    lp, st = sampler.log_prior(inputs.star_from_inputs(vi, np.linspace(1500.0, 4500.0, 3000)))
    assert st == 0 and np.isfinite(lp)
    x = 1500.0 + 0.1 * np.arange(30000)
    a, b = pkg.build_mode_table(3, c["params"], c["plength"], x), pkg.build_mode_table(12, v["params"], v["plength"], x)
    assert a[0] == b[0] == 0 and a[1].tobytes() == b[1].tobytes()
    with pytest.raises(pkg.TamcmcError) as e:
        inputs.GlobalInputs(p3, 0.01)
    assert "no prior the reference can run" in str(e.value)

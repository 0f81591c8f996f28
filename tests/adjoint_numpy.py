"""numpy yardstick of the adjoint gradient (test helper; uses no device code).

Tables come from the host builder (`pkg.build_mode_table`, bit-identical to the oracle's); the model row of a table is
`strict_numpy.eval_table`'s.  With S = sum_i (y_i / M_i + ln M_i) (the un-tempered logL is -S):

  frozen_central   the reference: central difference of S at theta +- h e_k where the perturbed tables keep the BASE table's windows
                   [i0, i1) ("frozen window"), summed in long double; its own uncertainty is R = max_k |g(h) - g(h/2)|;
  table_adjoint    G[row][f] = sum_i r_i dM_i/df on the row's window and Gn[j] = sum_i r_i dN_i/d|noise_j|, r_i = (1/M_i)(1 - y_i/M_i), with the
                   absolute sums sum_i |r_i dM_i/df| beside them (the scale of the device tolerance); f = nu[7], hv[7], gamma, asym, fc;
  adjoint_gradient table_adjoint contracted with the forward difference of the tables (the table Jacobian).
"""
import numpy as np

import strict_numpy

NF = 17
LD = np.longdouble


def tables(pkg, model_id, params, plength, x):
    st, mults, noise, nh = pkg.build_mode_table(model_id, params, plength, x)
    assert st == 0, st
    return mults, noise, nh


def _S(mults, noise, nh, x, y):
    M = strict_numpy.eval_table(mults, noise, nh, x)
    return np.sum((y / M).astype(LD)) + np.sum(np.log(M).astype(LD))


def steps(params, idx, rel=1e-6, floor=1e-2):
    return rel * np.maximum(np.abs(np.asarray(params)[idx]), floor)


def frozen_central(pkg, model_id, params, plength, idx, h, x, y):
    """d(-S)/dtheta_k by central differences, the windows of both perturbed tables frozen at the base table's."""
    base, _, _ = tables(pkg, model_id, params, plength, x)
    g = np.zeros(len(idx))
    for k, ip in enumerate(idx):
        S = []
        for sgn in (1.0, -1.0):
            P = np.array(params, dtype=np.float64)
            P[ip] = P[ip] + sgn * h[k]
            m, nz, nh = tables(pkg, model_id, P, plength, x)
            assert m.size == base.size
            m["i0"], m["i1"] = base["i0"], base["i1"]
            S.append(_S(m, nz, nh, x, y))
        g[k] = float(-(S[0] - S[1]) / (2 * LD(h[k])))
    return g


def reference(pkg, model_id, params, plength, idx, x, y):
    """(g, R): the frozen central difference at h = 1e-6 max(|theta|, 1e-2) and its own uncertainty max_k |g(h) - g(h/2)|."""
    h = steps(params, idx)
    g = frozen_central(pkg, model_id, params, plength, idx, h, x, y)
    g2 = frozen_central(pkg, model_id, params, plength, idx, 0.5 * h, x, y)
    return g, float(np.max(np.abs(g - g2)))


def table_adjoint(mults, noise, nh, x, y):
    """(G [rows x 17], Gabs [rows x 17], Gn [nnoise], Gnabs [nnoise]) of one table."""
    M = strict_numpy.eval_table(mults, noise, nh, x)
    r = (1.0 / M) * (1.0 - y / M)
    G, Ga = np.zeros((mults.size, NF)), np.zeros((mults.size, NF))

    def put(j, f, term):
        G[j, f] = float(np.sum(term.astype(LD)))
        Ga[j, f] = float(np.sum(np.abs(term).astype(LD)))

    for j, row in enumerate(mults):
        l, i0, i1 = int(row["l"]), int(row["i0"]), int(row["i1"])
        xl, rl = x[i0:i1], r[i0:i1]
        gam, al, fc = float(row["gamma"]), float(row["asym"]), float(row["fc"])
        if al != 0.0:
            u = xl / fc - 1.0
            a1 = 1.0 + al * u
            A = a1 * a1 + (0.5 * gam * al / fc) ** 2
        else:
            u, a1, A = np.zeros(xl.size), np.ones(xl.size), np.ones(xl.size)
        dG, s1 = np.zeros(xl.size), np.zeros(xl.size)
        for m in range(2 * l + 1):
            t = 2.0 * (xl - row["nu"][m]) / gam
            q = 1.0 + t * t
            hv = float(row["hv"][m])
            put(j, 7 + m, rl * A / q)
            put(j, m, rl * hv * A * (2.0 * t / (q * q)) * (2.0 / gam))
            dG = dG + hv * (A * 2.0 * t * t / (gam * q * q) + (0.5 * gam * al * al / (fc * fc)) / q)
            s1 = s1 + hv / q
        put(j, 14, rl * dG)
        if al != 0.0:
            put(j, 15, rl * s1 * (2.0 * a1 * u + 2.0 * (0.5 * gam / fc) ** 2 * al))
            put(j, 16, rl * s1 * (-2.0 * a1 * al * xl / (fc * fc) - 0.5 * gam * gam * al * al / fc ** 3))
    Gn, Gna = np.zeros(noise.size), np.zeros(noise.size)
    for k in range(nh):
        H, tau, p = noise[3 * k], noise[3 * k + 1], noise[3 * k + 2]
        if tau == 0:
            continue
        la = np.log(1e-3 * tau * x)
        z = np.exp(p * la)
        for f, term in ((0, r / (1 + z)), (1, -r * H * p * z / (tau * (1 + z) ** 2)), (2, -r * H * z * la / (1 + z) ** 2)):
            Gn[3 * k + f] = float(np.sum(term.astype(LD)))
            Gna[3 * k + f] = float(np.sum(np.abs(term).astype(LD)))
    Gn[-1] = float(np.sum(r.astype(LD)))
    Gna[-1] = float(np.sum(np.abs(r).astype(LD)))
    return G, Ga, Gn, Gna


def contract(G, Gn, base, noise0, m, noise):
    """dS to first order from the base table to table m (fields in declaration order, windows of m not read)."""
    dS = LD(0)
    for j in range(base.size):
        nc = 2 * int(base["l"][j]) + 1
        dS += np.sum((G[j, :nc] * (m["nu"][j, :nc] - base["nu"][j, :nc])).astype(LD))
        dS += np.sum((G[j, 7:7 + nc] * (m["hv"][j, :nc] - base["hv"][j, :nc])).astype(LD))
        dS += G[j, 14] * (m["gamma"][j] - base["gamma"][j])
        if base["asym"][j] != 0.0:
            dS += G[j, 15] * (m["asym"][j] - base["asym"][j]) + G[j, 16] * (m["fc"][j] - base["fc"][j])
    dS += np.sum((Gn * (noise - noise0)).astype(LD))
    return dS


def adjoint_gradient(pkg, model_id, params, plength, idx, hjac, x, y):
    """d(-S)/dtheta_k = -(G, Gn) . (table(theta + hjac e_k) - table(theta)) / hjac_applied."""
    base, nz0, nh = tables(pkg, model_id, params, plength, x)
    G, _, Gn, _ = table_adjoint(base, nz0, nh, x, y)
    g = np.zeros(len(idx))
    for k, ip in enumerate(idx):
        P = np.array(params, dtype=np.float64)
        P[ip] = P[ip] + hjac[k]
        m, nz, _ = tables(pkg, model_id, P, plength, x)
        assert m.size == base.size
        g[k] = float(-contract(G, Gn, base, nz0, m, nz) / LD(P[ip] - params[ip]))
    return g


def stars(synth):
    """The three stars of the gradient checks: name -> star (C2 local slice; C3 global fit with asymmetry; Classic)."""
    c2 = synth.make_c2_star(nx=4000)
    c3 = synth.make_c3_star(nx=20000, step=0.1, nmax=8)
    o = c3.plength[0] + c3.plength[1] + c3.plength[2:6].sum()
    c3.params[o + 13] = 15.0   # asymmetry on
    cl = synth.make_classic_star(nx=20000, nmax=6, step=0.05)
    return {"c2": c2, "c3_asym": c3, "classic": cl}


def corner_star(synth):
    """One small table with every corner of the row and noise kernels: windows of 50 .. 548 bins (shorter and longer than a workgroup of
    256), eleven rows clamped at the spectrum's lower edge (i0 = 0), four l = 3 rows (seven components), asymmetry on, the second Harvey
    term with tau = 0 (skipped, as in the model), 4000 bins (no multiple of any tile)."""
    s = synth.make_c3_star(nx=4000, step=1.0, nmax=4, fmin=2300.0)
    o = s.plength[0] + s.plength[1] + s.plength[2:6].sum()
    s.params[o + 13] = 15.0
    s.params[o + 14 + 4 + 4] = 0.0   # Harvey-Noise_tc of the second term
    return s


_CACHE = {}


def cached_reference(pkg, oracle, synth, name):
    """(star, y, g_ref, R) of stars()[name], computed once per process: the frozen central difference at the star's own parameters."""
    if name not in _CACHE:
        star = stars(synth)[name]
        y = spectrum(oracle, star)
        g, R = reference(pkg, star.model_id, star.params, star.plength, star.index_to_relax, star.x, y)
        _CACHE[name] = (star, y, g, R)
    return _CACHE[name]


def spectrum(oracle, star, seed=1):
    _, m0 = oracle.call_model(star.model_id, star.params, star.plength, star.x)
    return star.set_spectrum_from_model(m0, seed)

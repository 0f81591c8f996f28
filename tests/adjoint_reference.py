"""The table-space adjoint's definition at 50 digits, and the exact replay of its contraction (test helper; no device code).

Apart from csrc/adjoint.hip and from adjoint_numpy.table_adjoint, which share one hand derivation of dM/dgamma, dM/dasym and dM/dfc:
nothing here is differentiated on paper.  With M the 50-digit model row of the whole table (tile_reference.model_row_exact) and
r_i = (1/M_i)(1 - y_i/M_i),

    table_adjoint_exact   G[row][f] = sum_{i in [max(i0,0), min(i1,Nx))} r_i dM_i/df and Gn[j] = sum_i r_i dN_i/d|noise_j|, the derivatives
                          by CENTRAL DIFFERENCES IN FIELD SPACE: the one field of the one row (or noise entry) moved by +-h, only what
                          depends on it re-evaluated from the model's definition, every window frozen.  f = nu[7], hv[7], gamma, asym, fc.
                          Step h = REL |field| (REL = 1e-25; a field that is 0: REL) at WORK = 100 digits: the difference's O(h^2) term is
                          (h / gamma)^2 ~ 1e-43 of the derivative and its cancellation leaves 1e-75, so the sums hold to far more than
                          25 digits (test_adjoint_exact.py halves the step).  The rules of include/tamcmc_hip.h: components m < 2l+1 only,
                          the asym and fc entries 0 where the row's asym == 0, a Harvey term with tau == 0 skipped (its three entries 0),
                          the last noise entry sum_i r_i.
    contract_exact        sum G . (T_e - T_0) over the doubles as the exact rationals they are, in k_adj_contract's field rules, with
                          sum |G . (T_e - T_0)| beside it.
    dS_from_gradient      the exact inverse of fd_batch.hip's assemble_gradient for the likelihood's share.
"""
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

import tile_reference as tr

NF = 17
WORK = 100                 # digits of the differences
REL = Decimal("1e-25")     # relative field step
MILLI = tr.MILLI


def _D(v):
    return Decimal(float(v))


def _step(v, rel):
    return abs(v) * rel if v != 0 else rel


def _lorentz(x, nu, hv, g2):
    d = x - nu
    return hv / (1 + 4 * d * d / g2)


def _asy(x, g, a, fc):
    return (1 + a * (x / fc - 1)) ** 2 + (g * a / (2 * fc)) ** 2


def _row_value(x, nus, hvs, g, a, fc, asy):
    """One row at one bin from the definition (tile_reference's header): Decimal."""
    g2 = g * g
    s = Decimal(0)
    for nu, hv in zip(nus, hvs):
        s += _lorentz(x, nu, hv, g2)
    return s * _asy(x, g, a, fc) if asy else s


def _harvey(L, H, p):
    """H / (1 + (1e-3 tau x)^p) with L = ln(1e-3 tau x) (Decimal)."""
    return H / (1 + (p * L).exp())


def table_adjoint_exact(tab, noise, nh, x, y, rel=REL):
    """(G [rows x 17], Gabs [rows x 17], Gn [nn], Gnabs [nn]) of one table, lists of Decimal (nn = len(noise))."""
    nn = len(noise)
    M = tr.model_row_exact(tab, noise, nh, nn, x)
    G = [[Decimal(0)] * NF for _ in range(len(tab))]
    Ga = [[Decimal(0)] * NF for _ in range(len(tab))]
    Gn, Gna = [Decimal(0)] * nn, [Decimal(0)] * nn
    with localcontext() as ctx:
        ctx.prec = WORK
        r = [(1 - _D(y[i]) / M[i]) / M[i] for i in range(len(x))]
        xs = [_D(v) for v in x]
        for j, row in enumerate(tab):
            nc = 2 * int(row["l"]) + 1
            lo, hi = max(int(row["i0"]), 0), min(int(row["i1"]), len(x))
            nus, hvs = [_D(v) for v in row["nu"][:nc]], [_D(v) for v in row["hv"][:nc]]
            g, a, fc = _D(row["gamma"]), _D(row["asym"]), _D(row["fc"])
            asy = float(row["asym"]) != 0.0
            hnu = [_step(v, rel) for v in nus]
            hhv = [_step(v, rel) for v in hvs]
            hg, ha, hfc = _step(g, rel), _step(a, rel), _step(fc, rel)
            acc, aabs = G[j], Ga[j]
            for i in range(lo, hi):
                xi, ri = xs[i], r[i]
                fac = _asy(xi, g, a, fc) if asy else 1
                d = [None] * NF
                g2 = g * g
                for m in range(nc):
                    d[m] = fac * (_lorentz(xi, nus[m] + hnu[m], hvs[m], g2) - _lorentz(xi, nus[m] - hnu[m], hvs[m], g2)) / (2 * hnu[m])
                    d[7 + m] = fac * (_lorentz(xi, nus[m], hvs[m] + hhv[m], g2) - _lorentz(xi, nus[m], hvs[m] - hhv[m], g2)) / (2 * hhv[m])
                d[14] = (_row_value(xi, nus, hvs, g + hg, a, fc, asy) - _row_value(xi, nus, hvs, g - hg, a, fc, asy)) / (2 * hg)
                if asy:
                    d[15] = (_row_value(xi, nus, hvs, g, a + ha, fc, True) - _row_value(xi, nus, hvs, g, a - ha, fc, True)) / (2 * ha)
                    d[16] = (_row_value(xi, nus, hvs, g, a, fc + hfc, True) - _row_value(xi, nus, hvs, g, a, fc - hfc, True)) / (2 * hfc)
                for f in range(NF):
                    if d[f] is not None:
                        t = ri * d[f]
                        acc[f] += t
                        aabs[f] += abs(t)
        for k in range(int(nh)):
            H, tau, p = _D(noise[3 * k]), _D(noise[3 * k + 1]), _D(noise[3 * k + 2])
            if float(noise[3 * k + 1]) == 0.0:
                continue
            hH, ht, hp = _step(H, rel), _step(tau, rel), _step(p, rel)
            # ln(1e-3 (tau +- ht) x) = ln(1e-3 tau x) + ln(1 +- ht / tau): one logarithm per bin, two for the step
            up, dn = (1 + ht / tau).ln(), (1 - ht / tau).ln()
            for i in range(len(x)):
                L = (_D(MILLI) * tau * xs[i]).ln()
                ds = ((_harvey(L, H + hH, p) - _harvey(L, H - hH, p)) / (2 * hH),
                      (_harvey(L + up, H, p) - _harvey(L + dn, H, p)) / (2 * ht),
                      (_harvey(L, H, p + hp) - _harvey(L, H, p - hp)) / (2 * hp))
                for f in range(3):
                    t = r[i] * ds[f]
                    Gn[3 * k + f] += t
                    Gna[3 * k + f] += abs(t)
        for ri in r:
            Gn[nn - 1] += ri
            Gna[nn - 1] += abs(ri)
    return G, Ga, Gn, Gna


_CACHE = {}


def cached_table_adjoint(tab, noise, nh, x, y):
    """table_adjoint_exact as float64 arrays (each entry rounded once), computed once per process and table: tables that are the same
    bytes (a device builder that does not depend on the arithmetic mode or the geometry) share one reference."""
    key = (np.ascontiguousarray(tab).tobytes(), np.ascontiguousarray(noise, dtype=np.float64).tobytes(), int(nh),
           np.ascontiguousarray(x).tobytes(), np.ascontiguousarray(y).tobytes())
    if key not in _CACHE:
        _CACHE[key] = tuple(as_float(v) for v in table_adjoint_exact(tab, noise, nh, x, y))
    return _CACHE[key]


def as_float(G):
    """A (nested) list of Decimals as a float64 array (each entry rounded once)."""
    return np.array([[float(v) for v in row] for row in G]) if G and isinstance(G[0], list) else np.array([float(v) for v in G])


# ---------------------------------------------------------------- the contraction, exactly ----------------------------------------------------------------
def _F(v):
    return Fraction(float(v))


def contract_exact(G, Gn, base, noise0, tab, noise, nn, fields=None):
    """(dS, abs_sum): sum G . (T_e - T_0) and sum |G . (T_e - T_0)| as Fractions, every double taken exactly, in k_adj_contract's
    rules -- 2l+1 from the BASE row, asym / fc only where the base row's asym != 0, the first nn (the base's) noise entries, the windows of
    `tab` never read.  fields: a set that receives the field indices (0..16 of a row, 17 for the noise row) with a non-zero term."""
    dS, ab = Fraction(0), Fraction(0)
    fields = set() if fields is None else fields

    def add(gv, e, b, f):
        nonlocal dS, ab
        if e != b and gv != 0.0:
            t = _F(gv) * (_F(e) - _F(b))
            dS += t
            ab += abs(t)
            fields.add(f)

    G = np.asarray(G, dtype=np.float64)
    n = len(base)
    assert len(tab) >= n
    # rows that differ at all (a perturbation moves few rows; the exact arithmetic goes where a term can be non-zero)
    moved = [j for j in range(n) if tab[j].tobytes() != base[j].tobytes()]
    for j in moved:
        b, e = base[j], tab[j]
        nc = 2 * min(max(int(b["l"]), 0), 3) + 1
        for m in range(nc):
            add(G[j, m], e["nu"][m], b["nu"][m], m)
        for m in range(nc):
            add(G[j, 7 + m], e["hv"][m], b["hv"][m], 7 + m)
        add(G[j, 14], e["gamma"], b["gamma"], 14)
        if float(b["asym"]) != 0.0:
            add(G[j, 15], e["asym"], b["asym"], 15)
            add(G[j, 16], e["fc"], b["fc"], 16)
    for j in range(int(nn)):
        add(Gn[j], noise[j], noise0[j], 17)
    return dS, ab


def dS_from_gradient(g, x0, h, T, p):
    """The dS that assemble_gradient turned into the likelihood's share g of one component: g = fl(fl(-(long)p dS / T) / happ) with
    happ = fl(x0 + h) - x0, so dS = -g happ T / (long)p, here without rounding (Fraction)."""
    happ = _F((np.float64(x0) + np.float64(h)) - np.float64(x0))   # (the double the host forms)
    return -_F(g) * happ * _F(T) / int(p)

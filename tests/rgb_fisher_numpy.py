"""numpy yardstick of the expected (Fisher) information of the red-giant models, ids 25 / 27 (test helper; no device likelihood).

The host cannot build a red-giant table, so the tables are the ones the device builder exports (HipContext.rgb_batch_tables with
idx = [index_to_relax, index_to_relax], h = [+h, -h]: slot 1 + k is theta + h_k e_k, slot 1 + N + k is theta - h_k e_k -- the slots of
tamcmc_hip_fisher), as in tests/test_gpu_rgb_adjoint.py.  The class rule of csrc/adj_rgb_match.h and the form rule of csrc/fisher_rgb_rule.h
are restated here; model rows by strict_numpy.eval_table, the sums of F in long double (as tests/fisher_numpy.py)."""
import numpy as np

import strict_numpy

LD = np.longdouble
CENTRAL, ONE_SIDED_PLUS, ONE_SIDED_MINUS, UNFROZEN = "central", "one-sided +", "one-sided -", "unfrozen"


def linearisable(base, pert):
    """adj_rgb_class of two valid tables: same row count, same l row by row, every l=1 row strictly within half the distance from the base
    row's fc to its nearest l=1 neighbour among the rows next to it."""
    if base.size != pert.size:
        return False
    if not np.array_equal(base["l"], pert["l"]):
        return False
    n = base.size
    for j in range(n):
        if base["l"][j] != 1:
            continue
        gap = np.inf
        if j > 0 and base["l"][j - 1] == 1:
            gap = abs(base["fc"][j] - base["fc"][j - 1])
        if j + 1 < n and base["l"][j + 1] == 1:
            gap = min(gap, abs(base["fc"][j + 1] - base["fc"][j]))
        if not abs(pert["fc"][j] - base["fc"][j]) < 0.5 * gap:
            return False
    return True


def modes_linearisable(f0, f1):
    """The same rule on two lists of mixed-mode frequencies alone (the oracle's): what decides the class when no other row changes degree."""
    if f0.size != f1.size:
        return False
    gap = np.minimum(np.diff(f0, prepend=-np.inf), np.diff(f0, append=np.inf))
    return bool(np.all(np.abs(f1 - f0) < 0.5 * np.abs(gap)))


def form_of(base, plus, minus):
    lp, lm = linearisable(base, plus), linearisable(base, minus)
    return CENTRAL if lp and lm else ONE_SIDED_PLUS if lp else ONE_SIDED_MINUS if lm else UNFROZEN


def export(ctx, star, params, idx, h):
    """The 2 N + 1 tables of one chain as tamcmc_hip_fisher builds them: (tables, noise rows, Harvey counts)."""
    idx = np.asarray(idx, dtype=np.int32)
    tabs, noise, nh, status = ctx.rgb_batch_tables(star.model_id, params, star.plength, np.concatenate([idx, idx]), np.concatenate([h, -h]))
    assert (status == 0).all()
    return tabs, noise, nh


def _row(tab, noise, nh, x, windows=None):
    m = tab.copy()
    if windows is not None:
        assert m.size == windows.size
        m["i0"], m["i1"] = windows["i0"], windows["i1"]
    return strict_numpy.eval_table(m, noise, int(nh), x)


def fisher_rgb(star, params, idx, h, exported, force=None):
    """(F [N x N], U [N x Nx], h_applied [N], forms [N]) at `params` from the exported tables.  force: {k: form} overrides the rule for
    variable k (the measurement of one form against another at a point where both exist)."""
    tabs, noise, nh = exported
    idx = np.asarray(idx)
    N = idx.size
    x = star.x
    base = tabs[0]
    M0 = _row(base, noise[0], nh[0], x)
    U, happ, forms = np.zeros((N, x.size)), np.zeros(N), []
    for k in range(N):
        sp, sm = 1 + k, 1 + N + k
        x0 = float(params[idx[k]])
        xp, xm = np.float64(x0) + np.float64(h[k]), np.float64(x0) + np.float64(-h[k])
        form = (force or {}).get(k) or form_of(base, tabs[sp], tabs[sm])
        forms.append(form)
        if form == CENTRAL:
            Mp, Mm, happ[k] = _row(tabs[sp], noise[sp], nh[sp], x, base), _row(tabs[sm], noise[sm], nh[sm], x, base), xp - xm
        elif form == ONE_SIDED_PLUS:        # the - slot holds the base table: its row is M0
            Mp, Mm, happ[k] = _row(tabs[sp], noise[sp], nh[sp], x, base), M0, xp - x0
        elif form == ONE_SIDED_MINUS:
            Mp, Mm, happ[k] = M0, _row(tabs[sm], noise[sm], nh[sm], x, base), x0 - xm
        else:                               # each table on its own windows
            Mp, Mm, happ[k] = _row(tabs[sp], noise[sp], nh[sp], x), _row(tabs[sm], noise[sm], nh[sm], x), xp - xm
        U[k] = (Mp - Mm) / (happ[k] * M0)
    UL = U.astype(LD)
    F = np.array([[float(np.sum(UL[j] * UL[k])) for k in range(N)] for j in range(N)])
    return F, U, happ, forms

"""The windowed finite-difference route's result per slot, exactly: dS = S(table_k) - S(table_0), without the cancellation of two sums.

Apart from the kernels (csrc/fd_batch.hip k_fd_compare, csrc/kernels.hip k_fd_moments / k_fd_far, csrc/loglike_tile.h k_loglike<DELTA>),
from the brute-force batch and from the oracle: it shares no line with any of them.  It takes two tables as the batch built them
(Table: rows MULT_DTYPE, noise, nh, nn), x and y, and every double among them as the exact rational it is.  The tables themselves have
tests/table_reference.py; everything after them is pinned here.

    delta_exact        `decimal` at PREC = 50 digits, the plain formula: f_i = y_i/M1_i - y_i/M0_i + ln(M1_i/M0_i), dS = sum_i f_i
    slot_reference     the vectorised numpy.longdouble twin, formed WITHOUT cancellation:
                           dM_i  summed term by term over the rows and noise terms that differ, per component new - old (rows and
                                 noise entries equal in both tables are never summed)
                           u_i   = dM_i / M0_i
                           f_i   = -(y_i/M0_i) u_i/(1+u_i) + log1p(u_i)
                       (test_delta_reference.py pins it to the definition within 1/10 of the smallest budget it serves)
    device_dS          what the device's dS was: logL1 - logL0 = -(long)p dS / T and the gradient entry is that over
                       h_applied = (theta + h) - theta in doubles (assemble_gradient), so dS_dev = g h_applied T / (-p), three roundings.

The route's CLASSIFICATION restated in plain Python (classify, tile_paths), so that a test can say which path a (slot, tile) must take:
    change kind per row   0 unchanged (all 152 bytes equal), 1 heights only (degree, window, centre, width, asymmetry and the seven
                          frequencies equal), 2 pair, 3 / 4 present in the perturbed / the base table only
    full table            FAST arithmetic, no noise change and sum(2 per pair, 1 otherwise) > n_new: the whole perturbed table minus the
                          M0 plane (FAST_DIRECT keeps the pairs: slot_of)
    affected range        [min i0, max i1) over the windows of the changed rows (old and new), every bin when the noise changed or the
                          table is full
    light (k_fd_far)      1 .. 16 delta rows and flags = 0
    far (row, tile)       tile_reference.row_is_far
    moment tile           FAST with 64-lane workgroups, not a full table, every delta row that overlaps the tile covers it and is far,
                          a changed noise row only where the background series holds (tile_reference.series_gate at the steeper of
                          the two rows' exponents), and the gate sum_k |c_k| max(1/M0) <= 1e-5 on the SUMMED coefficients c_k of the
                          restated far_seed / far_coefs (tile_series.py).  A moment tile of a light slot is k_fd_far's (no bin of it is
                          walked and the launch's statistics say so); any other is the tile kernel's delta_moment_shortcut.

THE BUDGET (slot_budget): |dS_dev - dS_exact| <= truncation + far + rounding + planes, per slot, none of it fitted to the device.
With the twin's u_i, yr_i = y_i/M0_i, w_i = |1 - yr_i|/M0_i (the first-order weight of an error of dM at bin i):
  truncation   first omitted term.  Series bin (|u| <= 0.01): (|yr| + 1/6) |u|^6 / (1 - |u|); bin of a moment tile (u^3 omitted):
               (|yr| + 1/3) |u|^3 / (1 - |u|); closed-form bin: 0.
  far          for each far (delta row, tile) pair and component: tile_series.tau(rho, n) at the pair's OWN rho and the n the code keeps
               there (16 in k_fd_far, which runs far_coefs<false>; at least n_terms(rho^2) in the tile kernel: the wave's longest loop
               runs, so the component's own n bounds its tail from above), TAU_ASYM for a row with asymmetry; times |component| at the
               bin, times w_i; +new and -old counted separately.  FAST_DIRECT has no far field: 0.  A changed noise row on a tile whose
               background series holds (FAST): HARVEY_BUDGET (tile_series.py) times (|new term| + |old term|), times w_i.
  rounding     K_ROUND 2^-53 sum_i w_i A_i, A_i = what the device adds into dM at the bin, in absolute values: |new| + |old| per pair
               component, |dhv| x profile for a heights-only row, + M0_i for a full table, both rows' terms for a changed noise row;
               sum_k (|c_k new| + |c_k old|) on a moment tile.  Terms whose ARGUMENT is formed by a cancellation are weighted by what that
               does to them, as the issue weights a Harvey term:
                   Harvey term        1 + |p ln(1e-3 tau x)|: the exponent p (ln(1e-3 tau) + ln x) is rounded at its own size
                   Lorentzian         1 + (|A_m| + beta) 2|t| / (1 + t^2): t = (x - x_c) 2/gamma - A_m (fast_mult, loglike_tile.h:194) is
                                      rounded at the size |A_m| + beta of its two parts, and d ln(1/(1 + t^2)) = -2t/(1 + t^2) dt
                   asymmetry factor   + 2 |asym| (|x|/fc + 1) |ta| / (ta^2 + c2^2): ta = asym/fc x + (1 - asym) (loglike_tile.h:206)
                                      is rounded at the size of ITS two parts
               K_ROUND: twice the longest count of roundings, in units of what the weights above are attached to:
                   near-field component (loglike_tile.h)   2/gamma by reciprocal and two Newton steps 2 (:249), A_m 2 (:250), x - x_c 1
                       (:193), t 1 (:194) -- these six at the weighted size --, q 1 (:195), the common-denominator chain of an l = 3 row 6
                       steps of N <- N q + hv D (2 each) and D <- D q (1 each) = 18 (:198-203), reciprocal with one Newton step 2 and
                       its product 1 (:204), asymmetry: asym/fc 3 (:259-262), ta 1, factor 1, product 1 (:206-207), the row into
                       the bin's sum, one per staged row <= 64 (:209, CHUNK), u = dM r0 1 (:487), five fma of the series and the
                       product 6 (:490-494), the lane's K <= 8 bins 8 (:496), the workgroup's tree 8 (block_reduce), the fold of
                       the tiles by k_finalize <= 17 tiles here: 8 (tree)                                                    = 130
                   far coefficient, walked (far_seed / far_coefs / horner)   A_m 4, inv = reciprocal of A^2 + 1: 2 x 4 + 1 + 2 = 11,
                       c_0 12, two_req = 2 beta A inv: beta 3 + A 4 + inv 11 + 2 = 20 (:272-275); c_k = two_req c_(k-1) - q2 c_(k-2)
                       carries 12 + 22 k, and with |c_k| <= (k + 1) rho^k c_0, rho <= 1/6, the |c_k|-weighted mean of k is
                       2 rho / (1 - rho) = 0.4: 21 on sum_k |c_k| (:278-292); the lanes' vectors into the tile's 16 + WGS/16 <= 32
                       (:755-769); s = (x - x_c)/h 2, Horner 16 (:538-541); then as above from "the row into the bin's sum"
                       on (64 + 1 + 6 + 8 + 8 + 8)                                                                           = 166
                   moment form (k_fd_moments / k_fd_far, kernels.hip)   the coefficient 21 as above, the four waves' vectors 3 (:211-215),
                       a moment: weight (1 - yr) r0 2 (:112), s 2 and its power, weighted mean of k 0.4: 2 (:111, :119), eight
                       bins per lane 8 (:117) and the 64 lanes in order 63 (:133), the dot product's fma 16 + 31 (:226-233), the
                       fold of the tiles 8                                                                                  = 156
               K_ROUND = 2 x 166 = 332.
  planes       1/M0 and y/M0 are the FAST base launch's: 1e-12 sum_i |f_i|, the project's FAST row statement; and 3 x 2^-53 |dS| for the
               three roundings between the device's sum and the gradient entry it is read back from.
"""
from collections import namedtuple
from decimal import Decimal, localcontext

import numpy as np

import tile_reference as tr
import tile_series as ts

PREC = tr.PREC
LD = tr.LD
EPS = 2.0 ** -53
K_ROUND = 2 * 166          # derivation above
MOMENT_GATE = 1e-5         # moment_form_holds (loglike_tile.h)
U_SERIES = 0.01            # beyond it a bin takes the closed form
U_MARGIN = 1e-3            # relative margin the cases keep from it
FAR_ROWS = 16              # k_fd_far takes evaluations of 1 .. 16 delta rows
PLANES = 1e-12             # FAST row statement: |dM| <= 1e-12 M

Table = namedtuple("Table", "rows noise nh nn")
Config = namedtuple("Config", "name farfield wg tile_bins")   # farfield: FAST (False: FAST_DIRECT); tile_bins = wg x bins per thread


def config(name, wg, K):
    return Config("%s(%d,%d)" % (name, wg, K), name == "fast", wg, wg * K)


# ---------------------------------------------------------------- the definition, 50 digits ----------------------------------------------------------------
def delta_exact(t0, t1, x, y, bins):
    """{bin: f_i} (Decimal), f_i = y_i/M1_i - y_i/M0_i + ln(M1_i/M0_i): the plain formula, each table on its own windows."""
    m0 = tr.model_row_exact(t0.rows, t0.noise, t0.nh, t0.nn, x, bins)
    m1 = tr.model_row_exact(t1.rows, t1.noise, t1.nh, t1.nn, x, bins)
    out = {}
    with localcontext() as ctx:
        ctx.prec = PREC
        for i in m0:
            yi = Decimal(float(y[i]))
            out[i] = yi / m1[i] - yi / m0[i] + (m1[i] / m0[i]).ln()
    return out


# ---------------------------------------------------------------- classification (k_fd_compare) ----------------------------------------------------------------
def change_kind(ro, rn):
    if ro.tobytes() == rn.tobytes():
        return 0
    same = all(ro[k] == rn[k] for k in ("l", "i0", "i1", "fc", "gamma", "asym")) and bool(np.all(ro["nu"] == rn["nu"]))
    return 1 if same else 2


Slot = namedtuple("Slot", "kinds counts noise_changed full lo hi drows light pieces")


def classify(t0, t1, nx, full_tables=True):
    """The slot's delta entry.  drows: the delta table as the launch reads it, [(row, tag)] in table order, tag '+new' / '-old' / 'dh'
    (heights negated / differenced in doubles, as the kernel does) -- for a full table every row of the perturbed table.  pieces: the
    rows whose components make up dM (+new, -old, dh of the CHANGED rows, also for a full table)."""
    n0, n1 = len(t0.rows), len(t1.rows)
    kinds = []
    for j in range(max(n0, n1)):
        kinds.append(4 if j >= n1 else 3 if j >= n0 else change_kind(t0.rows[j], t1.rows[j]))
    if n0 == 0:   # (a base table that failed is empty: nothing is compared)
        kinds = [0] * len(kinds)
    noise_changed = n0 > 0 and any(float(t1.noise[i]) != float(t0.noise[i]) for i in range(int(t1.nn)))
    nrows = sum(2 if k == 2 else 1 for k in kinds if k)
    full = bool(full_tables and not noise_changed and nrows > n1)
    pieces, lo, hi = [], nx, 0
    for j, k in enumerate(kinds):
        if not k:
            continue
        if k != 4:
            lo, hi = min(lo, int(t1.rows[j]["i0"])), max(hi, int(t1.rows[j]["i1"]))
        if k != 3:
            lo, hi = min(lo, int(t0.rows[j]["i0"])), max(hi, int(t0.rows[j]["i1"]))
        if k in (2, 3):
            pieces.append((t1.rows[j].copy(), "+new"))
        if k == 1:
            r = t0.rows[j].copy()
            r["hv"] = t1.rows[j]["hv"] - t0.rows[j]["hv"]
            pieces.append((r, "dh"))
        if k in (2, 4):
            r = t0.rows[j].copy()
            r["hv"] = -t0.rows[j]["hv"]
            pieces.append((r, "-old"))
    drows = [(r.copy(), "+new") for r in t1.rows] if full else pieces
    if noise_changed or full:
        lo, hi = 0, nx
    elif not pieces:
        lo, hi = 0, 0
    counts = {"unchanged": kinds.count(0), "heights_only": kinds.count(1), "pair": kinds.count(2), "one_sided": kinds.count(3) + kinds.count(4)}
    light = 1 <= len(drows) <= FAR_ROWS and not noise_changed and not full
    return Slot(kinds, counts, noise_changed, full, lo, hi, drows, light, pieces)


# ---------------------------------------------------------------- the longdouble twin ----------------------------------------------------------------
def _hv_ld(row, hv):
    r = {k: row[k] for k in ("l", "gamma", "asym", "fc", "nu")}
    r["hv"] = hv
    return r


def _harvey_ld(H, tau, pw, xl):
    if float(tau) == 0.0:
        return np.zeros(xl.size, dtype=LD)
    return LD(H) / (LD(1) + np.power(LD(tr.MILLI) * LD(tau) * xl, LD(pw)))


def _arg_weight(row, xs, step):
    """[2l+1 x len(xs)] float64: 1 + the amplification of the roundings of a component's arguments (module docstring).  |A_m| + beta on
    the tile that holds the bin is at most |t| + 2 beta, and 2 beta = one tile's width x 2/gamma is taken at the widest tile (256 x 4):
    an upper bound for every geometry."""
    g, xs = float(row["gamma"]), np.asarray(xs, dtype=np.float64)
    out = np.ones((2 * int(row["l"]) + 1, xs.size))
    for k in range(out.shape[0]):
        t = 2.0 * (xs - float(row["nu"][k])) / g
        out[k] += (np.abs(t) + _BETA_BINS * abs(step) * 2.0 / g) * 2.0 * np.abs(t) / (1.0 + t * t)
    if float(row["asym"]) != 0.0:
        a, f = float(row["asym"]), float(row["fc"])
        ta = 1.0 + a * ((xs - f) / f)
        c2 = g * a / (2.0 * f)
        out += 2.0 * abs(a) * (np.abs(xs) / abs(f) + 1.0) * np.abs(ta) / (ta * ta + c2 * c2)
    return out


_BETA_BINS = 1024   # 2 beta = one tile's width x 2/gamma at the widest tile (256 x 4)

Reference = namedtuple("Reference", "slot slot_pairs dM u yr w f dS A M0 noise_terms")


def slot_of(ref, cfg):
    """The slot's delta entry under a configuration: full tables exist in FAST arithmetic only (the base launch's background series are
    at hand there, fd_batch.hip); FAST_DIRECT keeps the pairs and their range."""
    return ref.slot if cfg.farfield else ref.slot_pairs


def base_row(t0, x):
    return tr.model_row_ld(t0.rows, t0.noise, t0.nh, t0.nn, x)


def slot_reference(t0, t1, x, y, M0=None, full_tables=True):
    """The twin: everything of one slot that does not depend on the launch geometry."""
    x = np.asarray(x, dtype=np.float64)
    nx = x.size
    xl = x.astype(LD)
    step = float(x[1] - x[0])
    M0 = base_row(t0, x) if M0 is None else M0
    s = classify(t0, t1, nx, full_tables)
    dM = np.zeros(nx, dtype=LD)
    A = np.zeros(nx)
    for j, k in enumerate(s.kinds):
        if not k:
            continue
        ro = t0.rows[j] if k != 3 else None
        rn = t1.rows[j] if k != 4 else None
        if k == 1:
            sl = slice(int(ro["i0"]), int(ro["i1"]))
            c = tr._row_components_ld(_hv_ld(ro, rn["hv"].astype(LD) - ro["hv"].astype(LD)), xl[sl])
            dM[sl] += c.sum(axis=0)
            A[sl] += (np.abs(c).astype(np.float64) * _arg_weight(ro, x[sl], step)).sum(axis=0)
            continue
        a0, a1 = (int(rn["i0"]), int(rn["i1"])) if rn is not None else (0, 0)
        b0, b1 = (int(ro["i0"]), int(ro["i1"])) if ro is not None else (0, 0)
        c0, c1 = max(a0, b0), min(a1, b1)   # both rows: per component new - old; one row only: that row
        both = k == 2 and c1 > c0 and int(rn["l"]) == int(ro["l"])
        if both:
            sl = slice(c0, c1)
            dM[sl] += (tr._row_components_ld(rn, xl[sl]) - tr._row_components_ld(ro, xl[sl])).sum(axis=0)
        for r, w0, w1, sign in ((rn, a0, a1, 1), (ro, b0, b1, -1)):
            if r is None:
                continue
            sl = slice(w0, w1)
            c = tr._row_components_ld(r, xl[sl])
            A[sl] += (np.abs(c).astype(np.float64) * _arg_weight(r, x[sl], step)).sum(axis=0)
            if both:   # the parts of the window outside the common one
                for p0, p1 in ((w0, min(w1, c0)), (max(w0, c1), w1)):
                    if p1 > p0:
                        dM[p0:p1] += sign * c[:, p0 - w0:p1 - w0].sum(axis=0)
            else:
                dM[sl] += sign * c.sum(axis=0)
    noise_terms = []   # (|new term| + |old term|) float64 rows of the Harvey terms the device sums for a changed noise row
    if s.noise_changed:
        nh = int(t1.nh)
        lx = np.log(np.maximum(tr.MILLI * x, 1e-300))
        for k in range(nh):
            n1, n0 = t1.noise[3 * k:3 * k + 3], t0.noise[3 * k:3 * k + 3]
            vn, vo = _harvey_ld(n1[0], n1[1], n1[2], xl), _harvey_ld(n0[0], n0[1], n0[2], xl)
            if any(float(a) != float(b) for a, b in zip(n1, n0)):
                dM += vn - vo
            # (the device sums every term of both rows once the row changed: they all round)
            wn = 1.0 + np.abs(float(n1[2]) * (np.log(max(float(n1[1]), 1e-300)) + lx)) if float(n1[1]) != 0.0 else 1.0
            wo = 1.0 + np.abs(float(n0[2]) * (np.log(max(float(n0[1]), 1e-300)) + lx)) if float(n0[1]) != 0.0 else 1.0
            A += np.abs(vn).astype(np.float64) * wn + np.abs(vo).astype(np.float64) * wo
            noise_terms.append(np.abs(vn).astype(np.float64) + np.abs(vo).astype(np.float64))
        wh1, wh0 = t1.noise[int(t1.nn) - 1], t0.noise[int(t0.nn) - 1]
        if float(wh1) != float(wh0):
            dM += LD(wh1) - LD(wh0)
        A += abs(float(wh1)) + abs(float(wh0))
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    u = dM / M0
    yr = yl / M0
    f = -yr * u / (LD(1) + u) + np.log1p(u)
    w = (np.abs(LD(1) - yr) / M0).astype(np.float64)
    # (A without the + M0_i of a full table: slot_budget adds it where the configuration takes one)
    return Reference(s, classify(t0, t1, nx, False) if s.full else s, dM, u, yr.astype(np.float64), w, f, f.sum(), A, M0, noise_terms)


def device_dS(grad, theta, h, T, p=1.0):
    """dS the device summed, from its gradient entry: g = (-(long)p dS / T) / ((theta + h) - theta)."""
    happ = (np.float64(theta) + np.float64(h)) - np.float64(theta)
    return float(LD(grad) * LD(happ) * LD(T) / LD(-int(p)))


# ---------------------------------------------------------------- paths per tile, and the budget ----------------------------------------------------------------
def _piece_coefs(r, xc, h):
    """(summed coefficients [16], sum_k |c_k| over the components) of one far row on one tile: far_seed / far_coefs restated."""
    ig = 2.0 / float(r["gamma"])
    beta = ig * h
    tot, ab = [0.0] * ts.NC, 0.0
    asym = float(r["asym"]) != 0.0
    if asym:
        fcx = float(r["asym"]) / float(r["fc"])
        c2 = 0.5 * float(r["gamma"]) * fcx
        P = ts.asym_poly(fcx, float(r["asym"]), c2 * c2, xc, h)
    for m in range(2 * int(r["l"]) + 1):
        seed = ts.far_seed(float(r["hv"][m]), ig * (float(r["nu"][m]) - xc), beta)
        c = ts.far_coefs_asym(seed, P) if asym else ts.far_coefs(seed, False)
        tot = [a + b for a, b in zip(tot, c)]
        ab += sum(abs(v) for v in c)
    return tot, ab


def _noise_coefs(t0, t1, xc, h):
    tot, ab = [0.0] * ts.NC, 0.0
    for t, sign in ((t1, 1.0), (t0, -1.0)):
        for k in range(int(t.nh)):
            c = ts.harvey_term_series(sign * float(t.noise[3 * k]), float(t.noise[3 * k + 1]), float(t.noise[3 * k + 2]), xc, h)
            wgt = 1.0 + abs(float(t.noise[3 * k + 2]) * np.log(tr.MILLI * float(t.noise[3 * k + 1]) * xc)) if float(t.noise[3 * k + 1]) != 0.0 else 1.0
            for q in range(ts.NH):
                tot[q] += c[q]
            ab += wgt * sum(abs(v) for v in c)
    tot[0] += float(t1.noise[int(t1.nn) - 1]) - float(t0.noise[int(t0.nn) - 1])
    ab += abs(float(t1.noise[int(t1.nn) - 1])) + abs(float(t0.noise[int(t0.nn) - 1]))
    return tot, ab


GATE_MARGIN = 2.0   # a gate within this factor of 1 is not decided by the restatement: the device's own rounding may put it on either side
TilePath = namedtuple("TilePath", "tile t0 t1 far near moment by_far gate coef_abs far_margin decided")


def tile_paths(ref, t0, t1, x, cfg):
    """The path of every tile that overlaps the slot's range.  far / near: indices into slot.drows of the rows that overlap the tile.
    moment: the tile is taken by the moment form; by_far: by k_fd_far (light slot).  gate: sum_k |c_k| max(1/M0) / 1e-5 where the
    tile's rows are all far (None otherwise); decided: the gate is a factor GATE_MARGIN away from 1.  far_margin: the smallest |beta^2 / (r2 (A^2 + 1)) - 1| over the overlapping rows'
    components -- how far the geometric rule is from flipping."""
    s = slot_of(ref, cfg)
    x = np.asarray(x, dtype=np.float64)
    nx, x0, step = x.size, float(x[0]), float(x[1] - x[0])
    out = []
    if s.hi <= s.lo:
        return out
    for tile in range(s.lo // cfg.tile_bins, (s.hi - 1) // cfg.tile_bins + 1):
        a, b = tile * cfg.tile_bins, min((tile + 1) * cfg.tile_bins, nx)
        xc, h = tr.tile_geometry(tile, cfg.tile_bins, x0, step)
        far, near, margin = [], [], np.inf
        for q, (r, _) in enumerate(s.drows):
            if not (int(r["i0"]) < b and int(r["i1"]) > a):
                continue
            covers = int(r["i0"]) <= a and int(r["i1"]) >= b
            if covers:
                g = float(r["gamma"])
                r2 = tr.R2_FAR_ASYM if float(r["asym"]) != 0.0 else tr.R2_FAR
                for m in range(2 * int(r["l"]) + 1):
                    Am = 2.0 * (float(r["nu"][m]) - xc) / g
                    margin = min(margin, abs((2.0 * h / g) ** 2 / (r2 * (Am * Am + 1.0)) - 1.0))
            (far if cfg.farfield and covers and tr.row_is_far(r, a, b, xc, h) else near).append(q)
        gate = coef_abs = None
        moment, decided = False, True
        bg_ok = (not s.noise_changed) or _series_holds(t0, t1, xc, h)
        if cfg.farfield and cfg.wg == 64 and not s.full and not near and bg_ok:
            tot, coef_abs = [0.0] * ts.NC, 0.0
            for q in far:
                c, ab = _piece_coefs(s.drows[q][0], xc, h)
                tot = [u + v for u, v in zip(tot, c)]
                coef_abs += ab
            if s.noise_changed:
                c, ab = _noise_coefs(t0, t1, xc, h)
                tot = [u + v for u, v in zip(tot, c)]
                coef_abs += ab
            rmax = float(np.max(1.0 / np.abs(ref.M0[a:b]).astype(np.float64)))
            gate = sum(abs(v) for v in tot) * rmax / MOMENT_GATE
            moment = gate <= 1.0
            decided = not (1.0 / GATE_MARGIN <= gate <= GATE_MARGIN)
        out.append(TilePath(tile, a, b, far, near, moment, moment and s.light, gate, coef_abs, margin, decided))
    return out


def _series_holds(t0, t1, xc, h):
    """The background series may stand for BOTH noise rows on this tile: the gate at the steeper of their exponents."""
    n = 3 * int(t0.nh)
    both = np.maximum(np.abs(np.asarray(t0.noise[:n], dtype=np.float64)), np.abs(np.asarray(t1.noise[:n], dtype=np.float64)))
    return tr.series_gate(both, int(t0.nh), xc, h)


Budget = namedtuple("Budget", "truncation far rounding planes total n_moment_tiles n_done_tiles n_closed_bins walked walked_min walked_max")


def slot_budget(ref, t0, t1, x, cfg, paths=None):
    """The four named parts for one slot under one launch geometry, and what the launch's statistics must show for it.  A tile whose gate
    is not decided is granted the larger of its two truncations and roundings, and the walked bins a range (walked_min .. walked_max)."""
    s = slot_of(ref, cfg)
    x = np.asarray(x, dtype=np.float64)
    xl = x.astype(LD)
    paths = tile_paths(ref, t0, t1, x, cfg) if paths is None else paths
    au = np.abs(ref.u).astype(np.float64)
    ayr = np.abs(ref.yr)
    in_moment = np.zeros(x.size, dtype=bool)
    A = ref.A + ref.M0.astype(np.float64) if s.full else ref.A.copy()
    far = 0.0
    x0, step = float(x[0]), float(x[1] - x[0])
    # the rows whose far-field truncation does not cancel: the delta rows; for a full table the changed rows, new and old
    pieces = s.pieces
    for tp in paths:
        sl = slice(tp.t0, tp.t1)
        xc, h = tr.tile_geometry(tp.tile, cfg.tile_bins, x0, step)
        if tp.moment and tp.decided:
            in_moment[sl] = True
            A[sl] = tp.coef_abs
        elif not tp.decided:
            in_moment[sl] = True   # (u^3 omitted: the larger truncation)
            A[sl] = np.maximum(A[sl], tp.coef_abs)
        if not cfg.farfield:
            continue
        for r, _ in pieces:
            if not (int(r["i0"]) <= tp.t0 and int(r["i1"]) >= tp.t1 and tr.row_is_far(r, tp.t0, tp.t1, xc, h)):
                continue
            c = np.abs(tr._row_components_ld(r, xl[sl])).astype(np.float64)
            g = float(r["gamma"])
            for m in range(c.shape[0]):
                if float(r["asym"]) != 0.0:
                    t = ts.TAU_ASYM
                else:
                    Am = 2.0 * (float(r["nu"][m]) - xc) / g
                    q2 = (2.0 * h / g) ** 2 / (Am * Am + 1.0)
                    t = ts.tau(np.sqrt(q2), ts.NC if tp.by_far else ts.n_terms(q2))
                far += t * float((c[m] * ref.w[sl]).sum())
        if s.noise_changed and _series_holds(t0, t1, xc, h):
            for term in ref.noise_terms:
                far += ts.HARVEY_BUDGET * float((term[sl] * ref.w[sl]).sum())
    rng = slice(s.lo, s.hi)
    series = (~in_moment) & (au <= U_SERIES * (1.0 + U_MARGIN))   # (a bin that close to the threshold may take either form)
    trunc = np.where(in_moment, (ayr + 1.0 / 3.0) * au ** 3 / (1.0 - np.minimum(au, 0.5)),
                     np.where(series, (ayr + 1.0 / 6.0) * au ** 6 / (1.0 - np.minimum(au, 0.5)), 0.0))
    truncation = float(trunc[rng].sum())
    rounding = K_ROUND * EPS * float((ref.w[rng] * A[rng]).sum())
    planes = PLANES * float(np.abs(ref.f[rng]).sum()) + 3 * EPS * abs(float(ref.dS))
    n_done = sum(1 for tp in paths if tp.by_far)
    n_open = sum(1 for tp in paths if s.light and not tp.decided)
    n_sure = sum(1 for tp in paths if tp.by_far and tp.decided)
    return Budget(truncation, far, rounding, planes, truncation + far + rounding + planes, sum(1 for tp in paths if tp.moment), n_done,
                  int(np.count_nonzero(au[rng] > U_SERIES)), (s.hi - s.lo) - cfg.tile_bins * n_done, (s.hi - s.lo) - cfg.tile_bins * (n_sure + n_open),
                  (s.hi - s.lo) - cfg.tile_bins * n_sure)


# ---------------------------------------------------------------- the series and the moment form, restated in doubles ----------------------------------------------------------------
def series5(u, yr):
    """The per-bin series of the DELTA launch: f = sum_{n=1..5} (-1)^n (yr - 1/n) u^n, in doubles."""
    pz = u * (0.2 - yr) + (yr - 0.25)
    pz = u * pz + ((1.0 / 3.0) - yr)
    pz = u * pz + (yr - 0.5)
    pz = u * pz + (1.0 - yr)
    return u * pz


def moment2(u, yr):
    """The moment form's integrand: (1 - yr) u + (yr - 1/2) u^2."""
    return (1.0 - yr) * u + (yr - 0.5) * u * u


def bin_exact(u, yr):
    """-(yr) u / (1 + u) + ln(1 + u) at 50 digits."""
    with localcontext() as ctx:
        ctx.prec = PREC
        u, yr = Decimal(float(u)), Decimal(float(yr))
        return -yr * u / (1 + u) + (1 + u).ln()

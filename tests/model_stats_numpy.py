"""The accumulator law of the posterior model spectrum (include/tamcmc_hip.h, csrc/model_stats.hip) as a sequential numpy replay over
given model rows (test helper): one vector at a time, one IEEE operation per statement -- numpy neither fuses nor reorders them --
so that the replay over the device's own STRICT model rows gives the device's bits."""
import numpy as np

KEYS = ("mean", "var", "min", "max", "ratio", "background")


def accepted(weights, status=None):
    """Which vectors the law adds: table status OK and weight > 0."""
    w = np.asarray(weights, dtype=np.float64)
    ok = w > 0.0
    if status is not None:
        ok &= np.asarray(status) == 0
    return ok


def replay(rows, y=None, weights=None, bg_rows=None, status=None, shift=True):
    """rows [B x Nx] model rows in arrival order, y [Nx] (None: no ratio), weights [B] (None: ones), bg_rows [B x Nx] the background of
    each row (None: no background), status [B] table status (None: all good).  shift=False: the textbook sums of w M and w M^2
    without the reference plane (what the law is NOT; test_model_stats_reference.py pins the difference).
    Returns the dict ModelStats.result() returns (arrays None where their input is missing)."""
    rows = np.asarray(rows, dtype=np.float64)
    B, Nx = rows.shape
    w_all = np.ones(B) if weights is None else np.asarray(weights, dtype=np.float64)
    ok = accepted(w_all, status)
    failed = int((np.asarray(status) != 0).sum()) if status is not None else 0
    counts = (int(ok.sum()), failed, B - int(ok.sum()) - failed)
    R = None
    A1, A2, Q, G = np.zeros(Nx), np.zeros(Nx), np.zeros(Nx), np.zeros(Nx)
    mn, mx = np.full(Nx, np.inf), np.full(Nx, -np.inf)
    W = 0.0
    with np.errstate(all="ignore"):
        for b in range(B):
            if not ok[b]:
                continue
            M, w = rows[b], w_all[b]
            if R is None:
                R = M.copy() if shift else np.zeros(Nx)
            d = M - R
            A1 = A1 + w * d
            A2 = A2 + w * (d * d)
            mn = np.where(M < mn, M, mn)
            mx = np.where(M > mx, M, mx)
            if y is not None:
                Q = Q + w * (y / M)
            if bg_rows is not None:
                G = G + w * bg_rows[b]
            W = W + w
        if R is None:
            raise ValueError("nothing accepted")
        v = (A2 - A1 * A1 / W) / W
        out = {"mean": R + A1 / W, "var": np.where(v < 0.0, 0.0, v), "min": mn, "max": mx,
               "ratio": Q / W if y is not None else None, "background": G / W if bg_rows is not None else None}
    out["W"] = W
    out["counts"] = counts
    return out

"""CPU restatement of d3p_predict_discrepancy (include/d3p_hip.h): the six per-draw sums over the rows, float64, in
the stated summation order, GIVEN the float32 mean matrix mu (n, rows) that d3p_predict_mean_rows stores, the outcome matrix v (n,
rows) that d3p_predict_glm / d3p_predict_logreg store (float32 or int32) and the observed vector y (rows,) as float32.

    terms(family, mu, v, y, shift, sigma) -> (6, n, rows) float64: q(y), q(v), m, fl64(m m), ey, fl64(ey ey), each operation one IEEE
                                             float64 operation:  M = fl64(mu);  V = fl64(sigma) fl64(sigma) | M | M (1.0 - M);
                                             q(x) = 0.0 if e == 0.0 else (e e) / V, e = fl64(x) - M;  m = M - shift;  ey = fl64(y) - M
    ordered_sum(t)                        -> (n,): explicit loops over strips, tiles, quarters and rows (vectorised over the draws only): a
                                             quarter's accumulator starts from 0.0, tiles ascending; strip partial = ((q0 + q1) + q2) + q3;
                                             strips merged ascending from strip 0's  (tests/ppc_ref.py's order)
    discrepancy(...)                      -> (6, n): ordered_sum of each of the six
    discrepancy_naive(...)                -> (6, n): math.fsum of the same terms -- only to sanity-check the restatement on the host

numpy's float64 `+`, `*` and `/` are single IEEE operations (no fused multiply-add), which is what the kernel is compiled to.
"""
import math

import numpy as np

from .ppc_ref import QUARTER, TILE, same, strips  # noqa: F401  (re-exported: the tests take them from here)

FAMILIES = ("linear", "poisson", "logistic")


def terms(family, mu, v, y, shift, sigma=None):
    assert family in FAMILIES
    mu, v, y = np.asarray(mu), np.asarray(v), np.asarray(y)
    assert mu.dtype == np.float32 and y.dtype == np.float32 and v.dtype in (np.float32, np.int32)
    mu, v = (a.reshape(1, -1) if a.ndim == 1 else a for a in (mu, v))
    assert mu.shape == v.shape and y.shape == (mu.shape[1],)
    c = np.float64(shift)
    with np.errstate(all="ignore"):
        M = mu.astype(np.float64)
        if family == "linear":
            s = np.float64(np.float32(sigma))
            V = np.broadcast_to(s * s, M.shape)
        elif family == "poisson":
            V = M
        else:
            V = M * (1.0 - M)

        def q(x):
            e = x.astype(np.float64) - M
            return np.where(e == 0.0, 0.0, (e * e) / V)

        m = M - c
        ey = y.astype(np.float64)[None, :] - M
        return np.stack([q(y[None, :]), q(v), m, m * m, ey, ey * ey])


def ordered_sum(t):
    """t (n, rows) float64 -> (n,) in the order of d3p_rep_stats."""
    n, rows = t.shape
    assert rows >= 1
    tiles, per, n_strips = strips(rows)
    total = None
    with np.errstate(all="ignore"):
        for s in range(n_strips):
            qs = np.zeros((4, n))
            for tile in range(s * per, min((s + 1) * per, tiles)):
                for q in range(4):
                    lo = tile * TILE + q * QUARTER
                    for r in range(lo, min(lo + QUARTER, rows)):
                        qs[q] = qs[q] + t[:, r]
            part = ((qs[0] + qs[1]) + qs[2]) + qs[3]
            total = part if s == 0 else total + part
    return total


def discrepancy(family, mu, v, y, shift, sigma=None):
    t = terms(family, mu, v, y, shift, sigma)
    six, n, rows = t.shape
    return ordered_sum(t.reshape(six * n, rows)).reshape(six, n)   # (a sum does not depend on the other rows of the stack)


def discrepancy_naive(family, mu, v, y, shift, sigma=None):
    t = terms(family, mu, v, y, shift, sigma)
    return np.array([[math.fsum(row) if np.isfinite(row).all() else float(np.sum(row)) for row in k] for k in t])

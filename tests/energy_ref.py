"""Comparator of the energy score (d3p_amd/energy.py, d3p_amd/csrc/d3p_energy.hip): a numpy float64 restatement
with math.fsum sums, a float32 emulation of the kernel's distance rule, and the derived error bound.  Nothing here reaches a device.

    exact(draws, y)    -> {"es", "es_fair", "mae", "spread"}: (rows,) float64, distances and sums in float64 (fsum)
    emulate(draws, y)  -> the same from the kernel's float32 rule (t = fl32(a - b), fmaf chain, sqrtf), sums by fsum, rounded to float32
    bound(ex, n, d)    -> {"es", ...}: (rows,) float64, the largest |device - exact| the rule admits
"""
import math

import numpy as np

NAMES = ("es", "es_fair", "mae", "spread")
U32 = 2.0 ** -24      # float32 unit roundoff
U64 = 2.0 ** -53


def _as3(draws, y):
    draws = np.asarray(draws)
    if draws.ndim == 2:
        draws = draws[:, :, None]
    y = np.asarray(y).reshape(draws.shape[1], draws.shape[2])
    return draws, y


def _finish(S1, U, n):
    """The four scores of one row from S1 = sum_i dist(z_i, y) and U = sum_{i<j} dist(z_i, z_j), in float64."""
    with np.errstate(all="ignore"):
        S1, S2, nn = np.float64(S1), np.float64(2.0) * np.float64(U), np.float64(n)
        mae = S1 / nn
        spread = S2 / (2.0 * nn * nn)
        fair = S2 / (2.0 * nn * (nn - 1.0))
        return mae - spread, mae - fair, mae, spread


def _fsum(v):
    v = np.asarray(v, np.float64).ravel()
    if not np.isfinite(v).all():
        return float(v.sum())
    return math.fsum(v.tolist())


def _rows(draws, y, dist):
    draws, y = _as3(draws, y)
    n, rows, d = draws.shape
    out = {k: np.empty(rows, np.float64) for k in NAMES}
    iu = np.triu_indices(n, 1)
    for r in range(rows):
        z = draws[:, r, :]
        if not (np.isfinite(z.astype(np.float64)).all() and np.isfinite(y[r].astype(np.float64)).all()):
            vals = (np.nan,) * 4
        else:
            S1 = _fsum(dist(z, y[r][None, :]))
            U = _fsum(dist(z[iu[0]], z[iu[1]])) if n > 1 else 0.0
            vals = _finish(S1, U, n)
        for k, v in zip(NAMES, vals):
            out[k][r] = v
    return out


def _dist64(a, b):
    t = a.astype(np.float64) - b.astype(np.float64)
    return np.sqrt((t * t).sum(axis=1))


def _q32(a, b):
    """The kernel's chain over the last axis of a and b (which broadcast against each other): t_c = fl32(a_c - b_c), q <- fmaf(t_c, t_c, q)
    over c ascending; the root is taken where q is used.  fmaf is formed as the float64 t * t (exact: 48 bits) plus q rounded to float64
    and then to float32; the double rounding can differ from a true fmaf by one float32 ulp in rare ties, which is inside the bound and
    immaterial to the exact cases."""
    with np.errstate(all="ignore"):
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        q = np.zeros(np.broadcast_shapes(a32.shape[:-1], b32.shape[:-1]), np.float32)
        for c in range(a32.shape[-1]):
            t = (a32[..., c] - b32[..., c]).astype(np.float32)
            q = (t.astype(np.float64) * t.astype(np.float64) + q.astype(np.float64)).astype(np.float32)
        return q


def _dist32(a, b):
    with np.errstate(all="ignore"):
        return np.sqrt(_q32(a, b)).astype(np.float32).astype(np.float64)


def exact(draws, y):
    return _rows(draws, y, _dist64)


def emulate(draws, y):
    with np.errstate(all="ignore"):
        return {k: v.astype(np.float32) for k, v in _rows(draws, y, _dist32).items()}


def _half_ulp32(x):
    x = np.abs(np.asarray(x, np.float64))
    with np.errstate(all="ignore"):
        return 0.5 * np.spacing(np.maximum(x, np.float64(2.0 ** -126)).astype(np.float32)).astype(np.float64)


def bound(ex, n, d):
    """|device - exact| per output: every summand is non-negative, so the errors are relative.  dist carries at most
    (d / 2 + 2) 2^-24 (1 + 2^-10) (one rounding of t, doubled by the square and halved by the root: 1; the chain's d roundings halved:
    d / 2; the root's own: 1/2, rounded up to 1 with the second-order terms, d <= 8192), the float64 sums and the closing divisions
    (n^2 + 8) 2^-53.  es and es_fair are differences: their error is relative to mae + spread, not to themselves.  The final float32
    rounding adds half an ulp of the value rounded, which lies within the first term of the exact one."""
    rel = (d / 2.0 + 2.0) * U32 * (1.0 + 2.0 ** -10) + (n * n + 8.0) * U64
    mae, spread = np.abs(ex["mae"]), np.abs(ex["spread"])
    with np.errstate(all="ignore"):
        fair_spread = np.abs(ex["mae"] - ex["es_fair"])
    first = {"es": rel * (mae + spread), "es_fair": rel * (mae + fair_spread), "mae": rel * mae, "spread": rel * spread}
    return {k: first[k] + _half_ulp32(np.abs(ex[k]) + first[k]) for k in NAMES}

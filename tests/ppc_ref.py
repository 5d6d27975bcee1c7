"""CPU restatement of d3p_rep_stats / d3p_predict_stats (include/d3p_hip.h): the five per-draw statistics of a
draws x rows matrix over its rows, float64, in the stated summation order.

    strips(rows)                -> (tiles, per, strips): tiles = ceil(rows / 128), per = ceil(tiles / 512), strips = ceil(tiles / per)
    rep_stats(m, shift)         -> (5, n) float64: the restatement, explicit loops over strips, tiles, quarters and rows (vectorised over
                                   the draws only): a quarter's accumulator starts from 0.0 and takes e = fl64(v - c) and fl64(e e) one row
                                   at a time, tiles ascending; strip partial = ((q0 + q1) + q2) + q3; strips merged ascending from strip 0's
    rep_stats_naive(m, shift)   -> (5, n): math.fsum of the same terms -- only to sanity-check the restatement on the host

numpy's float64 `+` and `*` are single IEEE operations (no fused multiply-add), which is what the kernels are compiled to.
"""
import math

import numpy as np

TILE, QUARTER, MAX_STRIPS = 128, 32, 512


def strips(rows):
    tiles = -(-int(rows) // TILE)
    per = -(-tiles // MAX_STRIPS) if tiles else 0
    return tiles, per, (-(-tiles // per) if tiles else 0)


def _as_matrix(m):
    m = np.asarray(m)
    assert m.dtype in (np.float32, np.int32), m.dtype
    return m.reshape(1, -1) if m.ndim == 1 else m


def rep_stats(m, shift=0.0):
    m = _as_matrix(m)
    n, rows = m.shape
    assert rows >= 1
    c = np.float64(shift)
    v64 = m.astype(np.float64)                       # exact for float32 and int32
    tiles, per, n_strips = strips(rows)
    total = sq = None
    with np.errstate(all="ignore"):
        for s in range(n_strips):
            qsum = np.zeros((4, n))
            qsq = np.zeros((4, n))
            for t in range(s * per, min((s + 1) * per, tiles)):
                for q in range(4):
                    lo = t * TILE + q * QUARTER
                    for r in range(lo, min(lo + QUARTER, rows)):
                        e = v64[:, r] - c
                        qsum[q] = qsum[q] + e
                        qsq[q] = qsq[q] + e * e
            psum = ((qsum[0] + qsum[1]) + qsum[2]) + qsum[3]
            psq = ((qsq[0] + qsq[1]) + qsq[2]) + qsq[3]
            total = psum if s == 0 else total + psum
            sq = psq if s == 0 else sq + psq
        nan = np.isnan(v64).any(axis=1)
        lo = np.where(nan, np.nan, np.where(np.isnan(v64), np.inf, v64).min(axis=1))
        hi = np.where(nan, np.nan, np.where(np.isnan(v64), -np.inf, v64).max(axis=1))
    zeros = (m == 0).sum(axis=1).astype(np.float64)  # -0.0 == 0, NaN != 0
    return np.stack([total, sq, lo, hi, zeros])


def rep_stats_naive(m, shift=0.0):
    m = _as_matrix(m)
    c = float(shift)
    out = np.empty((5, m.shape[0]))
    for s, row in enumerate(m):
        e = [float(v) - c for v in row]
        out[0, s] = math.fsum(e)
        out[1, s] = math.fsum(x * x for x in e)
        out[2, s], out[3, s] = float(min(row)), float(max(row))
        out[4, s] = sum(1 for v in row if v == 0)
    return out


def same(a, b):
    """Equal by value, NaN equal to NaN (and +0 equal to -0: which zero min / max return is unspecified)."""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)

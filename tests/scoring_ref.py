"""Comparator of d3p_col_crps / d3p_amd.scoring for tests/test_scoring_host.py and tests/test_gpu_scoring.py: the rule of
include/d3p_hip.h restated three times.  Per column of n draws x and the observation y, with s = the draws sorted ascending and
d_i = s_i - y:

    A = sum_i |d_i|     G = sum_i (2 i - n + 1) d_i  (i from 0)  = 1/2 sum_i sum_j |x_i - x_j|
    crps = A / n - G / n^2     crps_fair = A / n - G / (n (n - 1))  (NaN at n = 1)     mae = A / n     spread = G / n^2
    below = #{x < y}     equal = #{x == y}      (IEEE comparison)
    a NaN or infinite draw, or a non-finite y: the four scores NaN  (int32 is never non-finite)

``score_at``        numpy float64 on the sorted columns, the two sums by math.fsum (exactly rounded sums of float64 terms)
``score_pairwise``  the O(n^2) definition  E|X - y| - 1/2 E|X - X'|  on the UNSORTED draws: an independent restatement
``score_exact``     fractions.Fraction, for small shapes: the exact rationals, and their float64 images

``bound(m, y)``: the error budget of one column, derived and not measured.  The device sums n float64 terms per sum, each lane in
sequence and the lanes in a tree: every partial sum rounds once, at most n - 1 additions lie on a term's path, and the terms
themselves carry up to three roundings (d_i, its product with the coefficient, |.| none), the final quotients and the difference
three more: at most (n + 8) roundings of relative size 2^-53 against the sums of the terms' magnitudes.  The result is rounded to
float32 once:

    |got - exact| <= 1/2 ulp32(exact) + (n + 8) 2^-53 (sum |d_i| / n + sum |(2 i - n + 1) d_i| / n^2)

and for crps_fair with n (n - 1) in place of n^2 in the last term.  The same budget holds for mae and spread (each is one of the two
terms), each with the ulp of its own exact value.
"""
import math
from fractions import Fraction

import numpy as np

from tests import hpdi_ref as HR

ROWS = ("crps", "crps_fair", "mae", "spread")
KINDS = HR.KINDS + ("binary",)
INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1
FLOAT_Y = ("inside", "below_all", "above_all", "one_draw", "tied_run", "all_draws", "minus_zero", "nan", "plus_inf", "minus_inf")
INT_Y = ("inside", "below_all", "above_all", "one_draw", "tied_run", "all_draws", "int32_min", "int32_max")


def matrix(kind, n, cols, seed=0):
    """tests/hpdi_ref.matrix's kinds and
    binary   int32 draws in {0, 1}, column c at the frequency (c mod 11) / 10: all 0, mixed, all 1 -- the Brier identity"""
    if kind != "binary":
        return HR.matrix(kind, n, cols, seed)
    rng = np.random.default_rng(9000 * n + cols + seed)
    return (rng.random(size=(n, cols)) < (np.arange(cols) % 11) / 10.0).astype(np.int32)


def y_kinds(m):
    return INT_Y if np.asarray(m).dtype == np.int32 else FLOAT_Y


def observations(m, kinds):
    """One observation per column of m, column c of the kind kinds[c]; of m's dtype.
    inside      the mean of the column's smallest and largest finite draw (int32: the floor)
    below_all / above_all   one step outside the finite draws (int32: clipped to the range)
    one_draw    the draw in row 0          tied_run   the most frequent value of the column (its longest run when sorted)
    all_draws   the draw in the last row: equal to ALL draws in the kinds 'equal' and, often, 'binary'
    minus_zero  -0.0 (against the +0 and -0 draws of 'quarters')     nan / plus_inf / minus_inf
    int32_min / int32_max   the extremes against counts: differences up to 2^32 - 1"""
    m = np.asarray(m)
    n, cols = m.shape
    is_int = m.dtype == np.int32
    y = np.zeros(cols, m.dtype)
    for c in range(cols):
        col, kind = m[:, c], kinds[c]
        fin = col if is_int else col[np.isfinite(col)]
        lo, hi = (fin.min(), fin.max()) if fin.size else (m.dtype.type(0), m.dtype.type(0))
        if kind == "inside":
            y[c] = (int(lo) + int(hi)) // 2 if is_int else np.float32(0.5 * (np.float64(lo) + np.float64(hi)))
        elif kind == "below_all":
            y[c] = max(int(lo) - 1, INT32_MIN) if is_int else np.nextafter(np.float32(lo), np.float32(-np.inf)) - np.float32(abs(lo))
        elif kind == "above_all":
            y[c] = min(int(hi) + 1, INT32_MAX) if is_int else np.nextafter(np.float32(hi), np.float32(np.inf)) + np.float32(abs(hi))
        elif kind == "one_draw":
            y[c] = col[0]
        elif kind == "tied_run":
            vals, counts = np.unique(fin if fin.size else col, return_counts=True)
            y[c] = vals[np.argmax(counts)]
        elif kind == "all_draws":
            y[c] = col[n - 1]
        elif kind == "minus_zero":
            y[c] = -0.0
        elif kind == "nan":
            y[c] = np.nan
        elif kind == "plus_inf":
            y[c] = np.inf
        elif kind == "minus_inf":
            y[c] = -np.inf
        elif kind == "int32_min":
            y[c] = INT32_MIN
        elif kind == "int32_max":
            y[c] = INT32_MAX
        else:
            raise ValueError(kind)
    return y


def rotation(m, r):
    """The kinds of the columns of m at rotation r: column c takes kind (c + r) mod K, so K rotations give every column every kind."""
    ks = y_kinds(m)
    return [ks[(c + r) % len(ks)] for c in range(np.asarray(m).shape[1])]


def nonfinite(m, y):
    """The columns whose four scores are NaN."""
    m, y = np.asarray(m), np.asarray(y)
    if m.dtype == np.int32:
        return np.zeros(m.shape[1], bool)
    return ~np.isfinite(m).all(axis=0) | ~np.isfinite(y)


def counts(m, y):
    """(below, equal): (2, cols) int64, numpy's IEEE comparison."""
    m, y = np.asarray(m), np.asarray(y)
    with np.errstate(invalid="ignore"):
        return np.stack([(m < y[None, :]).sum(0), (m == y[None, :]).sum(0)]).astype(np.int64)


def _terms(m, y):
    """(d, w d): the sorted differences and their weighted form, float64 (n, cols); non-finite columns as zeros."""
    m, y = np.asarray(m), np.asarray(y)
    bad = nonfinite(m, y)
    s = np.sort(np.where(bad[None, :], 0, m).astype(np.float64), axis=0)
    d = s - np.where(bad, 0, y).astype(np.float64)[None, :]
    n = m.shape[0]
    w = (2.0 * np.arange(n) - n + 1.0)[:, None]
    return d, w * d, bad


def score_at(m, y):
    """(4, cols) float64 -- crps, crps_fair, mae, spread, NOT yet rounded to float32 -- and the counts (2, cols)."""
    m = np.asarray(m)
    n, cols = m.shape
    d, wd, bad = _terms(m, y)
    out = np.empty((4, cols), np.float64)
    for c in range(cols):
        A, G = math.fsum(np.abs(d[:, c]).tolist()), math.fsum(wd[:, c].tolist())
        mae, spread = A / n, G / (n * n)
        fair = G / (n * (n - 1)) if n > 1 else np.nan
        out[:, c] = (mae - spread, mae - fair, mae, spread)
    out[:, bad] = np.nan
    return out, counts(m, y)


def score_pairwise(m, y):
    """The definition on the unsorted draws: mae = E|X - y|, spread = 1/2 E|X - X'| over all n^2 pairs (fair: the n (n - 1) pairs)."""
    m, y = np.asarray(m), np.asarray(y)
    n, cols = m.shape
    bad = nonfinite(m, y)
    out = np.empty((4, cols), np.float64)
    for c in range(cols):
        if bad[c]:
            out[:, c] = np.nan
            continue
        x = m[:, c].astype(np.float64)
        mae = math.fsum(np.abs(x - np.float64(y[c])).tolist()) / n
        pairs = math.fsum(np.abs(x[:, None] - x[None, :]).ravel().tolist())
        spread = 0.5 * pairs / (n * n)
        fair = 0.5 * pairs / (n * (n - 1)) if n > 1 else np.nan
        out[:, c] = (mae - spread, mae - fair, mae, spread)
    return out, counts(m, y)


def score_exact(m, y):
    """[[Fraction or None] * cols] * 4: the exact values on the sorted draws (None: NaN, by the non-finite rule or 0 / 0)."""
    m, y = np.asarray(m), np.asarray(y)
    n, cols = m.shape
    bad = nonfinite(m, y)
    out = [[None] * cols for _ in range(4)]
    for c in range(cols):
        if bad[c]:
            continue
        s = sorted(Fraction(int(v)) if m.dtype == np.int32 else Fraction(float(v)) for v in m[:, c])
        yc = Fraction(int(y[c])) if m.dtype == np.int32 else Fraction(float(y[c]))
        A = sum(abs(v - yc) for v in s)
        G = sum((2 * i - n + 1) * (v - yc) for i, v in enumerate(s))
        mae, spread = A / n, G / (n * n)
        out[0][c], out[2][c], out[3][c] = mae - spread, mae, spread
        out[1][c] = mae - G / (n * (n - 1)) if n > 1 else None
    return out


def ulp32(v):
    """The spacing of float32 in the binade of |v| (float64 in, float64 out): 2^(e - 24) for |v| = f 2^e, 1/2 <= f < 1, and the
    smallest subnormal 2^-149 below the normal range; NaN stays NaN."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(np.where(np.isfinite(v), v, 1.0))
    return np.where(np.isnan(v), np.nan, np.ldexp(1.0, np.maximum(e - 24, -149)))


def bound(m, y, exact=None):
    """(4, cols) float64: the budget per output (module docstring) around `exact` (default: score_at's values); NaN where those are NaN."""
    m = np.asarray(m)
    n = m.shape[0]
    if exact is None:
        exact = score_at(m, y)[0]
    d, wd, bad = _terms(m, y)
    a_term = np.abs(d).sum(axis=0) / n
    g_sum = np.abs(wd).sum(axis=0)
    acc = (n + 8) * 2.0 ** -53
    ecdf = acc * (a_term + g_sum / (n * n))
    fair = acc * (a_term + g_sum / (n * (n - 1))) if n > 1 else np.full_like(a_term, np.nan)
    out = 0.5 * ulp32(exact) + np.stack([ecdf, fair, ecdf, ecdf])
    out[:, bad] = np.nan
    return out


def within(got, want, tol):
    """(ok, worst): got (4, cols) float32 lies within tol of want, NaN by class on exactly want's NaNs; worst = the largest
    |got - want| / tol over the finite entries (0 where there is none)."""
    got, want, tol = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(tol, np.float64)
    nan = np.isnan(want)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), nan):
        return False, np.inf
    err = np.abs(got[~nan] - want[~nan])
    ratio = err / tol[~nan]
    return bool(np.all(err <= tol[~nan])), float(ratio.max()) if ratio.size else 0.0

"""Comparator of d3p_col_quantiles / d3p_amd.intervals for tests/test_intervals_host.py and tests/test_gpu_intervals.py: the quantile
rule of include/d3p_hip.h in numpy float64.

    h = (n - 1) p in float64,  lo = floor(h),  g = h - lo                                   (``positions``)
    a = the (lo+1)-th smallest value of the column, b = the (lo+2)-th smallest                 (the float32 / int32 values cast to float64)
    g == 0 or a == b: a;  one of a, b infinite: that infinity;  a = -inf and b = +inf: NaN
    otherwise d = b - a:  a + d g  where g < 0.5,  else  b - d (1 - g)                         (numpy's method='linear')
    one rounding to float32;  a NaN anywhere in the column: NaN

Results are compared BY VALUE (``same_values``): NaN against NaN, everything else with ``==`` -- -0 and +0 are one value in the
contract, and a sort of float64 values may return either.

The end-to-end bound of ``credible_interval`` (``mean_rows``) builds on tests/moments_ref.py and tests/loglik_ref.py and restates
neither: the device's mu[s, r] lies within e[s, r] = |dmu/dt| band_t + link_tol of the float64 one (moments_ref's docstring), an order
statistic of a column moves by at most the largest perturbation of the column, and the interpolation is a convex combination of two
of them, so  |q_dev - q_ref| <= max_s e[s, r] + 2^-23 |q_ref|  (the last term: the one rounding to float32).
"""
import math

import numpy as np

from tests import loglik_ref as LR
from tests import moments_ref as MR

PROBS = (0.0, 0.025, 0.05, 1.0 / 3.0, 0.5, 0.95, 0.975, 1.0)
KINDS = ("normal", "quarters", "equal", "descending", "counts")
HOST_N = (1, 2, 3, 31, 128, 257)
INT32_MAX = 2147483647


def positions(probs, n):
    """[(lo, g)] in Python floats, as d3p_amd.intervals computes them."""
    out = []
    for p in probs:
        h = (n - 1) * float(p)
        lo = int(math.floor(h))
        out.append((lo, h - lo))
    return out


def matrix(kind, n, cols, seed=0):
    """The test matrices, (n, cols): float32, and int32 for 'counts'.
    normal      random normal, column c at the scale 10^(c mod 7 - 3): 1e-3 .. 1e3
    quarters    normal at scale 2 rounded to quarters: heavy ties (and zeros of both signs)
    equal       every draw of a column the same value
    descending  strictly descending along the draws
    counts      Poisson-like int32 counts at rates 0.3 .. 3e4 by column, with 2147483647 and -1 among them"""
    rng = np.random.default_rng(1000 * n + cols + seed + 17 * KINDS.index(kind))
    if kind == "normal":
        scale = 10.0 ** (np.arange(cols) % 7 - 3.0)
        return (rng.normal(size=(n, cols)) * scale).astype(np.float32)
    if kind == "quarters":
        return (np.round(rng.normal(size=(n, cols)) * 2.0 * 4.0) / 4.0).astype(np.float32)
    if kind == "equal":
        return np.ascontiguousarray(np.repeat(rng.normal(size=(1, cols)).astype(np.float32), n, axis=0))
    if kind == "descending":
        base = rng.normal(size=(1, cols))
        return (base + (n - 1 - np.arange(n))[:, None] * (0.5 + rng.random(size=(1, cols)))).astype(np.float32)
    rate = 0.3 * 10.0 ** (np.arange(cols) % 6)
    m = rng.poisson(rate, size=(n, cols)).astype(np.int32)
    mark = rng.random(size=(n, cols))
    m[mark < 0.04] = INT32_MAX
    m[mark > 0.96] = -1
    return m


def cases():
    """(name, matrix) of the host sweep: every kind at every n of HOST_N, 9 columns."""
    return [(f"{kind} n={n}", matrix(kind, n, 9)) for kind in KINDS for n in HOST_N]


def quantiles_at(m, pos):
    """The rule at given positions [(lo, g)] for every column of m (n, cols): (Q, cols) float32."""
    m = np.asarray(m)
    n = m.shape[0]
    m64 = m.astype(np.float64)
    s = np.sort(m64, axis=0)                      # (NaN sorts last; such a column is NaN below)
    nan = np.isnan(m64).any(axis=0)
    out = np.empty((len(pos), m.shape[1]), np.float32)
    for q, (lo, g) in enumerate(pos):
        assert 0 <= lo < n and 0.0 <= g < 1.0 and (g == 0.0 or lo < n - 1)
        a = s[lo]
        b = s[min(lo + 1, n - 1)]
        with np.errstate(invalid="ignore", over="ignore"):
            d = b - a
            lin = a + d * g if g < 0.5 else b - d * (1.0 - g)
            res = np.where(np.isinf(a) & np.isinf(b), np.nan, np.where(np.isinf(a), a, np.where(np.isinf(b), b, lin)))
            res = np.where((a == b) | (g == 0.0), a, res)
            out[q] = np.where(nan, np.nan, res).astype(np.float32)
    return out


def quantiles(m, probs):
    return quantiles_at(m, positions(probs, np.asarray(m).shape[0]))


def same_values(got, want):
    """Equal by value: NaN by class, everything else with == (so -0 equals +0 and the infinities must agree in sign)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.all(got[~gn] == want[~wn]))


def first_difference(got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return None if bad.size == 0 else (tuple(int(i) for i in bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# the non-finite table: (column values, lo, g, expected); float32 columns of 4 draws
INF = np.inf
NONFINITE = [
    ([1.0, 2.0, 3.0, np.nan], 0, 0.0, np.nan),          # a NaN anywhere: NaN, also at p = 0
    ([1.0, 2.0, 3.0, np.nan], 1, 0.5, np.nan),
    ([-INF, 1.0, 2.0, 3.0], 0, 0.0, -INF),
    ([-INF, 1.0, 2.0, 3.0], 0, 0.25, -INF),             # exactly one of a, b infinite: that infinity
    ([-INF, 1.0, 2.0, 3.0], 1, 0.5, 1.5),
    ([0.0, 1.0, 2.0, INF], 2, 0.75, INF),
    ([0.0, 1.0, 2.0, INF], 3, 0.0, INF),
    ([-INF, -INF, INF, INF], 1, 0.5, np.nan),           # a = -inf and b = +inf: NaN
    ([-INF, -INF, INF, INF], 0, 0.5, -INF),             # a == b: a
    ([-INF, -INF, INF, INF], 2, 0.5, INF),
    ([-0.0, 0.0, -0.0, 0.0], 1, 0.5, 0.0),              # -0 and +0 are one value
    ([-0.0, 1.0, -1.0, 0.0], 1, 0.0, 0.0),
]


# ---------------------------------------------------------------- the conditional mean's rows form and the end-to-end bound
def mean_rows(family, X, W, b, sigma):
    """(mu (n, rows) float64 with float32's range for the Poisson rate, e (n, rows): the bound of the device's float32 mu)."""
    t = LR.linear_predictor(X, W, b)
    mu, _, dmu, _ = MR.conditional_moments(family, t, sigma)
    band = LR.product_band(X, W, b, X.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        e = dmu * band + MR._link_tol(family, mu)
    return mu, e


def interval_bound(q_ref, e):
    """Per (probability, row): max_s e[s, r] + 2^-23 |q_ref| (module docstring)."""
    return e.max(axis=0)[None, :] + MR.ROUND * np.abs(np.asarray(q_ref, np.float64))

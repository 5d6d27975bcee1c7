"""Comparator of d3p_col_hpdi / d3p_amd.intervals.hpdi for tests/test_hpdi_host.py and tests/test_gpu_hpdi.py: the rule of
numpyro.diagnostics.hpdi(x, prob, axis=0) as include/d3p_hip.h states it, restated in numpy.  Per column of n draws and per window
length L (``window_lengths``: L = int(prob n) in Python floats):

    s = the draws sorted ascending                      (-0 taken as +0; float32 stays float32, int32 becomes int64)
    len[i] = s[i + L] - s[i],  i = 0 .. n - L - 1       (float32: the float32 difference, one rounding; int32: the exact difference)
    i* = argmin(len), the first minimum                 (a NaN length -- inf - inf -- is below every other, the first one wins: np.argmin)
    (lower, upper) = (s[i*], s[i* + L])                 (stored values; an int32 count is cast to float32 once)
    a NaN anywhere in the column: both ends NaN         (the module's rule, not numpy's sort-last)

``hpdi_at`` is the vectorised form (np.sort, one subtraction of two slices, np.argmin); ``hpdi_loop`` says the same as a plain loop over
the windows of one column at a time, on a list sorted by Python; tests/test_hpdi_host.py holds the two equal.  Results are compared BY
VALUE (``same_values`` of tests/quantiles_ref.py): there is no tolerance anywhere.
"""
import numpy as np

from tests.quantiles_ref import INT32_MAX, first_difference, same_values  # noqa: F401  (re-exported for the tests)
from tests.quantiles_ref import KINDS as Q_KINDS
from tests.quantiles_ref import matrix as q_matrix

KINDS = Q_KINDS + ("lognormal", "bimodal", "two_windows", "infinities")
HOST_N = (1, 2, 3, 9, 31, 128, 257)


def window_lengths(probs, n):
    """[L] in Python floats, as d3p_amd.intervals computes them."""
    return [int(float(p) * n) for p in probs]


def sweep_lengths(n):
    """The window lengths of the sweeps: {0, 1, n // 2, int(0.9 n), n - 2, n - 1} clipped to [0, n - 1], without repeats, ascending."""
    return sorted({min(max(L, 0), n - 1) for L in (0, 1, n // 2, int(0.9 * n), n - 2, n - 1)})


def two_windows_plan(n):
    """(L0, a1, a2) of the kind 'two_windows', or None where n has too few windows: at L0 = int(0.9 n) exactly the windows that start at
    a1 = 1 and at a2 = n - L0 - 1 (the last one) have the minimal length 2 L0 - 1, every other window is 2 L0 or 2 L0 + 1 long."""
    L0 = int(0.9 * n)
    a1, a2 = 1, n - L0 - 1
    if L0 < 2 or a2 - a1 < 2 or a2 - a1 == L0:
        return None
    return L0, a1, a2


def matrix(kind, n, cols, seed=0):
    """The test matrices, (n, cols): those of tests/quantiles_ref.py and
    lognormal    exp(normal), column c at the scale 10^(c mod 5 - 2): skewed to the right
    bimodal      0.35 N(-3, 0.5) + 0.65 N(4, 1), scaled by column
    two_windows  the even numbers 2 i + 4 c with s[a1] and s[a2] raised by 1 (``two_windows_plan``), the draws shuffled per column:
                 small integers, so every float32 length is exact; two windows tie at the minimum of L0 and the first must win
    infinities   normal values with -inf in the first (c mod 4) sorted places and +inf in the last ((c // 4) mod 4): NaN lengths where
                 L is below such a count, infinite lengths elsewhere"""
    if kind in Q_KINDS:
        return q_matrix(kind, n, cols, seed)
    rng = np.random.default_rng(7000 * n + cols + seed + 31 * KINDS.index(kind))
    if kind == "lognormal":
        return (np.exp(rng.normal(size=(n, cols))) * 10.0 ** (np.arange(cols) % 5 - 2.0)).astype(np.float32)
    if kind == "bimodal":
        left = rng.random(size=(n, cols)) < 0.35
        v = np.where(left, rng.normal(-3.0, 0.5, size=(n, cols)), rng.normal(4.0, 1.0, size=(n, cols)))
        return (v * 10.0 ** (np.arange(cols) % 3 - 1.0)).astype(np.float32)
    if kind == "two_windows":
        s = 2.0 * np.arange(n)[:, None] + 4.0 * np.arange(cols)[None, :]
        plan = two_windows_plan(n)
        if plan is not None:
            s[plan[1]] += 1.0
            s[plan[2]] += 1.0
        out = np.empty((n, cols), np.float32)
        for c in range(cols):
            out[:, c] = s[rng.permutation(n), c]
        return out
    m = rng.normal(size=(n, cols)).astype(np.float32)
    for c in range(cols):
        lo, hi = min(c % 4, n), min((c // 4) % 4, n)
        order = np.argsort(m[:, c], kind="stable")
        m[order[:lo], c] = -np.inf
        if hi:
            m[order[n - hi:], c] = np.inf
    return m


def _sorted(m):
    """(s, nan): the columns sorted ascending as the contract orders them, and the columns that hold a NaN (sorted as if it were 0)."""
    m = np.asarray(m)
    if m.dtype == np.int32:
        return np.sort(m.astype(np.int64), axis=0), np.zeros(m.shape[1], bool)
    assert m.dtype == np.float32
    nan = np.isnan(m).any(axis=0)
    v = np.where(np.isnan(m), np.float32(0.0), m) + np.float32(0.0)      # (-0 + 0 = +0)
    return np.sort(v, axis=0), nan


def _first_minimum(s, L):
    n = s.shape[0]
    assert 0 <= L <= n - 1
    with np.errstate(invalid="ignore"):
        lens = s[L:] - s[:n - L]                                          # float32 - float32 = float32; int64 - int64 exact
    assert lens.dtype == s.dtype and lens.shape[0] == n - L
    return np.argmin(lens, axis=0)                                        # (the first NaN if there is one, else the first minimum)


def first_minimum(m, L):
    """i* per column: the vectorised rule."""
    return _first_minimum(_sorted(m)[0], L)


def hpdi_at(m, lens):
    """The rule at given window lengths for every column of m (n, cols): (2 Q, cols) float32, rows 2 q and 2 q + 1 lower and upper."""
    s, nan = _sorted(m)
    cols = np.arange(s.shape[1])
    out = np.empty((2 * len(lens), s.shape[1]), np.float32)
    for q, L in enumerate(lens):
        i = _first_minimum(s, L)
        out[2 * q] = np.where(nan, np.nan, s[i, cols].astype(np.float32))
        out[2 * q + 1] = np.where(nan, np.nan, s[i + L, cols].astype(np.float32))
    return out


def hpdi(m, probs):
    return hpdi_at(m, window_lengths(probs, np.asarray(m).shape[0]))


def hpdi_loop(m, lens):
    """The same rule, one column at a time, as a plain loop over the windows of a list that Python sorted."""
    m = np.asarray(m)
    n, cols = m.shape
    is_int = m.dtype == np.int32
    out = np.empty((2 * len(lens), cols), np.float32)
    for c in range(cols):
        col = [int(v) for v in m[:, c]] if is_int else [np.float32(0.0) if v == 0.0 else np.float32(v) for v in m[:, c]]
        if not is_int and any(v != v for v in col):
            out[:, c] = np.nan
            continue
        s = sorted(col)
        for q, L in enumerate(lens):
            best, best_len = 0, None
            for i in range(n - L):
                with np.errstate(invalid="ignore"):
                    d = s[i + L] - s[i]                                   # np.float32 - np.float32, or Python ints
                if best_len is None:
                    best, best_len = i, d
                elif best_len != best_len:
                    break                                                 # the first NaN length stands
                elif d != d or d < best_len:
                    best, best_len = i, d
            out[2 * q, c], out[2 * q + 1, c] = np.float32(s[best]), np.float32(s[best + L])
    return out


# the fixed columns: (values, L, (lower, upper)); float32 unless the values are ints
INF = np.inf
FIXED = [
    ([1.0, 2.0, 3.0, 10.0], 2, (1.0, 3.0)),
    ([10.0, 3.0, 2.0, 1.0, 2.5], 2, (2.0, 3.0)),                    # lengths 1.5, 1, 7.5 on (1, 2, 2.5, 3, 10)
    ([0.0, 1.0, 2.0, 3.0], 1, (0.0, 1.0)),                          # every window equally long: the first
    ([5.0, 1.0, 4.0], 0, (1.0, 1.0)),                               # L = 0: the smallest draw, width 0
    ([5.0, 1.0, 4.0], 2, (1.0, 5.0)),                               # L = n - 1: the whole range
    ([7.0], 0, (7.0, 7.0)),
    ([-0.0, 0.0, -0.0, 1.0], 2, (0.0, 0.0)),                        # -0 and +0 are one value
    ([1.0, np.nan, 3.0], 1, (np.nan, np.nan)),
    ([0.0, 1.0, 2.0, INF], 1, (0.0, 1.0)),
    ([-INF, 0.0, INF], 1, (-INF, 0.0)),                             # both lengths infinite: the first
    ([3, 1, 2147483647, -2147483648, 2], 4, (-2147483648.0, 2147483648.0)),   # the exact length 2^32 - 1; the ends round once
    ([16777217, 16777219, 16777219, 5], 1, (16777220.0, 16777220.0)),
]
# [-inf, -inf, 1, 2, inf, inf]: i* = 0 at every L (a NaN length is the lowest; where there is none every length is +inf)
INF_COLUMN = [-INF, -INF, 1.0, 2.0, INF, INF]
INF_TABLE = [(0, (-INF, -INF)), (1, (-INF, -INF)), (2, (-INF, 1.0)), (3, (-INF, 2.0)), (4, (-INF, INF)), (5, (-INF, INF))]

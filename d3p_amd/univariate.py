"""Per-column fidelity of a synthetic table against a real one on exact order statistics: every column sorted
over ALL rows, the two-sample Kolmogorov-Smirnov statistic, the 1-Wasserstein distance and the Spearman rank correlation.

    sort_columns(x)                                            -> (d, n) tensor of x's dtype
    midranks(x)                                                -> (n, d) int32, doubled
    spearman(x)                                                -> (d, d) float64
    cdf_distance(a, b)                                         -> CdfDistance(ks, ks_at, w1, n_a, n_b, ks_num)
    univariate_fidelity(real, synthetic, holdout=None, top=5)  -> UnivariateFidelity

PRIVACY.  Every number here is computed from the PRIVATE table, without noise.  Releasing a distance or a correlation, or choosing a
model by looking at one, is NOT covered by the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps of training
and nothing else.  The functions are a diagnostic for the person who holds the data.

``sort_columns`` is the kernel call (``d3p_sort_columns``, ``d3p_amd/csrc/d3p_sort_columns.hip``): ``x`` a 2-D CUDA tensor ``(n, d)``,
float32 or int32, with unit column stride and any row stride ``>= d`` (1-D: ``d = 1``), at most ``2^31 - 1`` rows.  Row ``c`` of the
result is column ``c`` in ascending order of the column reducers' order key: ``-0`` comes out as ``+0``, negative NaNs first, positive
NaNs last.  It is a keys-only radix sort -- no index is carried, where ``torch.sort`` carries an int64 per element -- and exact: the
sorted multiset is unique.  ``midranks`` comes from the same call: ``ranks2[i, c] = #{x_.c < x_ic} + #{x_.c <= x_ic} + 1``, twice the
1-based average rank, an exact integer under ties (at most ``2^30 - 1`` rows); a column that holds a NaN gets 0 in every row.

``spearman`` is ``covariance.correlation``'s arithmetic on ``column_moments`` of the doubled midranks (the factor 2 cancels): exact
integers in, so ties need no correction term.  The int32 path of ``column_moments`` is exact up to ``INT_EXACT = 2^24``: ``2 n`` beyond
that is a ``ValueError``.  A constant column and a column with a NaN give NaN in their row and column.

``cdf_distance`` sorts both tables and makes one call of ``d3p_column_cdf_distance``.  With ``F_a``, ``F_b`` the right-continuous
empirical distribution functions of a column: ``ks = max_v |F_a(v) - F_b(v)|`` from an exact integer numerator (``ks_num``, int64; one
division), ``ks_at`` the smallest pooled value that attains it, ``w1 = integral |F_a - F_b|`` in float64 in one fixed order (the
kernel's header states the order and the error bound).  A NaN in either table gives ``ks = NaN``, ``ks_num = -1``, ``w1 = NaN``; an
infinity without a NaN gives a valid ``ks`` and ``w1 = NaN``.

``univariate_fidelity`` compares ``synthetic`` with ``real``:

    ks, w1                                 per column, as above
    w1_scaled                              ``w1`` over the real column's interquartile range (numpy's ``method='linear'`` on the sorted
                                           column), NaN where that is 0
    worst_columns                          the ``top`` largest ks: ((column, ks), ..)
    spearman_diff_mean, spearman_diff_max  over the strict upper triangle of ``|spearman_s - spearman_r|``; pairs with a NaN in either
                                           table are left out and counted in ``n_pairs_skipped``
    worst_pairs                            the ``top`` largest: (((c, e), |difference|), ..)
    floor                                  with a ``holdout``: the same report for holdout against real (its own ``floor`` None)

Every host check runs before the device is touched; there is no CPU fallback.
"""
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from . import _tables as T
from . import covariance as CV
from ._lib import check, ptr, stream_ptr
from ._tables import INT_EXACT

__all__ = ["sort_columns", "midranks", "spearman", "cdf_distance", "univariate_fidelity", "CdfDistance", "UnivariateFidelity", "INT_EXACT"]

class CdfDistance(NamedTuple):
    ks: torch.Tensor       # (d,) float64: ks_num / (n_a n_b)
    ks_at: torch.Tensor    # (d,) of the tables' dtype: the smallest pooled value that attains ks
    w1: torch.Tensor       # (d,) float64
    n_a: int
    n_b: int
    ks_num: torch.Tensor   # (d,) int64: max |i n_b - j n_a|, -1 in a column with a NaN


class UnivariateFidelity(NamedTuple):
    ks: torch.Tensor
    w1: torch.Tensor
    w1_scaled: torch.Tensor
    worst_columns: Tuple[Tuple[int, float], ...]
    spearman_diff_mean: float
    spearman_diff_max: float
    worst_pairs: Tuple[Tuple[Tuple[int, int], float], ...]
    n_pairs_skipped: int
    n_real: int
    n_synthetic: int
    dim: int
    floor: Optional["UnivariateFidelity"]


def _check_spearman(dx, name, what):
    if 2 * dx[0] > INT_EXACT:
        raise ValueError(f"{what}: {name}: int32 values beyond 2^24 in magnitude: the doubled midranks reach 2 n = {2 * dx[0]} and "
                         "the kernel converts to float32, which is exact only up to there")


def _sort(x, dx, want_ranks):
    """One call of d3p_sort_columns on a checked table: the (d, n) sorted table and, if wanted, the (n, d) doubled midranks."""
    n, d, ld = dx
    lib = _lib.load()
    out = torch.empty((d, n), dtype=x.dtype, device=x.device)
    ranks = torch.empty((n, d), dtype=torch.int32, device=x.device) if want_ranks else None
    ws = torch.empty(int(lib.d3p_sort_columns_workspace(n, d, 1 if want_ranks else 0)), dtype=torch.uint8, device=x.device)
    check(lib.d3p_sort_columns(stream_ptr(), ptr(x), T.dtype_code(x), ld, n, d, ptr(out), n, ptr(ranks), d, ptr(ws),
                               int(ws.numel())))
    return out, ranks


def _cdf(sa, sb):
    """One call of d3p_column_cdf_distance on two sorted (d, n) tables."""
    d, n_a, n_b = int(sa.shape[0]), int(sa.shape[1]), int(sb.shape[1])
    lib = _lib.load()
    dev = sa.device
    num = torch.empty(d, dtype=torch.int64, device=dev)
    at = torch.empty(d, dtype=sa.dtype, device=dev)
    w1 = torch.empty(d, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.d3p_column_cdf_distance_workspace(n_a, n_b, d)), dtype=torch.uint8, device=dev)
    check(lib.d3p_column_cdf_distance(stream_ptr(), ptr(sa), n_a, n_a, ptr(sb), n_b, n_b, T.dtype_code(sa), d, ptr(num),
                                      ptr(at), ptr(w1), ptr(ws), int(ws.numel())))
    ks = torch.where(num < 0, torch.full_like(w1, float("nan")), num.to(torch.float64) / float(n_a * n_b))
    return CdfDistance(ks, at, w1, n_a, n_b, num)


def sort_columns(x):
    """Every column of ``x`` sorted over all rows (module docstring): a ``(d, n)`` tensor of ``x``'s dtype on its device."""
    what = "sort_columns"
    dx = T.check_rows(T.check_table(x, "x", what), "x", what, False)
    with T.on_device((("x", x),), what):
        return _sort(x, dx, False)[0]


def midranks(x):
    """The doubled midranks of every column of ``x`` (module docstring): ``(n, d)`` int32 on the table's device."""
    what = "midranks"
    dx = T.check_rows(T.check_table(x, "x", what), "x", what, True)
    with T.on_device((("x", x),), what):
        return _sort(x, dx, True)[1]


def _rank_m2(ranks):
    return CV._moments(ranks, (int(ranks.shape[0]), int(ranks.shape[1]), int(ranks.shape[1]))).m2


def spearman(x):
    """The ``(d, d)`` float64 Spearman rank correlation matrix of the columns of ``x`` (module docstring)."""
    what = "spearman"
    dx = T.check_rows(T.check_table(x, "x", what), "x", what, True)
    _check_spearman(dx, "x", what)
    with T.on_device((("x", x),), what):
        return CV._corr(_rank_m2(_sort(x, dx, True)[1]))


def cdf_distance(a, b):
    """The two-sample KS statistic and the 1-Wasserstein distance per column of the tables ``a`` and ``b`` (module docstring): a
    ``CdfDistance`` on the tables' device.  These are functions of the PRIVATE tables and are not covered by the accountant."""
    what = "cdf_distance"
    da, db = T.check_pair(a, b, ("a", "b"), what)
    T.check_rows(da, "a", what, False)
    T.check_rows(db, "b", what, False)
    with T.on_device((("a", a), ("b", b)), what):
        return _cdf(_sort(a, da, False)[0], _sort(b, db, False)[0])


def _iqr(s):
    """The interquartile range of every row of a sorted (d, n) table, numpy's method='linear', float64."""
    n = int(s.shape[1])

    def q(p):
        pos = p * (n - 1)
        lo = int(pos)
        hi = min(lo + 1, n - 1)
        a, b = s[:, lo].to(torch.float64), s[:, hi].to(torch.float64)
        return a + (b - a) * (pos - lo)
    return q(0.75) - q(0.25)


def _report(sr, rho_r, ss, rho_s, top):
    """UnivariateFidelity (floor None) from the sorted tables and the Spearman matrices of the real and of the other table."""
    d = int(sr.shape[0])
    dist = _cdf(sr, ss)
    iqr = _iqr(sr)
    scaled = torch.where(iqr > 0, dist.w1 / iqr, torch.full_like(iqr, float("nan")))
    w = torch.topk(torch.nan_to_num(dist.ks, nan=-1.0), min(top, d)) if top else None
    worst_c = tuple((i, float(dist.ks[i])) for i in w.indices.tolist()) if w is not None else ()
    kept, n_skipped, worst_p = T.worst_pairs((rho_s - rho_r).abs(), top)
    nan = float("nan")
    return UnivariateFidelity(dist.ks, dist.w1, scaled, worst_c, float(kept.mean()) if kept.numel() else nan,
                              float(kept.max()) if kept.numel() else nan, worst_p, n_skipped, int(sr.shape[1]), int(ss.shape[1]), d, None)


def univariate_fidelity(real, synthetic, holdout=None, top=5):
    """The per-column KS and Wasserstein-1 distances and the Spearman fidelity of ``synthetic`` against ``real`` -- and, with a
    ``holdout``, the noise floor that the holdout scores against ``real`` (module docstring): a ``UnivariateFidelity``.  These are
    functions of the PRIVATE tables and are not covered by the accountant."""
    what = "univariate_fidelity"
    tables = T.check_group(real, synthetic, holdout, ("real", "synthetic", "holdout"), what)
    for name, _, dx in tables:
        T.check_rows(dx, name, what, True)
        _check_spearman(dx, name, what)
    if isinstance(top, bool) or not isinstance(top, int) or top < 0:
        raise ValueError(f"{what}: top must be a non-negative int")
    with T.on_device(tables, what):
        sorted_rho = []
        for _, t, dx in tables:
            s, ranks = _sort(t, dx, True)
            sorted_rho.append((s, CV._corr(_rank_m2(ranks))))
        rep = _report(*sorted_rho[0], *sorted_rho[1], top)
        if holdout is not None:
            rep = rep._replace(floor=_report(*sorted_rho[0], *sorted_rho[2], top))
        return rep

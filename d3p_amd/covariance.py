"""Second-moment fidelity of a synthetic table against a real one: column means, covariance, Pearson correlation
and the Gaussian Frechet distance, from ONE contraction over the rows on the matrix cores.

    column_moments(x)                                         -> ColumnMoments(n, mean, m2)
    covariance(x, ddof=1)                                     -> (d, d) float64
    correlation(x)                                            -> (d, d) float64
    correlation_fidelity(real, synthetic, holdout=None, top=5) -> CorrelationFidelity

PRIVACY.  Every number here is computed from the PRIVATE table, without noise.  Releasing a mean, a correlation or a distance, or
choosing a model by looking at one, is NOT covered by the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps of
training and nothing else.  The functions are a diagnostic for the person who holds the data.

``column_moments`` is the kernel call (``d3p_column_moments``, ``d3p_amd/csrc/d3p_column_moments.hip``): ``x`` a 2-D CUDA tensor ``(n,
d)``, float32 or int32, with unit column stride and any row stride ``>= d`` (1-D: ``d = 1``).  ``mean[c]`` is the column mean and
``m2[c, e] = sum_i (x_ic - mean_c)(x_ie - mean_e)``, both float64, by the shifted-data algorithm: the rows are shifted by the float32
rounding of the column mean BEFORE the products are taken, so a column whose mean is a million times its spread loses nothing, where
the float32 Gram form of ``torch.cov`` loses everything.  ``m2`` is symmetric to the bit and deterministic to the bit: ``m2[c, e]``
depends on the columns ``c`` and ``e``, ``n``, ``d`` and the dtype alone (the kernel's header states the order of summation and
DESIGN 4z the error bound).  A column that holds a NaN or an infinity gets NaN in its mean and in its row and column of ``m2``, and
touches no other column.  int32 values beyond ``2^24`` in magnitude are a ``ValueError`` (this one check reads the table, so it runs
on the device, after every other).  The workspace and the outputs are allocated with ``torch.empty``.  Every other host check runs
before the device is touched; there is no CPU fallback.

``covariance`` is ``m2 / (n - ddof)`` and ``correlation`` is ``m2[c, e] / sqrt(m2[c, c] m2[e, e])``: float64 torch on the ``d x d``
result.  A column with ``m2[c, c] == 0`` (a constant) or a flagged column gives NaN in its row and column of the correlation; the
diagonal is exactly 1 otherwise.

``correlation_fidelity`` compares ``synthetic`` with ``real``:

    smd, sd_ratio                          per column ``|mean_s - mean_r| / sd_r`` and ``sd_s / sd_r`` (sd with ddof = 1)
    worst_columns                          the ``top`` largest smd: ((column, smd), ..)
    corr_diff_mean, corr_diff_max, corr_diff_frobenius
                                           over the strict upper triangle of ``corr_s - corr_r``: the mean absolute value, the largest
                                           and the root of the sum of squares; pairs with a NaN correlation in either table are left
                                           out and counted in ``n_pairs_skipped``
    worst_pairs                            the ``top`` largest: (((c, e), |difference|), ..)
    frechet                                the Gaussian 2-Wasserstein distance squared (the Frechet distance of the FID),
                                           ``|mu_r - mu_s|^2 + tr(C_r + C_s - 2 (C_r^{1/2} C_s C_r^{1/2})^{1/2})``
    floor                                  with a ``holdout``: the same report for holdout against real (its own ``floor`` None) -- what
                                           a fresh sample of the same distribution scores, as ``d3p_amd.marginals`` reports it

``frechet`` takes two symmetric float64 eigendecompositions in torch with the eigenvalues clamped at 0; it is plumbing with no
performance claim, and NaN when a column of either table is flagged.
"""
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from . import _tables as T
from ._lib import check, ptr, stream_ptr
from ._tables import INT_EXACT

__all__ = ["column_moments", "covariance", "correlation", "correlation_fidelity", "ColumnMoments", "CorrelationFidelity", "INT_EXACT"]


class ColumnMoments(NamedTuple):
    n: int
    mean: torch.Tensor     # (d,) float64
    m2: torch.Tensor       # (d, d) float64: sum_i (x_ic - mean_c)(x_ie - mean_e)


class CorrelationFidelity(NamedTuple):
    smd: torch.Tensor                  # (d,) float64: |mean_s - mean_r| / sd_r
    sd_ratio: torch.Tensor             # (d,) float64: sd_s / sd_r
    worst_columns: Tuple[Tuple[int, float], ...]
    corr_diff_mean: float
    corr_diff_max: float
    corr_diff_frobenius: float
    worst_pairs: Tuple[Tuple[Tuple[int, int], float], ...]
    n_pairs_skipped: int
    frechet: float
    n_real: int
    n_synthetic: int
    dim: int
    floor: Optional["CorrelationFidelity"]


def _moments(x, dx):
    """One call of d3p_column_moments on a checked table."""
    n, d, ld = dx
    lib = _lib.load()
    mean = torch.empty(d, dtype=torch.float64, device=x.device)
    m2 = torch.empty((d, d), dtype=torch.float64, device=x.device)
    ws = torch.empty(int(lib.d3p_column_moments_workspace(n, d)), dtype=torch.uint8, device=x.device)
    check(lib.d3p_column_moments(stream_ptr(), ptr(x), T.dtype_code(x), ld, n, d, ptr(mean), ptr(m2), d, ptr(ws), int(ws.numel())))
    return ColumnMoments(n, mean, m2)


def standardise(x, dx):
    """(shift, inverse std) of a checked table from ONE ``_moments`` call, for the walkers that centre and scale on load: the float32
    rounding of the column means, and ``1 / std`` (``ddof = 1``) in float64 with 0 for a constant column and for every column of a
    one-row table."""
    mom = _moments(x, dx)
    sd = (mom.m2.diagonal() / float(dx[0] - 1)).sqrt() if dx[0] > 1 else torch.zeros_like(mom.mean)
    return mom.mean.to(torch.float32), torch.where(sd > 0, 1.0 / sd, torch.zeros_like(sd))


def _check_ddof(ddof, n, what):
    if isinstance(ddof, bool) or not isinstance(ddof, int) or ddof < 0 or ddof >= n:
        raise ValueError(f"{what}: ddof must be an int in [0, n), got {ddof!r} at n = {n}")
    return ddof


def column_moments(x):
    """The column means and the centred cross-product matrix of ``x`` (module docstring): a ``ColumnMoments`` on the table's device."""
    what = "column_moments"
    dx = T.check_table(x, "x", what)
    with T.on_device((("x", x),), what, exact=(("x", x),)):
        return _moments(x, dx)


def covariance(x, ddof=1):
    """The ``(d, d)`` float64 covariance matrix of the columns of ``x``: ``m2 / (n - ddof)`` (module docstring)."""
    what = "covariance"
    dx = T.check_table(x, "x", what)
    _check_ddof(ddof, dx[0], what)
    with T.on_device((("x", x),), what, exact=(("x", x),)):
        return _moments(x, dx).m2 / float(dx[0] - ddof)


def _corr(m2):
    """The correlation matrix of a centred cross-product matrix: NaN in the row and column of a column whose m2[c, c] is 0 or NaN, the
    diagonal exactly 1 otherwise."""
    q = torch.diagonal(m2)
    scale = torch.sqrt(q[:, None] * q[None, :])
    bad = ~(q > 0) | ~torch.isfinite(q)
    r = m2 / scale
    r[bad, :] = float("nan")
    r[:, bad] = float("nan")
    good = (~bad).nonzero().flatten()
    r[good, good] = 1.0
    return r


def correlation(x):
    """The ``(d, d)`` float64 Pearson correlation matrix of the columns of ``x`` (module docstring)."""
    what = "correlation"
    dx = T.check_table(x, "x", what)
    with T.on_device((("x", x),), what, exact=(("x", x),)):
        return _corr(_moments(x, dx).m2)


def _sqrt_psd(c):
    """The symmetric square root of a symmetric positive semi-definite float64 matrix: eigenvalues clamped at 0."""
    w, v = torch.linalg.eigh(c)
    return (v * torch.sqrt(torch.clamp(w, min=0.0))) @ v.T


def _frechet(mu_r, c_r, mu_s, c_s):
    """|mu_r - mu_s|^2 + tr(C_r + C_s - 2 (C_r^{1/2} C_s C_r^{1/2})^{1/2}), NaN when a moment is not finite."""
    if not bool(torch.isfinite(mu_r).all() & torch.isfinite(mu_s).all() & torch.isfinite(c_r).all() & torch.isfinite(c_s).all()):
        return float("nan")
    root = _sqrt_psd(c_r)
    inner = root @ c_s @ root
    w = torch.linalg.eigvalsh(0.5 * (inner + inner.T))
    cross = torch.sqrt(torch.clamp(w, min=0.0)).sum()
    return float(((mu_r - mu_s) ** 2).sum() + torch.trace(c_r) + torch.trace(c_s) - 2.0 * cross)


def _report(mr, ms, top):
    """CorrelationFidelity (floor None) from the ColumnMoments of the real and of the other table."""
    d = int(mr.mean.shape[0])
    c_r, c_s = mr.m2 / max(mr.n - 1, 1), ms.m2 / max(ms.n - 1, 1)
    sd_r, sd_s = torch.sqrt(torch.diagonal(c_r)), torch.sqrt(torch.diagonal(c_s))
    smd = (ms.mean - mr.mean).abs() / sd_r
    ratio = sd_s / sd_r
    ranked = torch.nan_to_num(smd, nan=-1.0)
    w1 = torch.topk(ranked, min(top, d)) if top else None
    worst_c = tuple((i, float(smd[i])) for i in w1.indices.tolist()) if w1 is not None else ()
    kept, n_skipped, worst_p = T.worst_pairs((_corr(ms.m2) - _corr(mr.m2)).abs(), top)
    nan = float("nan")
    return CorrelationFidelity(smd, ratio, worst_c, float(kept.mean()) if kept.numel() else nan, float(kept.max()) if kept.numel() else nan,
                               float(torch.sqrt((kept * kept).sum())) if kept.numel() else nan, worst_p, n_skipped,
                               _frechet(mr.mean, c_r, ms.mean, c_s), mr.n, ms.n, d, None)


def correlation_fidelity(real, synthetic, holdout=None, top=5):
    """The mean, spread, correlation and Frechet fidelity of ``synthetic`` against ``real`` -- and, with a ``holdout``, the noise floor
    that the holdout scores against ``real`` (module docstring): a ``CorrelationFidelity``.  These are functions of the PRIVATE tables
    and are not covered by the accountant."""
    what = "correlation_fidelity"
    tables = T.check_group(real, synthetic, holdout, ("real", "synthetic", "holdout"), what)
    if isinstance(top, bool) or not isinstance(top, int) or top < 0:
        raise ValueError(f"{what}: top must be a non-negative int")
    with T.on_device(tables, what, exact=tables):
        mr, *others = [_moments(t, dims) for _, t, dims in tables]
        rep = _report(mr, others[0], top)
        if holdout is not None:
            rep = rep._replace(floor=_report(mr, others[1], top))
        return rep

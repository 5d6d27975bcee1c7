"""CRPS and PIT (rank) calibration of predictive draws against the observed outcomes.

    score_draws(matrix, y)                     -> {"crps", "crps_fair", "mae", "spread"}: (cols,) float32; {"below", "equal"}: (cols,) int32
    crps(matrix, y, fair=False)                -> (cols,) float32
    pit(matrix, y)                             -> (lower, upper): (cols,) float32
    pit_histogram(lower, upper, bins=10)       -> (bins,) float64
    draws_limit()                              -> d3p_col_crps_max_n()
    predictive_crps(rng_key, model, posterior_samples, X, y[, N], fair=False, pointwise=False, bins=10, slab_bytes=64 << 20) -> CRPSResult
    posterior_predictive_crps(rng_key, n, model, model_args, guide, params, fair=False, pointwise=False, bins=10, slab_bytes=64 << 20)
    compare_scores(a, b)                       -> ScoreComparison(crps_diff, se_diff), negative favouring a

``score_draws`` is the model-free reduction (``d3p_col_crps``, ``d3p_amd/csrc/d3p_crps.hip``, kernel in ``d3p_crps_kernel.h``) over
the matrix contract of ``intervals.quantiles``: a 2-D CUDA float32 or int32 tensor ``(draws, cols)``, any row stride, unit column stride; ``y`` holds one
observation per column.  Per column of ``n`` draws sorted ascending as ``s`` and ``d_i = s_i - y`` in float64:

    mae = sum |d_i| / n        spread = sum (2 i - n + 1) d_i / n^2 = 1/2 E|X - X'| over the empirical distribution
    crps = mae - spread        (the ECDF form: properscoring.crps_ensemble, scoringRules::crps_sample)
    crps_fair = mae - sum (2 i - n + 1) d_i / (n (n - 1))     (the unbiased spread; NaN at n = 1)
    below = #{x_s < y}         equal = #{x_s == y}             (IEEE comparison: a NaN counts nowhere, -0 equals +0)

each float rounded to float32 once.  A NaN or infinite draw, or a non-finite ``y``, makes the column's four scores NaN.  For draws in
{0, 1} the CRPS is ``(p - y)^2`` with ``p`` the draws' frequency of 1: the Brier score.  The column is sorted in LDS, which bounds
the draws: ``n <= draws_limit()`` = 18432, a ``ValueError`` above.  For an int32 matrix a float ``y`` with integral values in int32's
range is cast; any other ``y`` dtype mismatch is a ``ValueError``.

``pit`` is where ``y`` falls among its column's draws: ``(below / n, (below + equal) / n)``.  The two coincide for continuous outcomes
without ties; for counts they are the ends of the randomised PIT of Czado, Gneiting and Held (2009).  ``pit_histogram`` is the
NON-randomised histogram: each row spreads mass 1 uniformly over ``[lower, upper]``; where the two are equal it is a point mass in that
value's bin (1.0 goes to the last bin).  It sums to the row count; ``/ rows * bins`` gives the density.  A U shape says the predictive
is too narrow, a hump that it is too wide.

The model layer scores ``LinearRegression`` (float32 outcomes), ``PoissonRegression`` (int32 counts) and ``LogisticRegression`` (int32
in {0, 1}); every other model raises ``TypeError``.  The draws are exactly what ``predictive.predictive_samples`` and
``predictive.posterior_predictive_samples`` return for the same key.  As for ``intervals.predictive_interval`` the matrix is written
whole and its ``4 n rows`` bytes must fit ``slab_bytes`` (the outcome kernel has no row offset).  ``y`` is READ here: one label per row,
for Poisson non-negative integers.  Every host check runs before the device is touched; there is no CPU fallback.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import infer_util as U
from . import intervals as IV
from . import modelling as M
from . import predictive as PS
from ._lib import check, ptr, stream_ptr

__all__ = ["score_draws", "crps", "pit", "pit_histogram", "draws_limit", "predictive_crps", "posterior_predictive_crps", "compare_scores",
           "CRPSResult", "ScoreComparison"]

INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1


class CRPSResult(NamedTuple):
    crps: torch.Tensor           # 0-d float64: the mean over the rows (of crps_fair with fair=True)
    se: torch.Tensor             # its standard error from the pointwise values
    mae: torch.Tensor            # 0-d float64: the mean over the rows
    spread: torch.Tensor         # 0-d float64: the mean over the rows
    pit_histogram: torch.Tensor  # (bins,) float64
    n_draws: int
    n_rows: int
    pointwise: Optional[dict]    # None, or {"crps", "mae", "spread", "pit_lower", "pit_upper"}: (rows,) float32


class ScoreComparison(NamedTuple):
    crps_diff: torch.Tensor      # 0-d float64: mean CRPS of a minus that of b (negative favours a)
    se_diff: torch.Tensor        # its standard error from the paired pointwise differences


def draws_limit():
    """d3p_col_crps_max_n(): the largest draw count whose column is sorted in LDS (host only: no device is touched)."""
    return int(_lib.load().d3p_col_crps_max_n())


def _check_score_draws(n, what):
    most = draws_limit()
    if n > most:
        raise ValueError(f"{what}: {n} draws; the score sorts a column in LDS and runs at most {most} draws (n <= {most})")


def _observations(y, dtype, cols, what):
    """y as a 1-D tensor of `dtype` (the matrix's) and length cols, on whatever device it lies; the values are not moved."""
    if not isinstance(y, torch.Tensor):
        try:
            y = torch.as_tensor(np.asarray(y))
        except (TypeError, ValueError, RuntimeError) as e:
            raise ValueError(f"{what}: y is not an array of numbers") from e
    y = y.detach()
    if y.numel() != cols:
        raise ValueError(f"{what}: y: {cols} observations expected (one per column of the matrix), got {y.numel()}")
    y = y.reshape(cols)
    if y.dtype == dtype:
        return y
    if y.dtype == torch.bool or y.is_complex():
        raise ValueError(f"{what}: y must hold {dtype} values, got {y.dtype}")
    if dtype == torch.float32:
        if not (y.is_floating_point() or y.dtype in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)):
            raise ValueError(f"{what}: y must hold {dtype} values, got {y.dtype}")
        return y.to(torch.float32)
    # an int32 matrix: integers, or floats with integral values, in int32's range
    wide = y.to(torch.float64) if y.is_floating_point() else y.to(torch.int64)
    if y.is_floating_point() and not bool((wide == torch.floor(wide)).all()):   # (a NaN fails; an infinity fails the range below)
        raise ValueError(f"{what}: y: an int32 matrix is scored against integers, got non-integral (or non-finite) values")
    if not bool(((wide >= INT32_MIN) & (wide <= INT32_MAX)).all()):
        raise ValueError(f"{what}: y: values outside int32's range")
    return wide.to(torch.int32)


def _score(m, ld, n, cols, y):
    """The six rows of d3p_col_crps for the (n, cols) matrix that starts at tensor m; y on m's device, of m's dtype."""
    out = torch.empty((4, cols), dtype=torch.float32, device=m.device)
    counts = torch.empty((2, cols), dtype=torch.int32, device=m.device)
    if cols:
        check(_lib.load().d3p_col_crps(stream_ptr(), ptr(m), 0 if m.dtype == torch.float32 else 1, ld, n, cols, ptr(y), ptr(out), cols,
                                       ptr(counts), cols))
    return {"crps": out[0], "crps_fair": out[1], "mae": out[2], "spread": out[3], "below": counts[0], "equal": counts[1]}


def score_draws(matrix, y):
    """CRPS, fair CRPS, mean absolute error, spread and the two rank counts of every column of ``matrix`` against ``y`` (module
    docstring): ``{"crps", "crps_fair", "mae", "spread"}`` as ``(cols,)`` float32 and ``{"below", "equal"}`` as ``(cols,)`` int32 on the
    matrix's device."""
    return _score_draws(matrix, y, "score_draws")


def _score_draws(matrix, y, what):
    n, cols, ld = IV._check_matrix(matrix, what, _check_score_draws)
    y = _observations(y, matrix.dtype, cols, what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(matrix.device):
        return _score(matrix, ld, n, cols, y.to(matrix.device).contiguous())


def crps(matrix, y, fair=False):
    """The CRPS of every column's draws against ``y``: ``(cols,)`` float32; ``fair=True``: the unbiased-spread form."""
    return _score_draws(matrix, y, "crps")["crps_fair" if fair else "crps"]


def _pit_of(below, equal, n):
    return below.to(torch.float32) / n, (below + equal).to(torch.float32) / n


def pit(matrix, y):
    """``(lower, upper) = (below / n, (below + equal) / n)`` per column, float32 (module docstring)."""
    s = _score_draws(matrix, y, "pit")
    return _pit_of(s["below"], s["equal"], int(matrix.shape[0]))


def _bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, int) or bins < 1:
        raise ValueError(f"bins must be an int >= 1, got {bins!r}")
    return bins


def pit_histogram(lower, upper, bins=10):
    """The non-randomised PIT histogram over ``bins`` equal bins of [0, 1]: ``(bins,)`` float64 on the inputs' device.  Row r spreads
    mass 1 uniformly over ``[lower[r], upper[r]]``; where the two are equal it is a point mass in that value's bin, 1.0 in the last."""
    bins = _bins(bins)
    if not isinstance(lower, torch.Tensor) or not isinstance(upper, torch.Tensor) or lower.shape != upper.shape or lower.dim() != 1:
        raise ValueError("pit_histogram: lower and upper must be 1-D tensors of one length")
    lo, hi = lower.to(torch.float64), upper.to(torch.float64)
    if lo.numel() and not bool(((lo >= 0.0) & (lo <= hi) & (hi <= 1.0)).all()):
        raise ValueError("pit_histogram: 0 <= lower <= upper <= 1 is required in every row")
    edges = torch.arange(bins + 1, dtype=torch.float64, device=lo.device) / bins
    width = hi - lo
    point = width == 0.0
    # an interval row: its overlap with every bin over its width
    overlap = (torch.minimum(hi[:, None], edges[None, 1:]) - torch.maximum(lo[:, None], edges[None, :-1])).clamp_min(0.0)
    share = torch.where(point[:, None], torch.zeros_like(overlap), overlap / torch.where(point, torch.ones_like(width), width)[:, None])
    hist = share.sum(dim=0)
    # a point row: the bin of its value, 1.0 in the last
    at = torch.clamp(torch.floor(lo * bins).to(torch.int64), max=bins - 1)
    mine = (at[:, None] == torch.arange(bins, device=lo.device)[None, :]) & point[:, None]
    return hist + mine.to(torch.float64).sum(dim=0)


def _family(model, what):
    fam = U._FAMILY.get(type(model))
    if fam is None:
        raise TypeError(f"{what}: unsupported model {type(model).__name__} (LinearRegression, PoissonRegression and LogisticRegression "
                        "have scalar outcomes to score)")
    return fam


def _mean_and_se(x):
    """(mean_r x[r], sqrt(Var_r x[r] / rows)) in float64, the sample variance; one row: NaN (0 / 0)."""
    x = x.to(torch.float64)
    rows = x.shape[0]
    mean = x.sum() / rows
    dev = x - mean
    return mean, torch.sqrt((dev * dev).sum() / (rows - 1) / rows)


def _result(obs, y, n, rows, fair, pointwise, bins):
    obs = obs.reshape(n, rows)
    with torch.cuda.device(obs.device):
        s = _score(obs, rows, n, rows, y.to(obs.device).contiguous())
        point = s["crps_fair" if fair else "crps"]
        lower, upper = _pit_of(s["below"], s["equal"], n)
        mean, se = _mean_and_se(point)
        pw = {"crps": point, "mae": s["mae"], "spread": s["spread"], "pit_lower": lower, "pit_upper": upper} if pointwise else None
        return CRPSResult(mean, se, s["mae"].to(torch.float64).sum() / rows, s["spread"].to(torch.float64).sum() / rows,
                          pit_histogram(lower, upper, bins), n, rows, pw)


def _labels(model, fam, model_args, rows, what):
    """The observed outcomes as the predictive matrix's dtype: (rows,) float32 for the linear family, int32 for the other two."""
    U._data(model, model_args)   # (y present, one label per row, Poisson: counts)
    y = _observations(model_args[1], torch.float32 if fam == _lib.D3P_FAMILY_LINREG else torch.int32, rows, what)
    if fam == _lib.D3P_FAMILY_POISSON and not bool((y >= 0).all()):   # (whatever the model's validate_args: a negative count has no rank)
        raise ValueError(f"{what}: y: the labels of a PoissonRegression must be integers >= 0")
    return y


def predictive_crps(rng_key, model, posterior_samples, *model_args, fair=False, pointwise=False, bins=10, slab_bytes=64 << 20, **kwargs):
    """CRPS and PIT histogram of the outcomes ``obs`` over given posterior draws against the observed ``y``: the scores of what
    ``predictive_samples(rng_key, model, posterior_samples, X)`` returns, without that matrix leaving the device.  ``model_args = (X,
    y[, N])``.  ``fair=True`` scores with the unbiased spread; ``pointwise=True`` keeps the per-row arrays."""
    what = "predictive_crps"
    fam = _family(model, what)
    bins = _bins(bins)
    rows, d = PS._data(model, model_args, kwargs)
    y = _labels(model, fam, model_args, rows, what)
    n, _ = U._sample_shape(model, posterior_samples, d)
    _check_score_draws(n, what)
    IV._check_whole(n, rows, slab_bytes, what)
    M._check_key(rng_key)
    obs = PS.predictive_samples(rng_key, model, posterior_samples, *model_args, **kwargs)
    return _result(obs, y, n, rows, fair, pointwise, bins)


def posterior_predictive_crps(rng_key, n, model, model_args, guide, params, fair=False, pointwise=False, bins=10, slab_bytes=64 << 20, **kwargs):
    """``predictive_crps`` over ``n`` draws from the posterior predictive at ``params``: the scores of the ``obs`` that
    ``posterior_predictive_samples(rng_key, n, model, model_args, guide, params)`` returns for the same key."""
    what = "posterior_predictive_crps"
    fam = _family(model, what)
    U._check_guide(model, guide)
    bins = _bins(bins)
    n = PS._count(n)
    _check_score_draws(n, what)
    rows, d = PS._data(model, model_args, kwargs)
    y = _labels(model, fam, model_args, rows, what)
    IV._check_whole(n, rows, slab_bytes, what)
    obs = PS.posterior_predictive_samples(rng_key, n, model, model_args, guide, params, **kwargs)["obs"]
    return _result(obs, y, n, rows, fair, pointwise, bins)


def compare_scores(a, b):
    """Paired comparison of two ``CRPSResult`` over the same rows, both with ``pointwise=True``: ``ScoreComparison(crps_diff, se_diff)``,
    the mean of the pointwise CRPS of ``a`` minus that of ``b`` and its standard error.  CRPS is a loss: a NEGATIVE ``crps_diff`` favours
    ``a`` (``criteria.compare`` has the other sign, as an elpd is a gain)."""
    for name, r in (("a", a), ("b", b)):
        if not isinstance(r, CRPSResult) or r.pointwise is None:
            raise ValueError(f"compare_scores: {name} must be a CRPSResult with its pointwise arrays (pointwise=True)")
    if a.n_rows != b.n_rows:
        raise ValueError(f"compare_scores: the results cover {a.n_rows} and {b.n_rows} rows; a paired comparison needs the same rows")
    diff = a.pointwise["crps"].to(torch.float64) - b.pointwise["crps"].to(torch.float64)
    return ScoreComparison(*_mean_and_se(diff))

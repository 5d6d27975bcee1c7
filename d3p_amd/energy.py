"""The energy score of multivariate predictive draws against the observed outcomes.

    energy_score_draws(draws, y)                -> {"es", "es_fair", "mae", "spread"}: (rows,) float32
    energy_score(draws, y, fair=False)          -> (rows,) float32
    draws_limit()                               -> d3p_energy_score_max_n()
    posterior_predictive_energy_score(rng_key, n, model, model_args, guide, params, fair=False, pointwise=False, slab_bytes=64 << 20, **kw)
                                                -> EnergyScoreResult
    compare_energy_scores(a, b)                 -> EnergyScoreComparison(es_diff, se_diff), negative favouring a

The energy score (Gneiting & Raftery 2007) is the multivariate CRPS: ``ES = E|X - y| - 1/2 E|X - X'|`` with the Euclidean norm, over
the empirical distribution of a row's draws.  It is proper and in the outcome's own units; at ``d = 1`` it is ``scoring.crps``.

``energy_score_draws`` is the model-free reduction (``d3p_energy_score``, ``d3p_amd/csrc/d3p_energy.hip``): ``draws`` is a 3-D CUDA
float32 or int32 tensor ``(n, rows, d)`` with unit last stride, any row and draw strides that do not overlap -- what
``mixture.posterior_predictive_samples(...)["obs"]`` returns, and the int32 images of ``modelling.sample_multi_posterior_predictive`` for
the VAE; a 2-D ``(n, rows)`` tensor is ``d = 1``.  ``y`` holds ``(rows, d)`` observations (``(rows,)`` at ``d = 1``).  Per row, with
``dist`` the float32 distance rule of the kernel's header widened to float64, ``S1 = sum_i dist(x_i, y)`` and ``S2 = sum_{i != j} dist(x_i,
x_j)``:

    mae = S1 / n        spread = S2 / (2 n^2)        es = mae - spread        es_fair = mae - S2 / (2 n (n - 1))     (NaN at n = 1)

each rounded to float32 once.  A NaN or infinite element among a row's draws or in its ``y`` makes that row's four scores NaN.  int32
draws are converted to float32 on the device, which is exact up to ``2^24`` in magnitude: larger values are a ``ValueError`` (this
one check reads the draws, so it runs on the device, after every other).  For an int32 tensor a float ``y`` with integral values is
cast; ``n <= draws_limit()`` = 65535.

The model layer scores ``GaussianMixtureModel`` with ``GaussianMixtureGuide``; every other model raises ``TypeError`` (the regression
families' outcomes are scalar: ``scoring``).  The draws are exactly the ``obs`` tensor ``mixture.posterior_predictive_samples`` returns
for the same key.  It is written whole and its ``4 n rows d`` bytes must fit ``slab_bytes``.  ``model_args[1]`` (``obs``) is READ here as
the observations and is required.  Every other host check runs before the device is touched; there is no CPU fallback.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import infer_util as U
from . import mixture as MX
from ._lib import check, ptr, stream_ptr
from .models import GaussianMixtureGuide, GaussianMixtureModel
from .scoring import _mean_and_se, _observations

__all__ = ["energy_score_draws", "energy_score", "draws_limit", "posterior_predictive_energy_score", "compare_energy_scores",
           "EnergyScoreResult", "EnergyScoreComparison", "INT_EXACT"]

INT_EXACT = 2 ** 24   # |v| <= 2^24: every int32 the float32 conversion keeps exactly


class EnergyScoreResult(NamedTuple):
    es: torch.Tensor             # 0-d float64: the mean over the rows (of es_fair with fair=True)
    se: torch.Tensor             # its standard error from the pointwise values
    mae: torch.Tensor            # 0-d float64: the mean over the rows
    spread: torch.Tensor         # 0-d float64: the mean over the rows
    n_draws: int
    n_rows: int
    dim: int
    pointwise: Optional[dict]    # None, or {"es", "mae", "spread"}: (rows,) float32


class EnergyScoreComparison(NamedTuple):
    es_diff: torch.Tensor        # 0-d float64: mean energy score of a minus that of b (negative favours a)
    se_diff: torch.Tensor        # its standard error from the paired pointwise differences


def draws_limit():
    """d3p_energy_score_max_n(): the largest draw count the kernel walks (host only: no device is touched)."""
    return int(_lib.load().d3p_energy_score_max_n())


def _check_draws(draws, what):
    """(n, rows, d, ld_draw, ld_row) of the draws tensor after the host checks."""
    if not isinstance(draws, torch.Tensor) or draws.dim() not in (2, 3) or draws.dtype not in (torch.float32, torch.int32):
        raise ValueError(f"{what}: draws: a 3-D float32 or int32 CUDA tensor (draws, rows, d) is required (2-D (draws, rows): d = 1)")
    n, rows = int(draws.shape[0]), int(draws.shape[1])
    d = int(draws.shape[2]) if draws.dim() == 3 else 1
    if n < 1:
        raise ValueError(f"{what}: at least one draw")
    if d < 1:
        raise ValueError(f"{what}: d >= 1 is required")
    most = draws_limit()
    if n > most:
        raise ValueError(f"{what}: {n} draws; one workgroup walks all pairs of a row and runs at most {most} draws (n <= {most})")
    if draws.dim() == 3 and d > 1 and draws.stride(2) != 1:
        raise ValueError(f"{what}: the last axis of draws must have unit stride (rows and draws may be strided)")
    if draws.dim() == 3:
        ld_row = int(draws.stride(1)) if rows > 1 else d
    else:
        ld_row = int(draws.stride(1)) if rows > 1 else 1
    ld_draw = int(draws.stride(0)) if n > 1 else max(rows, 1) * ld_row
    if ld_row < d or ld_draw < rows * ld_row:
        raise ValueError(f"{what}: the rows or the draws of the tensor overlap or are not in (draws, rows, d) order (strides "
                         f"{tuple(draws.stride())})")
    return n, rows, d, ld_draw, ld_row


def _check_y(y, dtype, rows, d, what):
    """y as a (rows * d,) tensor of the draws' dtype on whatever device it lies."""
    shp = tuple(y.shape) if hasattr(y, "shape") else tuple(np.shape(y))
    if shp != (rows, d) and not (d == 1 and shp == (rows,)):
        raise ValueError(f"{what}: y: shape ({rows}, {d}) expected (one observation per row of the draws), got {shp}")
    return _observations(y, dtype, rows * d, what)


def _score(draws, dims, y):
    """The four rows of d3p_energy_score; y a contiguous (rows * d,) tensor of the draws' dtype on their device."""
    n, rows, d, ld_draw, ld_row = dims
    out = torch.empty((4, rows), dtype=torch.float32, device=draws.device)
    if rows:
        check(_lib.load().d3p_energy_score(stream_ptr(), ptr(draws), 0 if draws.dtype == torch.float32 else 1, ld_draw, ld_row, n, rows, d,
                                           ptr(y), d, ptr(out), rows))
    return {"es": out[0], "es_fair": out[1], "mae": out[2], "spread": out[3]}


def _energy_score_draws(draws, y, what):
    dims = _check_draws(draws, what)
    y = _check_y(y, draws.dtype, dims[1], dims[2], what)
    if not draws.is_cuda:
        raise ValueError(f"{what}: draws: a 3-D float32 or int32 CUDA tensor (draws, rows, d) is required (2-D (draws, rows): d = 1)")
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(draws.device):
        y = y.to(draws.device).contiguous()
        if draws.dtype == torch.int32 and draws.numel():
            # the one check that has to read the draws
            if bool(((draws > INT_EXACT) | (draws < -INT_EXACT)).any()) or bool(((y > INT_EXACT) | (y < -INT_EXACT)).any()):
                raise ValueError(f"{what}: int32 values beyond 2^24 in magnitude: the kernel converts to float32, which is exact only up "
                                 "to there (score a float32 tensor instead)")
        return _score(draws, dims, y)


def energy_score_draws(draws, y):
    """Energy score, its fair form, mean distance to ``y`` and spread of every row's draws (module docstring): ``{"es", "es_fair",
    "mae", "spread"}`` as ``(rows,)`` float32 on the draws' device."""
    return _energy_score_draws(draws, y, "energy_score_draws")


def energy_score(draws, y, fair=False):
    """The energy score of every row's draws against ``y``: ``(rows,)`` float32; ``fair=True``: the unbiased-spread form."""
    return _energy_score_draws(draws, y, "energy_score")["es_fair" if fair else "es"]


def posterior_predictive_energy_score(rng_key, n, model, model_args, guide, params, fair=False, pointwise=False, slab_bytes=64 << 20,
                                      **kwargs):
    """The energy score of ``n`` posterior predictive draws of the mixture model at ``params`` against the observations
    ``model_args[1]``: the scores of the ``obs`` that ``mixture.posterior_predictive_samples(rng_key, n, model, model_args, guide,
    params)`` returns for the same key.  ``fair=True`` scores with the unbiased spread; ``pointwise=True`` keeps the per-row arrays."""
    what = "posterior_predictive_energy_score"
    if not isinstance(model, GaussianMixtureModel):
        raise TypeError(f"{what}: unsupported model {type(model).__name__} (GaussianMixtureModel has multivariate outcomes to score; the "
                        "regression families: d3p_amd.scoring)")
    if not isinstance(guide, GaussianMixtureGuide):
        raise TypeError(f"{what}: guide must be a GaussianMixtureGuide, got {type(guide).__name__}")
    if n is None:
        raise ValueError(f"{what}: n must be an int >= 1 (a single draw has no spread to score)")
    n, _ = MX._count(n)
    most = draws_limit()
    if n > most:
        raise ValueError(f"{what}: {n} draws; one workgroup walks all pairs of a row and runs at most {most} draws (n <= {most})")
    args = list(model_args) if isinstance(model_args, (tuple, list)) else []
    obs = args[1] if len(args) > 1 and args[1] is not None else kwargs.get("obs")
    if obs is None:
        raise ValueError(f"{what}: model_args[1] (obs) is required: the draws are scored against it")
    k, rows, d = MX._shape(model, model_args, kwargs)
    y = _check_y(obs, torch.float32, rows, d, what)
    U._check_slab_bytes(slab_bytes)
    need = 4 * n * rows * d
    if need > slab_bytes:
        raise ValueError(f"{what}: the {n} x {rows} x {d} predictive tensor is written whole and needs slab_bytes >= {need}, got "
                         f"{slab_bytes}")
    draws = MX.posterior_predictive_samples(rng_key, n, model, model_args, guide, params, **kwargs)["obs"]
    with torch.cuda.device(draws.device):
        s = _score(draws, (n, rows, d, rows * d, d), y.to(draws.device).contiguous())
        point = s["es_fair" if fair else "es"]
        mean, se = _mean_and_se(point)
        pw = {"es": point, "mae": s["mae"], "spread": s["spread"]} if pointwise else None
        return EnergyScoreResult(mean, se, s["mae"].to(torch.float64).sum() / rows, s["spread"].to(torch.float64).sum() / rows, n, rows, d,
                                 pw)


def compare_energy_scores(a, b):
    """Paired comparison of two ``EnergyScoreResult`` over the same rows, both with ``pointwise=True``: ``EnergyScoreComparison(es_diff,
    se_diff)``, the mean of the pointwise score of ``a`` minus that of ``b`` and its standard error.  The score is a loss: a NEGATIVE
    ``es_diff`` favours ``a``."""
    for name, r in (("a", a), ("b", b)):
        if not isinstance(r, EnergyScoreResult) or r.pointwise is None:
            raise ValueError(f"compare_energy_scores: {name} must be an EnergyScoreResult with its pointwise arrays (pointwise=True)")
    if a.n_rows != b.n_rows or a.dim != b.dim:
        raise ValueError(f"compare_energy_scores: the results cover {a.n_rows} rows of dimension {a.dim} and {b.n_rows} of {b.dim}; a "
                         "paired comparison needs the same rows")
    diff = a.pointwise["es"].to(torch.float64) - b.pointwise["es"].to(torch.float64)
    return EnergyScoreComparison(*_mean_and_se(diff))

"""WAIC, PSIS-LOO and pairwise model comparison for the regression models and the Gaussian mixture model (DESIGN.md sections 4h, 4i).

    waic(model, posterior_samples, *model_args, ddof=1, pointwise=False)                                  -> WAICResult
    posterior_waic(rng_key, n, model, model_args, guide, params, ddof=1, pointwise=False, **kwargs)       -> WAICResult
    loo(model, posterior_samples, *model_args, pointwise=False, slab_bytes=64 << 20)                      -> LOOResult
    posterior_loo(rng_key, n, model, model_args, guide, params, pointwise=False, slab_bytes=64 << 20, **kwargs) -> LOOResult
    compare(a, b)                                                                                         -> ComparisonResult

The Watanabe-Akaike information criterion (Vehtari, Gelman & Gabry 2017, eqs. 11-13 and 23) over ``n`` posterior draws, with
``ll[s, r]`` the UNSCALED pointwise log-likelihood ``d3p_amd.infer_util`` resp. ``d3p_amd.mixture_density`` defines:

    lppd[r]      = logsumexp_s ll[s, r] - log n                       bit-identical to those modules' log_predictive_density
    p_waic[r]    = sum_s (ll[s, r] - mean_s ll[s, r])^2 / (n - ddof)   the between-draw variance: the effective number of parameters
    elpd_waic[r] = lppd[r] - p_waic[r]
    elpd_waic = sum_r elpd_waic[r];  p_waic = sum_r p_waic[r];  waic = -2 elpd_waic;  se = sqrt(rows Var_r elpd_waic[r])

``ddof = 1`` is the paper's and R ``loo``'s sample variance over the draws, ``ddof = 0`` ArviZ's.  Both pointwise arrays come from
one pass of the WAIC forms of ``k_loglik`` / ``k_gmm_density``; the ``n x rows`` matrix is never written.  The totals are 0-d float64
tensors on the device, summed over the rows in float64 with torch; nothing synchronises with the host.

Dispatch by model type.  ``LogisticRegression``, ``LinearRegression``, ``PoissonRegression``: ``model_args = (X, y[, N])`` and
``posterior_samples = {"w"[, "intercept"]}`` as for ``d3p_amd.infer_util``.  ``GaussianMixtureModel``: ``waic(model, {"pis", "mus",
"sigs"}, obs)`` and ``model_args = (k, obs, ...)`` in the posterior form, as for ``d3p_amd.mixture_density``.  The host checks, the
packing (packed samples are read in place) and the posterior forms' key rule are those modules' own.  Every other model raises
``TypeError``.  Every host check runs before the device is touched; there is no CPU fallback.

Special values: a draw with ``ll = -inf`` (a Poisson rate that overflows float32; a mixture draw whose every component is ``-inf``) is
left out of the variance's sums and makes the row's ``p_waic = +inf`` and ``elpd_waic = -inf`` -- ``lppd`` stays finite unless every
draw is ``-inf``.  A NaN makes the row NaN in all three pointwise arrays.  Non-finite rows propagate into the totals.  One row gives a
NaN ``se``.

``compare`` needs both results with ``pointwise=True`` over the same rows: ``elpd_diff = sum_r (a_r - b_r)`` and ``se_diff = sqrt(rows
Var_r (a_r - b_r))`` (sample variance), the paired form of eq. 24.  It is pure torch and runs where the pointwise tensors are.  Two
``WAICResult`` pair their ``elpd_waic``, two ``LOOResult`` their ``elpd_loo``; one of each is refused.

PSIS-LOO (the paper's section 2.1; Pareto-smoothed importance sampling of the leave-one-out predictive densities) over the same
``ll``: ``d3p_psis_loo`` (include/d3p_hip.h states the steps) gives per row ``elpd_loo[r]``, ``lppd[r]`` and the Pareto shape
``pareto_k[r]`` of the row's importance ratios, the diagnostic WAIC lacks: where ``k > k_threshold = min(1 - 1 / log10(n), 0.7)`` the
row's estimate is not to be trusted (``n_high_k`` counts those rows; ``+inf`` -- no fit: fewer than 5 tail draws, a ``-inf`` draw --
and NaN count as high).  ``p_loo[r] = lppd[r] - elpd_loo[r]``, ``looic = -2 elpd_loo``, totals and ``se`` as for WAIC.  Unlike WAIC
this reduction needs the column's order statistics, so the ``n x rows`` matrix IS written -- in row slabs: the rows are taken in
chunks of ``max(128, (slab_bytes // (4 n)) // 128 * 128)``, each chunk written by the rows entry (``d3p_loglik_rows`` /
``d3p_gmm_loglik_rows`` on offset views of the data) into one reused buffer and consumed by ``d3p_psis_loo`` on the same stream; the
latents are packed once.  The result does not depend on ``slab_bytes``.  ``n <= 65535``.  Special values: a ``-inf`` draw makes the
row's ``elpd_loo = -inf`` and ``pareto_k = +inf``; a NaN makes the row NaN.
"""
import math
from typing import NamedTuple, Optional

import torch

from . import infer_util as U
from . import mixture_density as MD
from .models import GaussianMixtureModel

__all__ = ["waic", "posterior_waic", "compare", "WAICResult", "ComparisonResult"]
# (loo, posterior_loo and LOOResult are public as well: the package exports them as d3p_amd.loo, d3p_amd.posterior_loo, d3p_amd.LOOResult)


class WAICResult(NamedTuple):
    elpd_waic: torch.Tensor      # 0-d float64
    p_waic: torch.Tensor         # 0-d float64
    waic: torch.Tensor           # -2 elpd_waic
    se: torch.Tensor             # standard error of elpd_waic
    n_draws: int
    n_rows: int
    pointwise: Optional[dict]    # None, or {"lppd", "p_waic", "elpd_waic"}: (rows,) float32


class LOOResult(NamedTuple):
    elpd_loo: torch.Tensor       # 0-d float64
    p_loo: torch.Tensor          # 0-d float64: sum_r (lppd[r] - elpd_loo[r])
    looic: torch.Tensor          # -2 elpd_loo
    se: torch.Tensor             # standard error of elpd_loo
    n_draws: int
    n_rows: int
    k_threshold: float           # min(1 - 1 / log10(n_draws), 0.7)
    n_high_k: torch.Tensor       # 0-d int64: rows with pareto_k > k_threshold (NaN and +inf count)
    pointwise: Optional[dict]    # None, or {"elpd_loo", "p_loo", "lppd", "pareto_k"}: (rows,) float32


class ComparisonResult(NamedTuple):
    elpd_diff: torch.Tensor      # 0-d float64: elpd (elpd_waic resp. elpd_loo) of a minus that of b
    se_diff: torch.Tensor        # its standard error from the paired pointwise differences


def _total_and_se(x):
    """(sum_r x[r], sqrt(rows Var_r x[r])) in float64, the sample variance; one row: NaN (0 / 0)."""
    x = x.to(torch.float64)
    rows = x.shape[0]
    total = x.sum()
    dev = x - total / rows if rows else x
    return total, torch.sqrt(rows * ((dev * dev).sum() / (rows - 1)))


def _result(lppd, pw, n, pointwise):
    elpd = lppd - pw
    total, se = _total_and_se(elpd)
    keep = {"lppd": lppd, "p_waic": pw, "elpd_waic": elpd} if pointwise else None
    return WAICResult(total, pw.to(torch.float64).sum(), -2.0 * total, se, int(n), int(lppd.shape[0]), keep)


def _is_mixture(model, what):
    if isinstance(model, GaussianMixtureModel):
        return True
    try:
        U._family(model)
    except TypeError:
        raise TypeError(f"{what}: unsupported model {type(model).__name__} (LogisticRegression, LinearRegression, PoissonRegression "
                        "and GaussianMixtureModel have a WAIC and a PSIS-LOO here)") from None
    return False


def _ddof(ddof):
    if ddof is None:
        raise ValueError("ddof must be 0 or 1, got None")
    U._check_ddof(2, ddof)   # (the value alone; n > ddof is checked where n is known)
    return int(ddof)


def waic(model, posterior_samples, *model_args, ddof=1, pointwise=False):
    """WAIC of ``model`` on ``model_args``' data over the given posterior draws (module docstring)."""
    mixture = _is_mixture(model, "waic")
    ddof = _ddof(ddof)
    if mixture:
        obs = model_args[0] if model_args else None
        lppd, pw = MD._from_samples(model, posterior_samples, obs, False, True, False, waic_ddof=ddof)
        n = MD.MX._shape_of(posterior_samples["pis"])[0]
    else:
        (lppd, pw), single, _, _ = U._over_samples(True, model, posterior_samples, model_args, waic_ddof=ddof)
        n = 1 if single else MD.MX._shape_of(posterior_samples["w"])[0]
    return _result(lppd, pw, n, pointwise)


def posterior_waic(rng_key, n, model, model_args, guide, params, ddof=1, pointwise=False, **kwargs):
    """``waic`` over ``n`` draws from the guide at ``params``, drawn on the device on the key rule of the model's
    ``posterior_log_predictive_density`` (``d3p_amd.infer_util`` / ``d3p_amd.mixture_density``) and consumed there: with the same key
    and ``n`` the draws are the ones ``sample_multi_posterior_predictive`` resp. ``mixture.posterior_predictive_samples`` returns."""
    mixture = _is_mixture(model, "posterior_waic")
    ddof = _ddof(ddof)
    if mixture:
        lppd, pw = MD._posterior(rng_key, n, model, model_args, guide, params, kwargs, True, False, waic_ddof=ddof)
    else:
        lppd, pw = U._posterior(rng_key, n, model, model_args, guide, params, waic_ddof=ddof)
    return _result(lppd, pw, int(n), pointwise)


def _k_threshold(n):
    """min(1 - 1 / log10(n), 0.7): the Pareto shape above which n draws do not give a reliable estimate (n = 1: -inf)."""
    return min(1.0 - 1.0 / math.log10(n), 0.7) if n > 1 else -math.inf


def _loo_result(elpd, lppd, khat, n, pointwise):
    p = lppd - elpd
    total, se = _total_and_se(elpd)
    thr = _k_threshold(int(n))
    high = torch.logical_not(khat <= thr).sum()
    keep = {"elpd_loo": elpd, "p_loo": p, "lppd": lppd, "pareto_k": khat} if pointwise else None
    return LOOResult(total, _total_and_se(p)[0], -2.0 * total, se, int(n), int(elpd.shape[0]), thr, high, keep)


def _slab_bytes(slab_bytes):
    U._check_slab_bytes(slab_bytes)   # (n <= 65535 is checked where n is known)
    return slab_bytes


def loo(model, posterior_samples, *model_args, pointwise=False, slab_bytes=64 << 20):
    """PSIS-LOO of ``model`` on ``model_args``' data over the given posterior draws (module docstring)."""
    mixture = _is_mixture(model, "loo")
    slab_bytes = _slab_bytes(slab_bytes)
    if mixture:
        obs = model_args[0] if model_args else None
        elpd, lppd, khat = MD._from_samples(model, posterior_samples, obs, False, True, False, loo_slab_bytes=slab_bytes)
        n = MD.MX._shape_of(posterior_samples["pis"])[0]
    else:
        (elpd, lppd, khat), single, _, _ = U._over_samples(True, model, posterior_samples, model_args, loo_slab_bytes=slab_bytes)
        n = 1 if single else MD.MX._shape_of(posterior_samples["w"])[0]
    return _loo_result(elpd, lppd, khat, n, pointwise)


def posterior_loo(rng_key, n, model, model_args, guide, params, pointwise=False, slab_bytes=64 << 20, **kwargs):
    """``loo`` over ``n`` draws from the guide at ``params``, drawn on the device on ``posterior_waic``'s key rule: with the same key
    and ``n`` the draws are the ones ``sample_multi_posterior_predictive`` resp. ``mixture.posterior_predictive_samples`` returns."""
    mixture = _is_mixture(model, "posterior_loo")
    slab_bytes = _slab_bytes(slab_bytes)
    if mixture:
        elpd, lppd, khat = MD._posterior(rng_key, n, model, model_args, guide, params, kwargs, True, False, loo_slab_bytes=slab_bytes)
    else:
        elpd, lppd, khat = U._posterior(rng_key, n, model, model_args, guide, params, loo_slab_bytes=slab_bytes)
    return _loo_result(elpd, lppd, khat, int(n), pointwise)


def compare(a, b):
    """Paired comparison of two ``WAICResult`` or of two ``LOOResult`` over the same rows, both with ``pointwise=True``:
    ``ComparisonResult(elpd_diff, se_diff)``, positive ``elpd_diff`` favouring ``a``."""
    for name, r in (("a", a), ("b", b)):
        if not isinstance(r, (WAICResult, LOOResult)) or r.pointwise is None:
            raise ValueError(f"compare: {name} must be a WAICResult or a LOOResult with its pointwise arrays (pointwise=True)")
    if type(a) is not type(b):
        raise ValueError(f"compare: a {type(a).__name__} and a {type(b).__name__} estimate different quantities; compare two of a kind")
    if a.n_rows != b.n_rows:
        raise ValueError(f"compare: the results cover {a.n_rows} and {b.n_rows} rows; a paired comparison needs the same rows")
    site = "elpd_waic" if isinstance(a, WAICResult) else "elpd_loo"
    diff = a.pointwise[site].to(torch.float64) - b.pointwise[site].to(torch.float64)
    return ComparisonResult(*_total_and_se(diff))

"""Whole-table log joint, ELBO and the PSIS Pareto-k diagnostic of a variational guide for the regression models (DESIGN.md
section 4j): is the guide ``DPSVI`` trained a usable approximation of the posterior?  (Yao, Vehtari, Simpson & Gelman 2018, "Yes,
but did it work?  Evaluating variational inference".)

    log_likelihood_total(model, posterior_samples, *model_args)                     -> (n,) float64   sum_r ll[s, r]
    log_joint(model, posterior_samples, *model_args)                                -> (n,) float64   + log prior of draw s
    guide_diagnostic(rng_key, n, model, model_args, guide, params, pointwise=False) -> GuideDiagnostic

With ``ll[s, r] = log p(y_r | x_r, w_s, intercept_s)`` the UNSCALED float32 pointwise log-likelihood of ``d3p_amd.infer_util`` (bit for
bit the values ``log_likelihood`` returns) and theta_s = [w_s | intercept_s] the D = d (+ 1) latents of draw s:

    log_likelihood_total[s] = sum_{r < rows} ll[s, r]                  float64 additions of the float32 values in the fixed order
                                                                       include/d3p_hip.h states (d3p_loglik_draw_sums); no n x rows matrix
    log p(theta_s) = - sum_k w_sk^2 / (2 prior_scale^2) - d (log prior_scale + log(2 pi) / 2)
                     [ - intercept_s^2 / (2 intercept_prior_scale^2) - (log intercept_prior_scale + log(2 pi) / 2) ]
    log_joint[s]   = log_likelihood_total[s] + log p(theta_s)          numpyro's log_density of the whole table at draw s
    log q(theta_s) = - sum_j z_sj^2 / 2 - sum_j log sigma_j - D log(2 pi) / 2,   z_sj = (theta_sj - loc_j) / sigma_j
    log r_s        = log_joint[s] - log q(theta_s)                     the log importance ratio of draw s

The prior and the guide density are computed per draw in float64 from the float32 latents and parameters (O(n D) torch arithmetic on
the device).  The guide is a diagonal normal: ``sigma = auto_scale`` itself for ``AutoDiagonalNormal``, ``sigma = exp(*_std_log)``, the
float64 exponential of the float32 parameter, for ``DiagonalNormalGuide`` and ``MeanFieldGuide``; loc and sigma follow the latent
columns [w | intercept].

This is the log joint of the WHOLE table, not a subsample estimate: ``model_args = (X, y[, N])`` and an ``N`` that is given must equal
the number of rows (``ValueError``).  ``LogisticRegression``, ``LinearRegression`` and ``PoissonRegression`` are accepted; every other
model raises ``TypeError``.  Dispatch, data checks, sample shapes, packing (packed samples are read in place), guide checks and the
key rule are ``d3p_amd.infer_util``'s own: with the same key and ``n``, ``guide_diagnostic`` uses the draws
``sample_multi_posterior_predictive`` returns.  A single sample (``w`` of shape ``(d,)``) returns a 0-d tensor.  Every host check runs
before the device is touched; there is no CPU fallback; nothing synchronises with the host.

``GuideDiagnostic`` over the n ratios (totals are 0-d float64 tensors on the device):

    elbo            = mean_s log r_s                       the full-data ELBO estimate
    elbo_se         = sqrt(Var_s log r_s / n)              sample variance; one draw: NaN
    log_evidence_is = logsumexp_s log r_s - log n          the importance-sampling estimate of log p(y | X): >= elbo (Jensen), equal to
                                                           it when every ratio is equal
    pareto_k        = the Pareto shape of the ratios' upper tail, from d3p_psis_loo (include/d3p_hip.h) on one column
    k_threshold     = min(1 - 1 / log10(n), 0.7)           (d3p_amd.criteria): above it the ratios' tail is too heavy for n draws
    ess             = (sum_s r_s)^2 / sum_s r_s^2          of the raw ratios, r_s = exp(log r_s - max_s log r_s)

``log r_s`` spans hundreds of thousands on a large table and cannot go to float32 as it is.  ``d3p_psis_loo`` takes a column ``ll``
and fits the tail of ``x = min ll - ll``; it is handed ``ll_s = float32(max_s log r_s - log r_s)``, which is >= 0 and 0 at the largest
ratio, so that its ``x_s = -ll_s`` are exactly the ratios shifted to a maximum of 0 (a matrix of one row at a leading dimension of
1; the elpd and lppd outputs of that call are discarded).  The rounding is harmless there: its absolute error is below 2^-24 |x|, the
fitted tail sits near 0 and a far draw carries weight exp(x).  ``n <= 65535`` as for PSIS-LOO (``ValueError``).  ``n <= 20`` leaves no
tail of 5 draws and ``pareto_k = +inf``.  EVERY RATIO EQUAL (max == min in float64, n >= 2: the guide is the posterior): there is no
tail either and ``d3p_psis_loo`` would say ``+inf``; ``pareto_k = -inf`` is reported instead (the lightest tail there is).  A NaN ratio
makes every total NaN.  A ``-inf`` ratio (a Poisson rate that overflows float32) gives ``elbo = -inf`` and ``pareto_k = +inf``;
``log_evidence_is`` stays finite unless every ratio is ``-inf``.

``pointwise=True`` keeps ``{"log_ratio", "log_joint", "log_q", "log_likelihood"}``, each ``(n,)`` float64.
"""
import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import _lib
from . import infer_util as U
from . import modelling as M
from ._lib import check, ptr, stream_ptr
from .models import AutoDiagonalNormal, MeanFieldGuide

__all__ = ["log_likelihood_total", "log_joint", "guide_diagnostic", "GuideDiagnostic"]

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_SUPPORTED = "LogisticRegression, LinearRegression and PoissonRegression"


class GuideDiagnostic(NamedTuple):
    elbo: torch.Tensor              # 0-d float64
    elbo_se: torch.Tensor           # 0-d float64
    log_evidence_is: torch.Tensor   # 0-d float64
    pareto_k: torch.Tensor          # 0-d float64
    k_threshold: float              # min(1 - 1 / log10(n_draws), 0.7)
    ess: torch.Tensor               # 0-d float64
    n_draws: int
    n_rows: int
    pointwise: Optional[dict]       # None, or {"log_ratio", "log_joint", "log_q", "log_likelihood"}: (n,) float64


def _family(model, what):
    try:
        return U._family(model)
    except TypeError:
        raise TypeError(f"{what}: unsupported model {type(model).__name__} ({_SUPPORTED} have a whole-table log joint here)") from None


def _table(model, model_args):
    """(rows, d) after infer_util's data checks; an N that is given must be the row count (the whole table, no subsample estimate)."""
    rows, d = U._data(model, model_args)
    total = model_args[2] if len(model_args) >= 3 else None
    if total is not None and int(total) != rows:
        raise ValueError(f"num_obs_total = {total} differs from the {rows} rows: this is the log joint of the whole table, not a subsample "
                         "estimate")
    return rows, d


def _draw_sums(model, fam, model_args, rows, d, n, latent):
    """(n,) float64: d3p_loglik_draw_sums over latent = (tensor at the first latent row, ld, w_off, b_col)."""
    first, ld, w_off, b_col = latent
    lib = _lib.load()
    X = M._f32(model_args[0], "X")
    y = M._f32(model_args[1], "y").reshape(rows)
    out = torch.empty((n,), dtype=torch.float64, device=X.device)
    nbytes = int(lib.d3p_loglik_draw_sums_workspace(rows, n))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=X.device)
    ms = U._model_struct(model, fam, d)
    check(lib.d3p_loglik_draw_sums(stream_ptr(), C.byref(ms), ptr(X), ptr(y), rows, ptr(first), ld, w_off, b_col, n, ptr(out), ptr(ws), nbytes))
    return out


def _columns(latent, n, d):
    """(w (n, d), intercept (n,) or None) float64 copies of the latent buffer's columns."""
    first, ld, w_off, b_col = latent
    base = first.storage_offset()
    w = torch.as_strided(first, (n, d), (ld, 1), base + w_off).to(torch.float64)
    b = None if b_col < 0 else torch.as_strided(first, (n,), (ld,), base + b_col).to(torch.float64)
    return w, b


def _log_prior(model, w, b):
    d = w.shape[1]
    lp = (w * w).sum(1) / (-2.0 * model.prior_scale ** 2) - d * (math.log(model.prior_scale) + _HALF_LOG_2PI)
    if b is not None:
        lp = lp + (b * b) / (-2.0 * model.intercept_prior_scale ** 2) - (math.log(model.intercept_prior_scale) + _HALF_LOG_2PI)
    return lp


def _guide_loc_sigma(guide, gparams):
    """(loc, sigma) float64 (D,) in the order of the latent columns [w | intercept]."""
    gp = {name: M._f32(v, f"params['{name}']").reshape(-1).to(torch.float64) for name, v in gparams}
    if isinstance(guide, MeanFieldGuide):
        return torch.cat([gp["w_loc"], gp["intercept_loc"]]), torch.exp(torch.cat([gp["w_std_log"], gp["intercept_std_log"]]))
    if isinstance(guide, AutoDiagonalNormal):
        return gp["auto_loc"], gp["auto_scale"]
    return gp[guide.site + "_loc"], torch.exp(gp[guide.site + "_std_log"])


def _log_q(theta, loc, sigma):
    z = (theta - loc) / sigma
    return (z * z).sum(1) * -0.5 - torch.log(sigma).sum() - theta.shape[1] * _HALF_LOG_2PI


def _from_samples(what, joint, model, posterior_samples, model_args):
    fam = _family(model, what)
    rows, d = _table(model, model_args)
    n, single = U._sample_shape(model, posterior_samples, d)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(M._device()):
        latent = U._pack(model, posterior_samples, n, d)
        out = _draw_sums(model, fam, model_args, rows, d, n, latent)
        if joint:
            out = out + _log_prior(model, *_columns(latent, n, d))
    return out[0] if single else out


def log_likelihood_total(model, posterior_samples, *model_args, **kwargs):
    """``(n,)`` float64: ``[s] = sum_r log p(y_r | x_r, sample s)`` over the whole table, the row sums of ``log_likelihood``'s matrix
    without that matrix (module docstring).  ``model_args`` and ``posterior_samples`` as for ``d3p_amd.infer_util.log_likelihood``."""
    return _from_samples("log_likelihood_total", False, model, posterior_samples, model_args)


def log_joint(model, posterior_samples, *model_args, **kwargs):
    """``(n,)`` float64: ``log_likelihood_total`` plus the log prior density of draw s -- numpyro's ``log_density`` of the model on
    the whole table at each draw (module docstring)."""
    return _from_samples("log_joint", True, model, posterior_samples, model_args)


def _pareto_k(lr, mx, mn, n):
    """The Pareto shape of the ratios exp(lr) as a 0-d float64 tensor (module docstring)."""
    col = (mx - lr).to(torch.float32).contiguous()
    out = torch.empty((3,), dtype=torch.float32, device=lr.device)
    check(_lib.load().d3p_psis_loo(stream_ptr(), ptr(col), 1, n, 1, ptr(out[0:]), ptr(out[1:]), ptr(out[2:])))
    k = out[2].to(torch.float64)
    inf = torch.full_like(k, math.inf)
    k = torch.where(torch.isneginf(lr).any(), inf, k)                    # (the kernel saw +inf, or NaN where every ratio is -inf)
    if n >= 2:
        k = torch.where((mx == mn) & torch.isfinite(mx), -inf, k)        # every ratio equal: the guide is the posterior
    return torch.where(torch.isnan(lr).any(), torch.full_like(k, math.nan), k)


def guide_diagnostic(rng_key, n, model, model_args, guide, params, pointwise=False):
    """ELBO, importance-sampling evidence and the Pareto k of ``n`` draws from the guide at ``params`` (as ``DPSVI.get_params``
    returns them) on the whole table ``model_args = (X, y[, N])``: a ``GuideDiagnostic`` (module docstring).  ``rng_key`` is a threefry
    (jax) key as for ``d3p_amd.modelling``; the draws follow ``sample_multi_posterior_predictive``'s key rule."""
    from .criteria import _k_threshold
    fam = _family(model, "guide_diagnostic")
    U._check_guide(model, guide)
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    if n > 65535:
        raise ValueError(f"{n} draws: the Pareto fit (d3p_psis_loo) runs at most 65535 draws (n <= 65535)")
    rows, d = _table(model, model_args)
    if not isinstance(params, dict):
        raise ValueError("params: the dict DPSVI.get_params returns is required")
    gparams = [(name, M._param(params, name, size)) for name, size in M._guide_param_names(guide, model, d)]
    key = M._check_key(rng_key)
    _lib.require_device()
    dev = key.device
    with torch.cuda.device(dev):
        latent = U._guide_latents(key, n, model, guide, gparams, d, rows, dev)
        ll = _draw_sums(model, fam, model_args, rows, d, n, latent)
        w, b = _columns(latent, n, d)
        lj = ll + _log_prior(model, w, b)
        theta = w if b is None else torch.cat([w, b.reshape(n, 1)], dim=1)
        lq = _log_q(theta, *_guide_loc_sigma(guide, gparams))
        lr = lj - lq
        elbo = lr.sum() / n
        dev_ = lr - elbo
        se = torch.sqrt((dev_ * dev_).sum() / (n - 1) / n)               # (one draw: 0 / 0 = NaN)
        mx, mn = lr.max(), lr.min()
        r = torch.exp(lr - mx)
        ess = r.sum() ** 2 / (r * r).sum()
        lis = torch.logsumexp(lr, 0) - math.log(n)
        k = _pareto_k(lr, mx, mn, n)
    keep = {"log_ratio": lr, "log_joint": lj, "log_q": lq, "log_likelihood": ll} if pointwise else None
    return GuideDiagnostic(elbo, se, lis, k, _k_threshold(n), ess, n, rows, keep)

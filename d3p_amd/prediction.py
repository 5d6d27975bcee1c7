"""Posterior predictive mean and variance of the regression models: a prediction for a new row, with its uncertainty.

    predictive_moments(model, posterior_samples, X[, y[, N]])                  -> {"mean": (rows,), "variance": (rows,)}
    posterior_predictive_moments(key, n, model, (X[, y[, N]]), guide, params)  -> the same over n draws from the guide

The moments of ``obs`` under the mixture ``(1/n) sum_s p(y | x_r, w_s, intercept_s)``, from the families' closed-form conditional
moments -- no outcome is sampled, so the result carries no Monte-Carlo noise beyond that of the ``n`` latent draws:

    t[s, r]  = X[r] . w_s (+ intercept_s)
    mu[s, r] = sigmoid(t)   | t        | exp(t)          (LogisticRegression | LinearRegression | PoissonRegression)
    v[s, r]  = mu (1 - mu)  | sigma^2  | mu
    mean[r]     = (1/n) sum_s mu[s, r]
    variance[r] = (1/n) sum_s v[s, r] + (1/n) sum_s (mu[s, r] - mean[r])^2      (law of total variance; population form, 1/n)

float32 links without clamps, float64 accumulation, one rounding to float32.  A NaN linear predictor makes its row NaN; otherwise a
Poisson rate ``exp(t)`` that overflows float32 in any draw makes the row ``(+inf, +inf)``, never NaN.

The work runs in ``d3p_amd/csrc/d3p_moments.hip``: the draws x rows product on the matrix cores with the
moments as its epilogue; the ``n x rows`` matrix is never written.  Every other model raises ``TypeError``.  There is no CPU fallback.
"""
import ctypes as C

import torch

from . import _lib
from . import modelling as M
from ._lib import check, ptr, stream_ptr
from .infer_util import _FAMILY, _check_guide, _guide_latents, _model_struct, _pack, _sample_shape

__all__ = ["predictive_moments", "posterior_predictive_moments"]


def _family(model):
    fam = _FAMILY.get(type(model))
    if fam is None:
        raise TypeError(f"predictive_moments: unsupported model {type(model).__name__} (LogisticRegression, LinearRegression and "
                        "PoissonRegression have closed-form moments over a linear predictor)")
    return fam


def _data(model, model_args):
    """(rows, d) of model_args = (X[, y[, N]]) after the host checks; the labels and N are accepted and not read."""
    if len(model_args) < 1 or model_args[0] is None:
        raise ValueError(f"{type(model).__name__}: model_args = (X[, y[, N]]) with X of shape (rows, d)")
    rows, d = M._rows_of(model_args[0], "X")
    if model.d is not None and int(model.d) != d:
        raise ValueError(f"X has {d} columns, the model {model.d}")
    if rows < 1 or d < 1:
        raise ValueError("X: at least one row and one column")
    return rows, d


def _launch(model, fam, X, rows, d, n, latent):
    """latent = (tensor at the first latent row, ld, w_off, b_col); returns the two (rows,) float32 tensors on the current GPU."""
    first, ld, w_off, b_col = latent
    X = M._f32(X, "X")
    mean = torch.empty((rows,), dtype=torch.float32, device=X.device)
    var = torch.empty((rows,), dtype=torch.float32, device=X.device)
    ms = _model_struct(model, fam, d)
    check(_lib.load().d3p_predict_moments(stream_ptr(), C.byref(ms), ptr(X), rows, ptr(first), ld, w_off, b_col, n, ptr(mean), ptr(var)))
    return {"mean": mean, "variance": var}


def predictive_moments(model, posterior_samples, *model_args, **kwargs):
    """Mean and variance of the posterior predictive of ``obs`` over given samples: ``{"mean": (rows,), "variance": (rows,)}``
    float32 on the GPU, the variance by the law of total variance in its population form (module docstring).

    ``model_args = (X[, y[, N]])``, the models' call signature; ``y`` and ``N`` are accepted and not read.
    ``posterior_samples = {"w": (n, d)[, "intercept": (n,) or (n, 1)]}`` as torch tensors or numpy arrays (what
    ``sample_multi_posterior_predictive`` returns is read in place).  A single sample (``w`` of shape ``(d,)``) is ``n = 1``: the
    mean is ``mu`` and the variance ``v``."""
    fam = _family(model)
    rows, d = _data(model, model_args)
    n, _ = _sample_shape(model, posterior_samples, d)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(M._device()):
        return _launch(model, fam, model_args[0], rows, d, n, _pack(model, posterior_samples, n, d))


def posterior_predictive_moments(rng_key, n, model, model_args, guide, params, **kwargs):
    """``predictive_moments`` over ``n`` draws from the guide at ``params`` (as ``DPSVI.get_params`` returns them), drawn on the
    device and consumed there.  ``model_args = (X[, y[, N]])``; ``rng_key`` is a threefry (jax) key as for ``d3p_amd.modelling``.
    The draws follow ``sample_multi_posterior_predictive``'s key rule (draw i on ``split(rng_key, n)[i]``, the guide's chain, site
    key 0 onwards): with the same key and ``n`` the latents are the ones that function returns, whatever the family.  Guides:
    ``AutoDiagonalNormal``, ``DiagonalNormalGuide``; ``MeanFieldGuide`` for logistic regression."""
    fam = _family(model)
    _check_guide(model, guide)
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    rows, d = _data(model, model_args)
    if not isinstance(params, dict):
        raise ValueError("params: the dict DPSVI.get_params returns is required")
    gparams = [(name, M._param(params, name, size)) for name, size in M._guide_param_names(guide, model, d)]
    key = M._check_key(rng_key)
    _lib.require_device()
    dev = key.device
    with torch.cuda.device(dev):
        latent = _guide_latents(key, n, model, guide, gparams, d, rows, dev)
        return _launch(model, fam, model_args[0], rows, d, n, latent)

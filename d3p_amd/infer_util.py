"""Pointwise log-likelihoods and log predictive densities of the regression models: the part of ``numpyro.infer.util`` a DP-VI
user needs to evaluate what ``DPSVI`` trained.

    log_likelihood(model, posterior_samples, X, y[, N])            -> {"obs": (n, rows)}     numpyro.infer.util.log_likelihood
    log_predictive_density(model, posterior_samples, X, y[, N])    -> (rows,)   log (1/n) sum_s p(y_r | x_r, sample s)
    posterior_log_predictive_density(key, n, model, (X, y), guide, params) -> (rows,)   the same over n draws from the guide

All values are UNSCALED log-probabilities ``log p(y_r | x_r, w_s, intercept_s)``: no plate factor (the total count ``N`` of the
models' call signature is accepted and not used) and no observation scale -- numpyro's ``log_likelihood`` returns
``fn.log_prob(value)`` of the observed site.  float32, no clamps: a Poisson rate ``exp(t)`` that overflows gives ``-inf`` as in
float32 jax; the density forms treat such a draw as probability 0 and return ``-inf`` only where every draw is.

The work runs in ``d3p_amd/csrc/d3p_loglik.hip``: the draws x rows product on the matrix cores with the
likelihood as its epilogue; the density forms never write the ``n x rows`` matrix.  ``LogisticRegression``, ``LinearRegression``
and ``PoissonRegression`` are accepted; every other model raises ``TypeError``.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import modelling as M
from ._lib import check, ptr, stream_ptr
from .models import (AutoDiagonalNormal, DiagonalNormalGuide, LinearRegression, LogisticRegression, MeanFieldGuide,
                     PoissonRegression)

__all__ = ["log_likelihood", "log_predictive_density", "posterior_log_predictive_density"]

_FAMILY = {LogisticRegression: _lib.D3P_FAMILY_LOGREG, LinearRegression: _lib.D3P_FAMILY_LINREG,
           PoissonRegression: _lib.D3P_FAMILY_POISSON}


def _family(model):
    fam = _FAMILY.get(type(model))
    if fam is None:
        raise TypeError(f"log_likelihood: unsupported model {type(model).__name__} (LogisticRegression, LinearRegression and "
                        "PoissonRegression have a per-row likelihood over a linear predictor)")
    return fam


def _obs_site(model, d, rows):
    """The observed site's name: the one modelling._model_sites gives the regression layout."""
    return M._model_sites(LogisticRegression(d, intercept=model.intercept), d, rows)[-1][0]


def _data(model, model_args):
    """(rows, d) of model_args = (X, y[, N]) after the host checks; N does not enter an unscaled log-probability."""
    if len(model_args) < 1 or model_args[0] is None:
        raise ValueError(f"{type(model).__name__}: model_args = (X, y[, N]) with X of shape (rows, d)")
    rows, d = M._rows_of(model_args[0], "X")
    if model.d is not None and int(model.d) != d:
        raise ValueError(f"X has {d} columns, the model {model.d}")
    if rows < 1 or d < 1:
        raise ValueError("X: at least one row and one column")
    y = model_args[1] if len(model_args) >= 2 else None
    if y is None:
        raise ValueError("y is missing: model_args = (X, y[, N]); a log-likelihood needs the observed labels")
    if M._numel(y) != rows:
        raise ValueError(f"y: {rows} labels expected (one per row of X), got {M._numel(y)}")
    if isinstance(model, PoissonRegression):
        model.check_labels(y)
    return rows, d


def _sample_shape(model, samples, d):
    """(n, single) of posterior_samples = {"w": (n, d) or (d,)[, "intercept": (n,), (n, 1) or a scalar]}."""
    if not isinstance(samples, dict) or "w" not in samples:
        raise ValueError("posterior_samples: 'w' is missing")
    w = samples["w"]
    shp = tuple(w.shape) if hasattr(w, "shape") else tuple(np.shape(w))
    if len(shp) == 1 and shp[0] == d:
        n, single = 1, True
    elif len(shp) == 2 and shp[1] == d and shp[0] >= 1:
        n, single = shp[0], False
    else:
        raise ValueError(f"posterior_samples['w']: shape (n, {d}) or ({d},) expected, got {shp}")
    if model.intercept:
        if "intercept" not in samples:
            raise ValueError("posterior_samples: 'intercept' is missing (the model has an intercept)")
        if M._numel(samples["intercept"]) != n:
            raise ValueError(f"posterior_samples['intercept']: {n} values expected (one per sample), got {M._numel(samples['intercept'])}")
    return n, single


def _packed_view(w, b, n, d):
    """(buffer tensor whose data_ptr is the first latent row, ld, w_off, b_col) when w (n, d) and b (n,) or None already are
    columns of one row-major float32 buffer on the current GPU -- as sample_multi_posterior_predictive returns them -- else None."""
    ts = [w] + ([b] if b is not None else [])
    dev = M._device()
    if not all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == dev for t in ts):
        return None
    if w.stride(1) != 1 and d > 1:
        return None
    ld = w.stride(0) if n > 1 else None
    o_w = w.storage_offset()
    if b is None:
        if ld is not None and ld < d:
            return None
        return w, (ld or d), 0, -1
    if b.untyped_storage().data_ptr() != w.untyped_storage().data_ptr():
        return None
    if n > 1 and b.stride(0) != ld:
        return None
    o_b = b.storage_offset()
    base = min(o_w, o_b)
    w_off, b_col = o_w - base, o_b - base
    if ld is None:
        ld = max(w_off + d, b_col + 1)
    if w_off + d > ld or b_col >= ld or w_off <= b_col < w_off + d:
        return None
    first = w if base == o_w else b
    return first, ld, w_off, b_col


def _pack(model, samples, n, d):
    """The (n, D) latent buffer [w | intercept] of the kernels: a view when the samples already are one, else one copy."""
    w = samples["w"]
    b = samples["intercept"] if model.intercept else None
    if isinstance(w, torch.Tensor) and (b is None or isinstance(b, torch.Tensor)):
        view = _packed_view(w.detach().reshape(n, d), None if b is None else b.detach().reshape(n), n, d)
        if view is not None:
            return view
    D = d + int(model.intercept)
    buf = torch.empty((n, D), dtype=torch.float32, device=M._device())
    buf[:, :d] = M._f32(w, "posterior_samples['w']").reshape(n, d)
    if b is not None:
        buf[:, d] = M._f32(b, "posterior_samples['intercept']").reshape(n)
    return buf, D, 0, (d if model.intercept else -1)


def _model_struct(model, fam, d):
    """d3p_logreg_model for the log-likelihood entries: family, intercept and lik_sigma are read; the scales stay 1 (unscaled)."""
    return _lib.LogregModel(d, int(model.intercept), model.prior_scale, model.intercept_prior_scale, 1.0, 1.0, fam,
                            _lib.D3P_GUIDE_SOFTPLUS, float(getattr(model, "obs_scale", 0.0)) if fam == _lib.D3P_FAMILY_LINREG else 0.0)


def _check_slab_bytes(slab_bytes):
    if isinstance(slab_bytes, bool) or not isinstance(slab_bytes, int) or slab_bytes < 1:
        raise ValueError(f"slab_bytes must be an int >= 1, got {slab_bytes!r}")


def _loo_chunk(n, slab_bytes):
    """Rows per slab of the PSIS-LOO forms (slab_bytes None: not one): max(128, a multiple of 128 whose n x chunk float32 matrix fits
    slab_bytes).  Host checks only: slab_bytes an int >= 1 and n <= 65535 (d3p_psis_loo's limit)."""
    if slab_bytes is None:
        return None
    _check_slab_bytes(slab_bytes)
    if n > 65535:
        raise ValueError(f"{n} posterior draws: PSIS-LOO runs at most 65535 draws (n <= 65535)")
    return max(128, (slab_bytes // (4 * n)) // 128 * 128)


def _psis_slabs(rows, n, chunk, dev, fill):
    """PSIS-LOO over the rows in slabs of `chunk`: fill(lo, count, buf) launches the rows entry that writes ll[:, lo:lo + count] as an
    (n, count) matrix at the head of the one reused buffer, and d3p_psis_loo follows on the same stream.  Returns (elpd_loo, lppd,
    pareto_k), each (rows,) float32."""
    lib = _lib.load()
    elpd, lppd, khat = (torch.empty((rows,), dtype=torch.float32, device=dev) for _ in range(3))
    buf = torch.empty((n * min(chunk, rows),), dtype=torch.float32, device=dev)
    for lo in range(0, rows, chunk):
        count = min(chunk, rows - lo)
        fill(lo, count, buf)
        check(lib.d3p_psis_loo(stream_ptr(), ptr(buf), count, n, count, ptr(elpd[lo:]), ptr(lppd[lo:]), ptr(khat[lo:])))
    return elpd, lppd, khat


def _launch(lppd, model, fam, model_args, rows, d, n, latent, waic_ddof=None, loo_chunk=None):
    """latent = (tensor at the first latent row, ld, w_off, b_col); returns (n, rows) or (rows,) float32 on the current GPU.
    waic_ddof = 0 or 1 (d3p_amd.criteria): the WAIC form, which returns (lppd, p_waic), both (rows,).  loo_chunk (d3p_amd.criteria):
    the PSIS-LOO form in row slabs of that many rows, which returns (elpd_loo, lppd, pareto_k), each (rows,)."""
    first, ld, w_off, b_col = latent
    X = M._f32(model_args[0], "X")
    y = M._f32(model_args[1], "y").reshape(rows)
    if loo_chunk is not None:
        ms = _model_struct(model, fam, d)

        def fill(lo, count, buf):
            check(_lib.load().d3p_loglik_rows(stream_ptr(), C.byref(ms), ptr(X[lo:lo + count]), ptr(y[lo:lo + count]), count, ptr(first), ld,
                                              w_off, b_col, n, ptr(buf)))
        return _psis_slabs(rows, n, loo_chunk, X.device, fill)
    if waic_ddof is not None:
        out, pw = torch.empty((rows,), dtype=torch.float32, device=X.device), torch.empty((rows,), dtype=torch.float32, device=X.device)
        ms = _model_struct(model, fam, d)
        check(_lib.load().d3p_loglik_waic(stream_ptr(), C.byref(ms), ptr(X), ptr(y), rows, ptr(first), ld, w_off, b_col, n, int(waic_ddof),
                                          ptr(out), ptr(pw)))
        return out, pw
    out = torch.empty((rows,) if lppd else (n, rows), dtype=torch.float32, device=X.device)
    ms = _model_struct(model, fam, d)
    fn = _lib.load().d3p_loglik_lppd if lppd else _lib.load().d3p_loglik_rows
    check(fn(stream_ptr(), C.byref(ms), ptr(X), ptr(y), rows, ptr(first), ld, w_off, b_col, n, ptr(out)))
    return out


def _over_samples(lppd, model, posterior_samples, model_args, waic_ddof=None, loo_slab_bytes=None):
    fam = _family(model)
    rows, d = _data(model, model_args)
    n, single = _sample_shape(model, posterior_samples, d)
    _check_ddof(n, waic_ddof)
    chunk = _loo_chunk(n, loo_slab_bytes)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(M._device()):
        out = _launch(lppd, model, fam, model_args, rows, d, n, _pack(model, posterior_samples, n, d), waic_ddof, chunk)
    return out, single, rows, d


def _check_ddof(n, ddof):
    """The WAIC forms' divisor n - ddof (None: not a WAIC form): ddof is 0 or 1 and n > ddof."""
    if ddof is None:
        return
    if isinstance(ddof, bool) or ddof not in (0, 1):
        raise ValueError(f"ddof must be 0 or 1, got {ddof!r}")
    if n <= ddof:
        raise ValueError(f"{n} posterior draw(s): the variance over the draws with ddof = {ddof} needs n > ddof")


def log_likelihood(model, posterior_samples, *model_args, **kwargs):
    """numpyro.infer.util.log_likelihood(model, posterior_samples, *args): ``{"obs": (n, rows) float32}`` with
    ``[s, r] = log p(y_r | x_r, sample s)``, UNSCALED (no plate factor, no observation scale).

    ``model_args = (X, y[, N])``, the models' call signature; ``posterior_samples = {"w": (n, d)[, "intercept": (n,) or (n, 1)]}``
    as torch tensors or numpy arrays (what ``sample_multi_posterior_predictive`` returns is read in place).  A single sample
    (``w`` of shape ``(d,)``) returns ``(rows,)``."""
    out, single, rows, d = _over_samples(False, model, posterior_samples, model_args)
    return {_obs_site(model, d, rows): out[0] if single else out}


def log_predictive_density(model, posterior_samples, *model_args, **kwargs):
    """The log pointwise predictive density over given samples: ``(rows,)`` float32 with
    ``[r] = logsumexp_s log p(y_r | x_r, sample s) - log n`` of the UNSCALED log-probabilities of ``log_likelihood``, computed
    without the ``(n, rows)`` matrix.  A draw of probability 0 (``-inf``) counts as 0; a row is ``-inf`` only if every draw is."""
    return _over_samples(True, model, posterior_samples, model_args)[0]


def _check_guide(model, guide):
    ok = (AutoDiagonalNormal, DiagonalNormalGuide) + ((MeanFieldGuide,) if isinstance(model, LogisticRegression) else ())
    if not isinstance(guide, ok):
        raise TypeError(f"log predictive density: guide {type(guide).__name__} is not supported with {type(model).__name__}")


def _guide_latents(key, n, model, guide, gparams, d, rows, dev):
    """n draws of the guide's latents: one d3p_predict_draws launch with the multi form's key split and the guide chain's site keys,
    exactly the launch sample_multi_posterior_predictive makes (with `obs` observed, which takes no key).  Returns the latent
    tuple of _launch."""
    gp = {name: M._f32(v, f"params['{name}']") for name, v in gparams}
    plan = M.site_plan(LogisticRegression(d, intercept=model.intercept), guide, {"obs"}, d=d, rows=rows)   # (the regression layout)
    kind = _lib.D3P_PREDICT_SCALE_GIVEN if isinstance(guide, AutoDiagonalNormal) else _lib.D3P_PREDICT_SCALE_EXP
    sites = []
    for st in plan:
        if st.chain != "guide":
            continue
        if isinstance(guide, MeanFieldGuide):
            loc, sc = gp[st.name + "_loc"], gp[st.name + "_std_log"]
        elif isinstance(guide, DiagonalNormalGuide):
            loc, sc = gp[guide.site + "_loc"], gp[guide.site + "_std_log"]
        else:
            loc, sc = gp["auto_loc"], gp["auto_scale"]
        sites.append((st, loc, sc, kind, 0.0, 1.0, None))
    D = sum(st.size for st, *_ in sites)
    latent, _ = M._draw_sites(key, n, True, True, sites, None, D, dev)
    w_cols, b_idx = M._latent_layout(d, model.intercept)   # one site over [w | intercept], or the sites 'w' then 'intercept'
    return latent, latent.shape[1], w_cols.start, (-1 if b_idx is None else b_idx)


def posterior_log_predictive_density(rng_key, n, model, model_args, guide, params, **kwargs):
    """``log_predictive_density`` over ``n`` draws from the guide at ``params`` (as ``DPSVI.get_params`` returns them), drawn on the
    device and consumed there: ``(rows,)`` float32, UNSCALED log-probabilities.  ``model_args = (X, y[, N])``; ``rng_key`` is a
    threefry (jax) key as for ``d3p_amd.modelling``.  The draws follow ``sample_multi_posterior_predictive``'s key rule (draw i on
    ``split(rng_key, n)[i]``, the guide's chain, site key 0 onwards): with the same key and ``n`` the latents are the ones that
    function returns.  Guides: ``AutoDiagonalNormal``, ``DiagonalNormalGuide``; ``MeanFieldGuide`` for logistic regression."""
    return _posterior(rng_key, n, model, model_args, guide, params)


def _posterior(rng_key, n, model, model_args, guide, params, waic_ddof=None, loo_slab_bytes=None):
    fam = _family(model)
    _check_guide(model, guide)
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    rows, d = _data(model, model_args)
    _check_ddof(n, waic_ddof)
    chunk = _loo_chunk(n, loo_slab_bytes)
    if not isinstance(params, dict):
        raise ValueError("params: the dict DPSVI.get_params returns is required")
    gparams = [(name, M._param(params, name, size)) for name, size in M._guide_param_names(guide, model, d)]
    key = M._check_key(rng_key)
    _lib.require_device()
    dev = key.device
    with torch.cuda.device(dev):
        latent = _guide_latents(key, n, model, guide, gparams, d, rows, dev)
        return _launch(True, model, fam, model_args, rows, d, n, latent, waic_ddof, chunk)

"""Predictive sampling for the regression family: outcomes of ``obs`` drawn from the prior or posterior predictive.

    predictive_samples(rng_key, model, posterior_samples, X[, y[, N]])            -> obs (n, rows)
    posterior_predictive_samples(rng_key, n, model, (X[, y[, N]]), guide, params) -> {"w", ["intercept",] "obs"}
    prior_predictive_samples(rng_key, n, model, (X,), substitutes=None)           -> {"w", ["intercept",] "obs"}

``LinearRegression`` gives ``obs`` as float32, ``PoissonRegression`` and ``LogisticRegression`` as int32; every other model raises
``TypeError``.  ``d3p_amd.modelling`` keeps refusing the two newer families; this module covers the three, and for
``LogisticRegression`` it runs ``modelling``'s own path: latents and ``obs`` are the ones ``sample_multi_posterior_predictive`` /
``sample_multi_prior_predictive`` return for the same key, bit for bit.

Key rule (DESIGN.md sections 4b, 4e), that of ``modelling``'s multi forms: draw ``i`` runs on ``split(rng_key, n)[i]``; a posterior draw
splits that key into the model's and the guide's chain; site keys follow program order, and the key of ``obs`` is the one
``d3p_predict_draws`` returns.  For the two newer families the latents are those ``posterior_predictive_moments`` and
``posterior_log_predictive_density`` consume: ``sample_multi_posterior_predictive``'s for a ``LogisticRegression`` of the same ``d``,
intercept and guide.  ``predictive_samples`` has no latent site to draw: the ``obs`` key of sample ``s`` is ``split(rng_key, n)[s]``.

Outcome rules, with ``t[s, r] = X[r] . w_s (+ intercept_s)`` in float32:

    linear    obs = fl(t + fl(eps * obs_scale)), eps = normal(obs key, (rows,))[r]            (numpyro's Normal.sample)
    Poisson   lam = exp(t) in float32, then in float64: inversion below a rate of 10, Hoermann's transformed rejection (PTRS) from
              there, on uniforms of fold_in(obs key, j).  NaN t gives -1, a rate of 0 gives 0, a rate of +inf or a draw above
              2^31 - 1 gives 2147483647.  This is the project's own rule: ``jax.random.poisson`` is not restated, so the counts are
              Poisson-distributed but not the ones jax would draw from the same key.

The work runs in ``d3p_amd/csrc/d3p_predict_glm.hip``: the draws x rows product on the matrix cores with the
outcome rule as its epilogue; ``t``, ``eps`` and the uniforms never reach memory.  There is no CPU fallback.
"""
import ctypes as C

import torch

from . import _lib
from . import modelling as M
from ._lib import check, ptr, stream_ptr
from .infer_util import _FAMILY, _check_guide, _model_struct, _pack, _sample_shape
from .models import AutoDiagonalNormal, DiagonalNormalGuide, LogisticRegression, MeanFieldGuide

__all__ = ["predictive_samples", "posterior_predictive_samples", "prior_predictive_samples"]


def _family(model):
    fam = _FAMILY.get(type(model))
    if fam is None:
        raise TypeError(f"predictive sampling: unsupported model {type(model).__name__} (LogisticRegression, LinearRegression and "
                        "PoissonRegression draw outcomes over a linear predictor)")
    return fam


def _data(model, model_args, kwargs):
    """(rows, d) of model_args = (X[, y[, N]]) after the host checks; y is accepted and not read, N only compared with the rows."""
    if not isinstance(model_args, (tuple, list)) or len(model_args) < 1 or model_args[0] is None:
        raise ValueError(f"{type(model).__name__}: model_args = (X[, y[, N]]) with X of shape (rows, d)")
    rows, d = M._rows_of(model_args[0], "X")
    if model.d is not None and int(model.d) != d:
        raise ValueError(f"X has {d} columns, the model {model.d}")
    M._check_plate(M._num_obs_total(kwargs, model_args[2] if len(model_args) >= 3 else None), rows)
    if rows < 1 or d < 1:
        raise ValueError("X: at least one row and one column")
    return rows, d


def _count(n):
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    return n


def _stand_in(model, d):
    """The LogisticRegression with the model's latent sites: the regression layout of modelling.site_plan."""
    return LogisticRegression(d, prior_scale=model.prior_scale, intercept=model.intercept, intercept_prior_scale=model.intercept_prior_scale)


def _outcomes(model, fam, X, rows, d, n, latent, obs_keys):
    """latent = (tensor at the first latent row, ld, w_off, b_col); obs (n, rows) on the current GPU."""
    first, ld, w_off, b_col = latent
    X = M._f32(X, "X")
    lib = _lib.load()
    if fam == _lib.D3P_FAMILY_LOGREG:
        obs = torch.empty((n, rows), dtype=torch.int32, device=X.device)
        check(lib.d3p_predict_logreg(stream_ptr(), ptr(X), rows, d, ptr(first), ld, w_off, b_col, n, ptr(obs_keys), ptr(obs)))
        return obs
    obs = torch.empty((n, rows), dtype=torch.float32 if fam == _lib.D3P_FAMILY_LINREG else torch.int32, device=X.device)
    ms = _model_struct(model, fam, d)
    check(lib.d3p_predict_glm(stream_ptr(), C.byref(ms), ptr(X), rows, d, ptr(first), ld, w_off, b_col, n, ptr(obs_keys), ptr(obs)))
    return obs


def predictive_samples(rng_key, model, posterior_samples, *model_args, **kwargs):
    """Outcomes of ``obs`` over given samples: ``(n, rows)`` on the GPU, float32 (linear) or int32 (Poisson, logistic), sample ``s``
    drawn with the ``obs`` key ``split(rng_key, n)[s]``.

    ``model_args = (X[, y[, N]])``; ``y`` and ``N`` are accepted and not read.  ``posterior_samples = {"w": (n, d)[, "intercept": (n,)
    or (n, 1)]}`` as torch tensors or numpy arrays, read as in ``predictive_moments``: packed views (what
    ``posterior_predictive_samples`` returns) in place, otherwise packed once.  A single sample (``w`` of shape ``(d,)``) is ``n = 1``
    and returns ``(rows,)``.

    Relation to ``posterior_predictive_samples(key, n, ...)``: both apply ONE outcome rule, ``obs[s] = rule(t_s, obs key of s)``, to
    the same ``t_s`` when handed the latents that call returned; they differ in the ``obs`` key alone.  There it is the ``obs`` site's
    key of draw ``s`` -- ``split(mk)[1]`` with ``mk = split(split(key, n)[s])[0]``, the model's chain -- here ``split(rng_key, n)[s]``.
    A threefry key cannot be chosen to make the two coincide, so the outcomes are independent draws from the same predictive, each
    reproducible on the CPU from its own key (tests/predictive_glm_ref.py)."""
    fam = _family(model)
    rows, d = _data(model, model_args, kwargs)
    n, single = _sample_shape(model, posterior_samples, d)
    key = M._check_key(rng_key)
    _lib.require_device()   # (every check above runs without a device)
    dev = key.device
    with torch.cuda.device(dev):
        obs_keys = torch.empty((n, 2), dtype=torch.uint32, device=dev)
        check(_lib.load().d3p_tf_split(stream_ptr(), ptr(key), n, ptr(obs_keys)))
        obs = _outcomes(model, fam, model_args[0], rows, d, n, _pack(model, posterior_samples, n, d), obs_keys)
    return obs[0] if single else obs


def _latents(key, n, model, rows, d, guide, gparams, substitutes):
    """n draws of the latent sites and the obs keys: one d3p_predict_draws launch with the multi form's key split -- exactly the
    launch modelling makes for a LogisticRegression of the same layout.  Returns ({"w"[, "intercept"]} as views of the packed buffer,
    the kernels' latent tuple (first, ld, w_off, b_col), the obs keys (n, 2) or None, the obs Site).  The half of _draw that
    d3p_amd.ppc shares: there the outcomes are reduced (d3p_predict_stats) instead of stored."""
    dev = key.device
    posterior = guide is not None
    stand_in = _stand_in(model, d)
    plan = M.site_plan(stand_in, guide, set(substitutes), d=d, rows=rows)
    sites = []
    if posterior:
        gp = {name: M._f32(v, f"params['{name}']") for name, v in gparams}
        kind = _lib.D3P_PREDICT_SCALE_GIVEN if isinstance(guide, AutoDiagonalNormal) else _lib.D3P_PREDICT_SCALE_EXP
        for st in plan:
            if st.chain != "guide":
                continue
            if isinstance(guide, MeanFieldGuide):   # (logistic regression only: _check_guide)
                loc, sc = gp[st.name + "_loc"], gp[st.name + "_std_log"]
            elif isinstance(guide, DiagonalNormalGuide):
                loc, sc = gp[guide.site + "_loc"], gp[guide.site + "_std_log"]
            else:
                loc, sc = gp["auto_loc"], gp["auto_scale"]
            sites.append((st, loc, sc, kind, 0.0, 1.0, None))
    else:
        for st in plan:
            if st.name == "obs":
                continue
            prior = model.intercept_prior_scale if st.name == "intercept" else model.prior_scale
            value = M._f32(substitutes[st.name], f"substitutes['{st.name}']").reshape(-1) if st.substituted else None
            sites.append((st, None, None, _lib.D3P_PREDICT_SCALE_CONST, 0.0, prior, value))
    obs_site = next(st for st in plan if st.name == "obs")
    D = sum(st.size for st, *_ in sites)
    latent, obs_keys = M._draw_sites(key, n, True, posterior, sites, obs_site, D, dev)
    w_cols, b_idx = M._latent_layout(d, model.intercept)   # one guide site over [w | intercept], or the sites 'w' then 'intercept'
    out = {"w": latent[:, w_cols]}
    if b_idx is not None:
        out["intercept"] = latent[:, b_idx]
    return out, (latent, latent.shape[1], w_cols.start, -1 if b_idx is None else b_idx), obs_keys, obs_site


def _draw(key, n, model, fam, X, rows, d, guide, gparams, substitutes):
    """n draws of the latent sites and of obs for the linear / Poisson families: _latents, then the outcome kernel."""
    out, latent, obs_keys, obs_site = _latents(key, n, model, rows, d, guide, gparams, substitutes)
    if obs_site.substituted:
        dev = key.device
        o = torch.as_tensor(substitutes["obs"]).to(dev)
        out["obs"] = o.reshape((1,) + tuple(o.shape)).expand((n,) + tuple(o.shape))
    else:
        out["obs"] = _outcomes(model, fam, X, rows, d, n, latent, obs_keys)
    return out


def _sites_of(res, model):
    return {k: res[k] for k in (("w", "intercept") if model.intercept else ("w",)) + ("obs",)}


def posterior_predictive_samples(rng_key, n, model, model_args, guide, params, **kwargs):
    """``n`` draws from the posterior predictive at ``params`` (as ``DPSVI.get_params`` returns them): ``{"w": (n, d)[, "intercept":
    (n,)], "obs": (n, rows)}`` on the GPU, the latents as views of one packed buffer.  ``model_args = (X[, y[, N]])``; ``rng_key`` is a
    threefry (jax) key as for ``d3p_amd.modelling``, and the draws follow ``sample_multi_posterior_predictive``'s key rule (module
    docstring).  Guides: ``AutoDiagonalNormal``, ``DiagonalNormalGuide``; ``MeanFieldGuide`` for logistic regression."""
    fam = _family(model)
    _check_guide(model, guide)
    n = _count(n)
    rows, d = _data(model, model_args, kwargs)
    if not isinstance(params, dict):
        raise ValueError("params: the dict DPSVI.get_params returns is required")
    gparams = [(name, M._param(params, name, size)) for name, size in M._guide_param_names(guide, model, d)]
    key = M._check_key(rng_key)
    if fam == _lib.D3P_FAMILY_LOGREG:   # modelling's own path (which ends in require_device after the same checks)
        return _sites_of(M.sample_multi_posterior_predictive(key, n, model, (model_args[0],), guide, (model_args[0],), params), model)
    _lib.require_device()
    with torch.cuda.device(key.device):
        return _draw(key, n, model, fam, model_args[0], rows, d, guide, gparams, {})


def prior_predictive_samples(rng_key, n, model, model_args, substitutes=None, **kwargs):
    """``n`` draws from the prior predictive: ``{"w": (n, d)[, "intercept": (n,)], "obs": (n, rows)}`` on the GPU.  ``model_args =
    (X[, y[, N]])``; ``substitutes`` freezes sites (``w``, ``intercept``, ``obs``) to given values, the same in every draw; a frozen
    site takes no key, as in ``sample_multi_prior_predictive``, whose key rule the draws follow (module docstring)."""
    fam = _family(model)
    n = _count(n)
    rows, d = _data(model, model_args, kwargs)
    substitutes = dict(substitutes or {})
    names = dict(M._model_sites(_stand_in(model, d), d, rows))
    for k, v in substitutes.items():
        if k not in names:
            raise ValueError(f"substitutes: '{k}' is not a sample site of {type(model).__name__} ({list(names)})")
        if M._numel(v) != names[k]:
            raise ValueError(f"substitutes['{k}']: {names[k]} values expected, got {M._numel(v)}")
    key = M._check_key(rng_key)
    if fam == _lib.D3P_FAMILY_LOGREG:
        return _sites_of(M.sample_multi_prior_predictive(key, n, model, (model_args[0],), substitutes), model)
    _lib.require_device()
    with torch.cuda.device(key.device):
        return _draw(key, n, model, fam, model_args[0], rows, d, None, None, substitutes)

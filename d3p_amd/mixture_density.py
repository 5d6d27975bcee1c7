"""Held-out log predictive density and responsibilities of the Gaussian mixture model over posterior draws.

    log_likelihood(model, posterior_samples, obs)            -> {"obs": (n, rows)} float32
    log_predictive_density(model, posterior_samples, obs)    -> (rows,) float32
    responsibilities(model, posterior_samples, obs)          -> (rows, k) float32
    posterior_log_predictive_density(rng_key, n, model, model_args, guide, params, **kw) -> (rows,)
    posterior_responsibilities(rng_key, n, model, model_args, guide, params, **kw)       -> (rows, k)
    posterior_summary(rng_key, n, model, model_args, guide, params, **kw) -> {"log_predictive_density", "responsibilities"}, one pass

``d3p_amd.infer_util`` keeps refusing ``GaussianMixtureModel``; this module is the family's scoring surface, as ``d3p_amd.mixture`` is
its sampling surface.  With ``a[s, r, j] = log pis[s, j] + sum_c log N(obs[r, c]; mus[s, j, c], sigs[s, j, c])``:

    ll[s, r]   = logsumexp_j a[s, r, j]                 log_likelihood: UNSCALED (no plate factor), as numpyro's log_likelihood returns it
    lppd[r]    = logsumexp_s ll[s, r] - log n           log_predictive_density
    resp[r, j] = (1 / n) sum_s exp(a[s, r, j] - ll[s, r])   responsibilities: the soft assignment averaged over the draws

``posterior_samples = {"pis": (n, k), "mus": (n, k, d), "sigs": broadcastable to (n, k, d)}`` with the leading draw axis required.
Samples that are views of one packed float32 buffer in the kernels' layout ``[pis | mus | sigs]`` per draw -- what
``mixture.posterior_predictive_samples`` returns -- are read in place; anything else is packed once.  The ``posterior_*`` functions
take ``model_args = (k, obs, num_obs_total, d)`` as ``d3p_amd.mixture`` reads them, with ``obs`` REQUIRED (its values are used); they
draw the latents with the one ``d3p_predict_gmm_draws`` launch on the multi form's key rule, so they are the latents
``mixture.posterior_predictive_samples(rng_key, n, ...)`` returns for the same key, and consume them on the device.

Arithmetic (``d3p_amd/csrc/d3p_gmm_density.hip``): the direct form in float32 with ``1 / sigs`` formed once per draw and ``log pis_j -
sum_c log sigs_jc - d log(2 pi) / 2`` hoisted per (draw, component); the sums over the draws in float64 in a fixed order: the reduced
forms never hold an ``(n, rows)`` or ``(n, rows, k)`` array, and two calls give identical bits.

Special values: ``pis[s, j] == 0`` makes that component add nothing (responsibility 0 in that draw).  A draw whose every component is
``-inf`` has ``ll = -inf``, not NaN -- and contributes NaN (0 / 0) to that row's ``responsibilities``, so the row's responsibilities
are NaN; if every draw is ``-inf``, ``lppd = -inf``.  A NaN anywhere in a row of ``obs`` makes that row's outputs NaN; a NaN in a draw's
latents makes that draw's ``ll`` NaN for every row, and with it every reduced output.  Every host check runs before the device is
touched; there is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from . import mixture as MX
from . import modelling as M
from ._lib import check, ptr, stream_ptr
from .infer_util import _check_ddof, _loo_chunk, _psis_slabs
from .models import GaussianMixtureGuide, GaussianMixtureModel

__all__ = ["log_likelihood", "log_predictive_density", "responsibilities", "posterior_log_predictive_density",
           "posterior_responsibilities", "posterior_summary", "ROW_TILE", "DRAW_TILE"]

# rows one workgroup of k_gmm_density owns (D3P_GD_ROW_TILE), and the number of waves that split the draws among themselves
# (D3P_GD_DRAW_TILE: wave w takes the draws w, w + 4, ...; the two largest shapes, whose four latent copies do not fit in LDS, use 2)
ROW_TILE = 64
DRAW_TILE = 4

SITES = ("pis", "mus", "sigs")


def _check_model(model):
    if not isinstance(model, GaussianMixtureModel):
        raise TypeError(f"mixture density: model must be a GaussianMixtureModel, got {type(model).__name__}")


def _sample_shapes(samples):
    """(n, k, d) of posterior_samples, every shape checked."""
    if not isinstance(samples, dict) or any(name not in samples for name in SITES):
        raise ValueError(f"posterior_samples: a dict with {SITES} is required")
    ps, ms = MX._shape_of(samples["pis"]), MX._shape_of(samples["mus"])
    if len(ps) != 2:
        raise ValueError(f"posterior_samples['pis']: shape (n, k) with the leading draw axis expected, got {ps}")
    n, k = int(ps[0]), int(ps[1])
    if len(ms) != 3 or ms[0] != n or ms[1] != k:
        raise ValueError(f"posterior_samples['mus']: shape ({n}, {k}, d) expected, got {ms}")
    d = int(ms[2])
    MX._broadcastable(samples["sigs"], (n, k, d), "posterior_samples['sigs']")
    if n < 1:
        raise ValueError("posterior_samples: at least one draw (n must be >= 1)")
    if n > 2 ** 31 - 1:
        raise ValueError("posterior_samples: n <= 2^31 - 1")
    return n, k, d


def _packed_view(pis, mus, sigs, n, k, d, device):
    """(tensor whose data_ptr is the first latent row, ld) when pis (n, k), mus (n, k, d) and sigs (n, k, d) already are the columns
    [pis | mus | sigs] of one row-major float32 buffer on `device` -- as mixture.posterior_predictive_samples returns them -- else
    None.  Pointers and strides only; nothing is read."""
    ts = (pis, mus, sigs)
    if not all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device for t in ts):
        return None
    if tuple(pis.shape) != (n, k) or tuple(mus.shape) != (n, k, d) or tuple(sigs.shape) != (n, k, d):
        return None
    base = pis.untyped_storage().data_ptr()
    if any(t.untyped_storage().data_ptr() != base for t in ts):
        return None
    kd = k * d
    ld = pis.stride(0) if n > 1 else k + 2 * kd
    if ld < k + 2 * kd:
        return None

    def strides_ok(t, want):   # (the stride of an axis of length 1 is arbitrary)
        return all(size == 1 or st == w for size, st, w in zip(t.shape, t.stride(), want))

    if not (strides_ok(pis, (ld, 1)) and strides_ok(mus, (ld, d, 1)) and strides_ok(sigs, (ld, d, 1))):
        return None
    o = pis.storage_offset()
    if mus.storage_offset() != o + k or sigs.storage_offset() != o + k + kd:
        return None
    return pis, int(ld)


def _pack(samples, n, k, d):
    """The (n, ld) latent buffer of the kernels: the samples themselves when they are a packed view, else one copy."""
    view = None
    if all(isinstance(samples[name], torch.Tensor) for name in SITES):
        view = _packed_view(samples["pis"].detach(), samples["mus"].detach(), samples["sigs"].detach(), n, k, d, M._device())
    if view is not None:
        return view
    kd = k * d
    buf = torch.empty((n, k + 2 * kd), dtype=torch.float32, device=M._device())
    buf[:, :k] = M._f32(samples["pis"], "posterior_samples['pis']")
    buf[:, k:k + kd] = M._f32(samples["mus"], "posterior_samples['mus']").reshape(n, kd)
    buf[:, k + kd:] = torch.broadcast_to(M._f32(samples["sigs"], "posterior_samples['sigs']"), (n, k, d)).reshape(n, kd)
    return buf, k + 2 * kd


def _run(x, rows, d, latent, ld, k, n, want_ll, want_lppd, want_resp, waic_ddof=None, loo_chunk=None):
    """The launches on the current device; x is (rows, d) float32 contiguous there.  waic_ddof = 0 or 1 (d3p_amd.criteria): the
    WAIC form, which returns (lppd, p_waic), both (rows,).  loo_chunk (d3p_amd.criteria): the PSIS-LOO form in row slabs of that many
    rows, which returns (elpd_loo, lppd, pareto_k), each (rows,)."""
    dev = x.device
    lib = _lib.load()
    if loo_chunk is not None:
        def fill(lo, count, buf):
            check(lib.d3p_gmm_loglik_rows(stream_ptr(), ptr(x[lo:lo + count]), count, d, ptr(latent), ld, k, n, ptr(buf)))
        return _psis_slabs(rows, n, loo_chunk, dev, fill)
    if waic_ddof is not None:
        lppd, pw = torch.empty((rows,), dtype=torch.float32, device=dev), torch.empty((rows,), dtype=torch.float32, device=dev)
        if rows > 0:
            check(lib.d3p_gmm_loglik_waic(stream_ptr(), ptr(x), rows, d, ptr(latent), ld, k, n, int(waic_ddof), ptr(lppd), ptr(pw)))
        return lppd, pw
    if want_ll:
        ll = torch.empty((n, rows), dtype=torch.float32, device=dev)
        if rows > 0:
            check(lib.d3p_gmm_loglik_rows(stream_ptr(), ptr(x), rows, d, ptr(latent), ld, k, n, ptr(ll)))
        return ll
    lppd = torch.empty((rows,), dtype=torch.float32, device=dev) if want_lppd else None
    resp = torch.empty((rows, k), dtype=torch.float32, device=dev) if want_resp else None
    if rows > 0:
        check(lib.d3p_gmm_loglik_reduce(stream_ptr(), ptr(x), rows, d, ptr(latent), ld, k, n, ptr(lppd), ptr(resp)))
    return lppd, resp


def _from_samples(model, samples, obs, want_ll, want_lppd, want_resp, waic_ddof=None, loo_slab_bytes=None):
    _check_model(model)
    n, k, d = _sample_shapes(samples)
    _check_ddof(n, waic_ddof)
    chunk = _loo_chunk(n, loo_slab_bytes)
    if obs is None:
        raise ValueError("obs is required")
    rows, d_obs = M._rows_of(obs, "obs")
    if int(d_obs) != d:
        raise ValueError(f"obs: shape (rows, {d}) expected, got {tuple(obs.shape)}")
    rows = int(rows)
    MX._check_limits(k, d, rows)
    _lib.require_device()
    dev = obs.device if isinstance(obs, torch.Tensor) and obs.is_cuda else M._device()
    with torch.cuda.device(dev):
        x = M._f32(obs, "obs")
        latent, ld = _pack(samples, n, k, d)
        return _run(x, rows, d, latent, ld, k, n, want_ll, want_lppd, want_resp, waic_ddof, chunk)


def log_likelihood(model, posterior_samples, obs):
    """``{"obs": ll}`` with ``ll[s, r] = log p(obs[r] | draw s)``, ``(n, rows)`` float32 on the GPU: unscaled, as
    ``numpyro.infer.util.log_likelihood`` returns the site's ``log_prob``."""
    return {"obs": _from_samples(model, posterior_samples, obs, True, False, False)}


def log_predictive_density(model, posterior_samples, obs):
    """``lppd[r] = logsumexp_s ll[s, r] - log n``, ``(rows,)`` float32, without writing ``ll``."""
    return _from_samples(model, posterior_samples, obs, False, True, False)[0]


def responsibilities(model, posterior_samples, obs):
    """``resp[r, j] = mean_s softmax_j(a[s, r, :])``, ``(rows, k)`` float32.  A draw in which every component of a row is ``-inf``
    contributes NaN (0 / 0) to that row."""
    return _from_samples(model, posterior_samples, obs, False, False, True)[1]


def _posterior_latents(rng_key, n, model, model_args, guide, params, kwargs, host_checks=None):
    """Every host check of the ``posterior_*`` functions, then the one ``d3p_predict_gmm_draws`` launch on the multi form's key rule:
    ``(x (rows, d) float32, rows, d, latent (n, ld) float32, ld, k, n)`` on the key's device.  ``host_checks(n)`` runs among the host
    checks, before ``model_args`` is read."""
    _check_model(model)
    if not isinstance(guide, GaussianMixtureGuide):
        raise TypeError(f"mixture density: guide must be a GaussianMixtureGuide, got {type(guide).__name__}")
    if n is None:
        raise ValueError("n must be >= 1 (the number of posterior draws)")
    nn, _ = MX._count(n)
    if nn > 2 ** 31 - 1:
        raise ValueError("n <= 2^31 - 1")
    if host_checks is not None:
        host_checks(nn)
    k, rows, d = MX._shape(model, model_args, kwargs)
    a = list(model_args) + [None] * (4 - len(model_args))
    obs = a[1] if a[1] is not None else kwargs.get("obs")
    if obs is None:
        raise ValueError("GaussianMixtureModel: obs is required (model_args[1] or obs=): its values are scored")
    MX._check_limits(k, d, rows)
    if not isinstance(params, dict):
        raise ValueError("params: the dict DPSVI.get_params returns is required")
    for name, shp in (("alpha_log", (k,)), ("mus_loc", (k, d))):
        if MX._shape_of(M._param(params, name, int(np.prod(shp)))) != shp:
            raise ValueError(f"params['{name}']: shape {shp} expected, got {MX._shape_of(params[name])}")
    key = M._check_key(rng_key)   # (last of the checks: everything above runs without a device)
    _lib.require_device()
    lib = _lib.load()
    dev = key.device
    with torch.cuda.device(dev):
        alpha_log, mus_loc = M._f32(params["alpha_log"], "params['alpha_log']"), M._f32(params["mus_loc"], "params['mus_loc']")
        x = M._f32(obs, "obs")
        ld = k + 2 * k * d
        latent = torch.empty((nn, ld), dtype=torch.float32, device=dev)
        obs_keys = torch.empty((nn, 2), dtype=torch.uint32, device=dev)   # (written by the launch, not used here)
        check(lib.d3p_predict_gmm_draws(stream_ptr(), ptr(key), nn, 1, 1, k, d, ptr(alpha_log), ptr(mus_loc),
                                        float(model.prior_mu_scale), None, None, None, ptr(latent), ptr(obs_keys)))
    return x, rows, d, latent, ld, k, nn


def _posterior(rng_key, n, model, model_args, guide, params, kwargs, want_lppd, want_resp, waic_ddof=None, loo_slab_bytes=None):
    chunk = []

    def host_checks(nn):
        _check_ddof(nn, waic_ddof)
        chunk.append(_loo_chunk(nn, loo_slab_bytes))
    x, rows, d, latent, ld, k, nn = _posterior_latents(rng_key, n, model, model_args, guide, params, kwargs, host_checks)
    with torch.cuda.device(x.device):
        return _run(x, rows, d, latent, ld, k, nn, False, want_lppd, want_resp, waic_ddof, chunk[0])


def posterior_log_predictive_density(rng_key, n, model, model_args, guide, params, **kwargs):
    """``log_predictive_density`` of ``model_args``' ``obs`` under ``n`` posterior draws at ``params`` on ``rng_key``: the draws
    ``mixture.posterior_predictive_samples(rng_key, n, ...)`` returns, consumed on the device."""
    return _posterior(rng_key, n, model, model_args, guide, params, kwargs, True, False)[0]


def posterior_responsibilities(rng_key, n, model, model_args, guide, params, **kwargs):
    """``responsibilities`` of ``model_args``' ``obs`` under ``n`` posterior draws at ``params`` on ``rng_key``."""
    return _posterior(rng_key, n, model, model_args, guide, params, kwargs, False, True)[1]


def posterior_summary(rng_key, n, model, model_args, guide, params, **kwargs):
    """Both of the above from ONE pass over the draws: ``{"log_predictive_density": (rows,), "responsibilities": (rows, k)}``."""
    lppd, resp = _posterior(rng_key, n, model, model_args, guide, params, kwargs, True, True)
    return {"log_predictive_density": lppd, "responsibilities": resp}

"""Predictive sampling and cluster assignment for the Gaussian mixture model (reference examples/gaussian_mixture_model.py:51-161).

    prior_predictive_samples(rng_key, n, model, model_args, substitutes=None, with_intermediates=False, **kw)
    posterior_predictive_samples(rng_key, n, model, model_args, guide, params, with_intermediates=False, **kw)
    assignment_log_posterior(obs, mus, sigs, pis)   -> (rows, k) float32
    assign(obs, mus, sigs, pis)                     -> (rows,) int32
    compute_assignment_accuracy(X_test, original_assignment, original_modes, posterior_modes, posterior_pis)

``d3p_amd.modelling`` keeps refusing ``GaussianMixtureModel``; this module is the family's surface.  ``model`` is
a ``GaussianMixtureModel``, ``guide`` a ``GaussianMixtureGuide``; ``model_args = (k, obs_or_None, num_obs_total, d)`` with ``k=`` /
``d=`` / ``num_obs_total=`` keywords, read as the reference's ``model`` reads them (:51-61): with ``obs`` given only its shape is used,
and a ``num_obs_total`` that differs from the rows is refused (full plates only, as in ``modelling``).  ``rng_key`` is a threefry (jax)
key.  ``n=None`` is the single-draw form (no leading axis, the draw runs on ``rng_key`` itself); an integer ``n`` the multi form.  Both
sampling functions return ``{"pis": (n, k), "mus": (n, k, d), "sigs": (n, k, d), "obs": (n, rows, d)}`` as CUDA float32 tensors, the
latents as views of one packed buffer; with ``with_intermediates`` every site is ``(value, [])`` as in ``modelling`` and ``obs`` is
``(xs, (zs,))`` with ``zs`` the ``(n, rows)`` int32 component of every row (the reference's trace).

Key rule (section 4b's, extended): draw ``i`` runs on ``split(rng_key, n)[i]``; the prior seeds the model's
chain with that key, the posterior does ``model_key, guide_key = split(key)``; every key-taking sample statement does ``chain,
site_key = split(chain)`` in program order ``pis, mus, sigs`` (guide or model), then ``obs`` (model).  A substituted site takes no key,
so the later sites' keys shift; in the posterior the three latents are substituted by the guide's draws, so ``obs`` takes the model
chain's key 0.

Site rules (one device function each, ``d3p_amd/csrc/d3p_predict_gmm.hip``): ``pis = g / sum g`` with ``g_j`` the project's own
Gamma(alpha_j, 1) draw in float64 (``alpha = exp(alpha_log)``, prior: 1; no bit parity with ``jax.random.gamma``); ``mus = fl(loc +
fl(normal * scale))`` with ``(mus_loc, 1)`` in the guide and ``(0, prior_mu_scale)`` in the model; ``sigs = 1 / -logf(u)``; ``obs`` is
``GaussianMixture.sample_with_intermediates``: ``z = min(#{j : cum_j < u}, k - 1)`` on the float32 running sum of ``pis`` taken left to
right, ``x = fl(mus[z] + fl(sigs[z] * eps))``.  Every host check runs before the device is touched; there is no CPU fallback.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import modelling as M
from ._lib import check, ptr, stream_ptr
from .models import GaussianMixtureGuide, GaussianMixtureModel

__all__ = ["prior_predictive_samples", "posterior_predictive_samples", "assignment_log_posterior", "assign",
           "compute_assignment_accuracy", "ROW_TILE"]

# rows of the output one workgroup of k_predict_gmm_obs covers (2 D3P_PGM_TP in d3p_predict_gmm.hip: TP rows of the lower half of the
# normals' stream and their partners in the upper half)
ROW_TILE = 128

LATENT_SITES = ("pis", "mus", "sigs")

# chain: "model" or "guide" (the seed handler the statement runs under); key_index: how many key-taking statements precede it under
# that handler (None: substituted, it takes no key)
Site = namedtuple("Site", ["name", "chain", "key_index"])


def _key_plan(posterior, substituted=()):
    """The family's trace as a list of Site in program order pis, mus, sigs, obs: the host's statement of the rule
    d3p_predict_gmm_draws applies on its own (it counts the key indices from which values are given).  Nothing here reaches the
    device; _sample uses it to refuse bad `substitutes`, tests/mixture_ref.py to rebuild the keys the device must have used."""
    substituted = set(substituted)
    unknown = substituted - set(LATENT_SITES)
    if unknown:
        raise ValueError(f"substitutes: {sorted(unknown)} are not latent sites of GaussianMixtureModel {LATENT_SITES}")
    if posterior:
        if substituted:
            raise ValueError("substitutes are a prior-predictive argument")
        # the guide's draws are substituted into the model: its three latent statements take no key, obs takes key 0
        return [Site(name, "guide", i) for i, name in enumerate(LATENT_SITES)] + [Site("obs", "model", 0)]
    plan, nxt = [], 0
    for name in LATENT_SITES + ("obs",):
        if name in substituted:
            plan.append(Site(name, "model", None))
        else:
            plan.append(Site(name, "model", nxt))
            nxt += 1
    return plan


def _check_limits(k, d, rows=0):
    if k < 1 or d < 1:
        raise ValueError(f"GaussianMixtureModel: k and d must be >= 1 (k = {k}, d = {d})")
    if k > 32 or d > 256 or (k > 16 and d > 128):
        raise ValueError(f"GaussianMixtureModel: supported shapes are k <= 16 with d <= 256 and k <= 32 with d <= 128 (k = {k}, d = {d})")
    if rows * d >= 2 ** 32:
        raise ValueError(f"rows * d = {rows * d} must stay below 2^32 (one threefry stream per draw)")


def _shape(model, model_args, kwargs):
    """(k, rows, d) from model_args = (k, obs_or_None, num_obs_total, d) and the keywords, as the reference's model reads them."""
    if not isinstance(model_args, (tuple, list)):
        raise ValueError("GaussianMixtureModel: model_args = (k, obs_or_None, num_obs_total, d)")
    a = list(model_args) + [None] * (4 - len(model_args))
    if len(a) > 4:
        raise ValueError("GaussianMixtureModel: model_args = (k, obs_or_None, num_obs_total, d)")
    k = a[0] if a[0] is not None else (kwargs.get("k") if kwargs.get("k") is not None else model.k)
    obs = a[1] if a[1] is not None else kwargs.get("obs")
    total = a[2] if a[2] is not None else M._num_obs_total(kwargs)
    d = a[3] if a[3] is not None else (kwargs.get("d") if kwargs.get("d") is not None else model.d)
    if k is None:
        raise ValueError("GaussianMixtureModel: the number of components k is required (model_args[0], k= or GaussianMixtureModel(k=))")
    if obs is not None:
        rows, d = M._rows_of(obs, "obs")      # (only the shape is used: `obs` is the site being drawn)
        M._check_plate(total, rows)
    else:
        if total is None:
            raise ValueError("GaussianMixtureModel: without obs, num_obs_total is required")
        if d is None:
            raise ValueError("GaussianMixtureModel: without obs, the dimension d is required")
        rows = int(total)
    k, rows, d = int(k), int(rows), int(d)
    if rows < 1:
        raise ValueError("GaussianMixtureModel: at least one row")
    return k, rows, d


def _count(n):
    if n is None:
        return 1, False
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    return n, True


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else tuple(np.shape(x))


def _broadcastable(x, shape, what):
    try:
        ok = np.broadcast_shapes(_shape_of(x), shape) == shape
    except ValueError:
        ok = False
    if not ok:
        raise ValueError(f"{what}: shape {_shape_of(x)} does not broadcast to {shape}")


def _sample(rng_key, n, model, model_args, guide, params, substitutes, with_intermediates, kwargs):
    posterior = guide is not None
    if not isinstance(model, GaussianMixtureModel):
        raise TypeError(f"mixture predictive sampling: model must be a GaussianMixtureModel, got {type(model).__name__}")
    if posterior and not isinstance(guide, GaussianMixtureGuide):
        raise TypeError(f"mixture predictive sampling: guide must be a GaussianMixtureGuide, got {type(guide).__name__}")
    nn, multi = _count(n)
    k, rows, d = _shape(model, model_args, kwargs)
    _check_limits(k, d, rows)
    substitutes = dict(substitutes or {})
    _key_plan(posterior, substitutes)   # (refuses names that are no latent site, and substitutes in the posterior)
    shapes = {"pis": (k,), "mus": (k, d), "sigs": (k, d)}
    for name, v in substitutes.items():
        _broadcastable(v, shapes[name], f"substitutes['{name}']")
    if posterior:
        if not isinstance(params, dict):
            raise ValueError("params: the dict DPSVI.get_params returns is required")
        for name, shp in (("alpha_log", (k,)), ("mus_loc", (k, d))):
            if _shape_of(M._param(params, name, int(np.prod(shp)))) != shp:
                raise ValueError(f"params['{name}']: shape {shp} expected, got {_shape_of(params[name])}")
    if not (model.prior_mu_scale > 0):
        raise ValueError("GaussianMixtureModel: prior_mu_scale must be > 0")
    key = M._check_key(rng_key)   # (last of the checks: everything above runs without a device)
    _lib.require_device()
    lib = _lib.load()
    dev = key.device
    with torch.cuda.device(dev):
        alpha_log = M._f32(params["alpha_log"], "params['alpha_log']") if posterior else None
        mus_loc = M._f32(params["mus_loc"], "params['mus_loc']") if posterior else None
        given = {name: torch.broadcast_to(M._f32(v, f"substitutes['{name}']"), shapes[name]).contiguous() for name, v in substitutes.items()}
        kd = k * d
        latent = torch.empty((nn, k + 2 * kd), dtype=torch.float32, device=dev)
        obs_keys = torch.empty((nn, 2), dtype=torch.uint32, device=dev)
        check(lib.d3p_predict_gmm_draws(stream_ptr(), ptr(key), nn, int(multi), int(posterior), k, d, ptr(alpha_log), ptr(mus_loc),
                                        float(model.prior_mu_scale), ptr(given.get("pis")), ptr(given.get("mus")), ptr(given.get("sigs")),
                                        ptr(latent), ptr(obs_keys)))
        obs = torch.empty((nn, rows, d), dtype=torch.float32, device=dev)
        zs = torch.empty((nn, rows), dtype=torch.int32, device=dev) if with_intermediates else None
        check(lib.d3p_predict_gmm_obs(stream_ptr(), ptr(latent), latent.shape[1], k, d, rows, nn, ptr(obs_keys), ptr(obs), ptr(zs)))
    out = {"pis": latent[:, :k], "mus": latent[:, k:k + kd].view(nn, k, d), "sigs": latent[:, k + kd:].view(nn, k, d), "obs": obs}
    if not multi:
        out = {name: v[0] for name, v in out.items()}
        zs = zs[0] if zs is not None else None
    if with_intermediates:
        out = {name: (v, (zs,) if name == "obs" else []) for name, v in out.items()}
    return out


def prior_predictive_samples(rng_key, n, model, model_args, substitutes=None, with_intermediates=False, **kwargs):
    """``n`` draws from the prior predictive (``n=None``: one draw on ``rng_key`` itself, no leading axis).  ``substitutes`` may hold any
    subset of ``pis`` (k,), ``mus`` and ``sigs`` (broadcast to (k, d)); a given site is the same in every draw and takes no key."""
    return _sample(rng_key, n, model, model_args, None, None, substitutes, with_intermediates, kwargs)


def posterior_predictive_samples(rng_key, n, model, model_args, guide, params, with_intermediates=False, **kwargs):
    """``n`` draws from the posterior predictive at ``params = {"alpha_log": (k,), "mus_loc": (k, d)}`` (as ``DPSVI.get_params`` returns
    them); ``n=None``: one draw on ``rng_key`` itself, no leading axis."""
    if guide is None:
        raise TypeError("mixture predictive sampling: guide must be a GaussianMixtureGuide, got NoneType")
    return _sample(rng_key, n, model, model_args, guide, params, None, with_intermediates, kwargs)


def _assign_args(obs, mus, sigs, pis):
    rows, d = M._rows_of(obs, "obs")
    shp = _shape_of(mus)
    if len(shp) != 2 or shp[1] != d:
        raise ValueError(f"mus: shape (k, {d}) expected, got {shp}")
    k = int(shp[0])
    _broadcastable(sigs, (k, d), "sigs")
    if _shape_of(pis) != (k,):
        raise ValueError(f"pis: shape ({k},) expected, got {_shape_of(pis)}")
    _check_limits(k, int(d), int(rows))
    return int(rows), int(d), k


def _run_assign(obs, mus, sigs, pis, want_a, want_arg):
    rows, d, k = _assign_args(obs, mus, sigs, pis)
    _lib.require_device()
    dev = obs.device if isinstance(obs, torch.Tensor) and obs.is_cuda else M._device()
    with torch.cuda.device(dev):
        x, mu, pi = M._f32(obs, "obs"), M._f32(mus, "mus"), M._f32(pis, "pis")
        sg = torch.broadcast_to(M._f32(sigs, "sigs"), (k, d)).contiguous()
        a = torch.empty((rows, k), dtype=torch.float32, device=x.device) if want_a else None
        arg = torch.empty((rows,), dtype=torch.int32, device=x.device) if want_arg else None
        if rows > 0:
            check(_lib.load().d3p_gmm_assign(stream_ptr(), ptr(x), rows, d, ptr(mu), ptr(sg), ptr(pi), k, ptr(a), ptr(arg)))
    return a, arg


def assignment_log_posterior(obs, mus, sigs, pis):
    """``a[r, j] = log pis_j + sum_c log N(obs[r, c]; mus[j, c], sigs[j, c])``, unnormalised: the reference's
    ``compute_assignment_log_posterior`` (:113-128) as it returns it, ``(rows, k)`` float32 on the GPU.  The direct form
    ``((x - mu) / sig)^2`` in float32.  A NaN anywhere in a row makes the whole row NaN."""
    return _run_assign(obs, mus, sigs, pis, True, False)[0]


def assign(obs, mus, sigs, pis):
    """``argmax_j`` of ``assignment_log_posterior``'s rows, the first maximum on ties, as ``(rows,)`` int32 -- without writing the
    ``(rows, k)`` array.  A row with a NaN gets -1."""
    return _run_assign(obs, mus, sigs, pis, False, True)[1]


def inverse_mode_map(mode_map, k):
    """The reference's inverse map (:142-146): the identity as a base, then ``inv[mode_map[j]] = j`` for j = 0 .. k - 1 in order, so a
    learned component claimed by two true modes stands for the later one and an unclaimed one for itself.  Pure host logic."""
    inv = {j: j for j in range(k)}
    inv.update({int(mode_map[j]): j for j in range(k)})
    return inv


def compute_assignment_accuracy(X_test, original_assignment, original_modes, posterior_modes, posterior_pis):
    """The reference's ``compute_assignment_accuracy`` (:130-161): the true modes are assigned to learned components by the
    log-posterior with unit scales and the learned weights, the held-out points likewise, the points' assignments go through the
    inverse of the modes' map and are compared with the generating assignment.  Returns a Python float."""
    k, d = _shape_of(original_modes)
    ones = torch.ones((k, d), dtype=torch.float32)
    mode_map = assign(original_modes, posterior_modes, ones, posterior_pis).cpu().tolist()
    inv = inverse_mode_map(mode_map, k)
    post = assign(X_test, posterior_modes, ones, posterior_pis)
    table = torch.tensor([inv.get(j, j) for j in range(max(k, int(_shape_of(posterior_modes)[0])))], dtype=torch.int64, device=post.device)
    remapped = torch.where(post >= 0, table[post.clamp(min=0).long()], torch.full_like(post, -1, dtype=torch.int64))
    truth = torch.as_tensor(original_assignment).to(post.device).long()
    return float((truth == remapped).float().mean())

"""Prior and posterior predictive sampling: mirror of ``d3p.modelling`` (reference d3p/modelling.py:39-223).

The reference traces numpyro model / guide functions under ``seed`` / ``substitute`` handlers.  numpyro is not importable in
this build, so the model and guide are the declared objects of ``d3p_amd.models`` and each family's trace is a
SITE PLAN (``site_plan``): which sample sites there are, in program order, under which seed handler, and which of them take a
key.  The draws themselves run on the GPU (``d3p_amd/csrc/d3p_predict.hip``), where each restated numpyro / jax rule lives in
one device function (unpinned like the rest of numpyro's key plumbing).

``rng_key`` is a threefry (jax) key -- a (2,) 32-bit CUDA tensor, as ``d3p_amd.random.debug.PRNGKey`` or
``rng_suite.convert_to_jax_rng_key`` make it -- as in the reference, which takes a jax key here.  Results are dicts from site
name to CUDA tensors; the multi forms add a leading ``n`` axis to every site.

Not mirrored: ``get_samples_from_trace``, ``make_observed_model`` and ``map_args_obs_to_shape`` operate on
numpyro traces and handlers, which this build does not have.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .models import (AutoDiagonalNormal, DiagonalNormalGuide, GaussianMean, GaussianMixtureModel, LogisticRegression,
                     MeanFieldGuide, VAEGuide, VAEModel)

__all__ = ["sample_prior_predictive", "sample_posterior_predictive", "sample_multi_prior_predictive",
           "sample_multi_posterior_predictive", "site_plan", "Site"]

# One sample site of a family's trace.  chain: "model" or "guide" (the seed handler it runs under); key_index: how many
# key-taking sample statements precede it under that handler (None: it takes no key -- substituted or observed);
# substituted: its value comes from `substitutes` / the guide's draw / the observed data.
Site = namedtuple("Site", ["name", "size", "chain", "key_index", "substituted"])


def _latent_layout(d, intercept):
    """Where the latent sites sit in a row of the (n, D) latent buffer: (w columns, intercept column or None).  This is also the
    unpacking of AutoDiagonalNormal's `_auto_latent` (columns 0 .. d - 1 are `w`, column d the intercept: the order the rest of
    this repository uses, examples/logistic_regression.py and the kernels with an intercept).  VERDICT.md questions that order;
    settling it is an edit of this function alone."""
    return slice(0, d), (d if intercept else None)


def _model_sites(model, d, rows, B=None, Z=None, D=None):
    """[(name, size)] of the model's sample statements in program order (the plate of size == subsample size takes no key)."""
    if isinstance(model, LogisticRegression):
        return [("w", d)] + ([("intercept", 1)] if model.intercept else []) + [("obs", rows)]
    if isinstance(model, GaussianMean):
        return [("mu", d), ("obs", rows * d)]
    if isinstance(model, VAEModel):
        return [("z", B * Z), ("obs", B * D)]     # numpyro.module with its parameters given takes no key
    raise TypeError(f"no site plan for model {type(model).__name__}")


def _guide_sites(guide, model, d, B=None, Z=None):
    """[(name, size)] of the guide's key-taking sample statements in program order."""
    D = d + (1 if getattr(model, "intercept", False) else 0)
    if isinstance(guide, AutoDiagonalNormal):
        # the unpacked sites after `_auto_latent` are Delta sites; nothing samples under the guide's handler after them
        return [("_auto_latent", D)]
    if isinstance(guide, MeanFieldGuide):
        return list(guide.sites(d))
    if isinstance(guide, DiagonalNormalGuide):
        return [(guide.site, D)]
    if isinstance(guide, VAEGuide):
        return [("z", B * Z)]
    raise TypeError(f"no site plan for guide {type(guide).__name__}")


def site_plan(model, guide=None, substituted=(), *, d=None, rows=None, B=None, Z=None, D=None):
    """The family's trace as a list of Site, guide sites first (posterior) then the model's.  Pure host logic.

    Prior (guide None): every model site takes the next key of the model's handler unless it is in `substituted`.
    Posterior: the guide's sites take the guide handler's keys; the model's latent sites are substituted by the guide's draws
    (sample_posterior_predictive substitutes the guide samples into the model, modelling.py:119-124) and its `obs` takes the
    model handler's next key unless it is in `substituted` (observed)."""
    substituted = set(substituted)
    plan = []
    if guide is not None:
        k = 0
        for name, size in _guide_sites(guide, model, d, B, Z):
            plan.append(Site(name, size, "guide", k, False))
            k += 1
        substituted |= {name for name, _ in _model_sites(model, d, rows or 1, B, Z, D or 1) if name != "obs"}
    k = 0
    for name, size in _model_sites(model, d, rows, B, Z, D):
        if name in substituted:
            plan.append(Site(name, size, "model", None, True))
        else:
            plan.append(Site(name, size, "model", k, False))
            k += 1
    return plan


# ------------------------------------------------------------------------------------------------ argument handling
def _check_key(rng_key):
    if not (isinstance(rng_key, torch.Tensor) and rng_key.is_cuda and rng_key.numel() == 2 and rng_key.element_size() == 4
            and rng_key.dtype in (torch.uint32, torch.int32)):
        raise TypeError("rng_key must be a threefry (jax) key: a (2,) 32-bit CUDA tensor (d3p_amd.random.debug.PRNGKey or "
                        "rng_suite.convert_to_jax_rng_key)")
    return rng_key.contiguous()


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _f32(x, what):
    """float32, contiguous, on the current GPU (torch tensors, numpy arrays and Python numbers)."""
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        try:
            t = torch.as_tensor(np.asarray(x, dtype=np.float32))
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: not an array of numbers") from e
    if t.is_complex():
        raise ValueError(f"{what}: complex values")
    return t.to(device=_device(), dtype=torch.float32).contiguous()


def _numel(x):
    return int(x.numel()) if isinstance(x, torch.Tensor) else int(np.size(x))


def _rows_of(x, what):
    shp = tuple(x.shape)
    if len(shp) != 2:
        raise ValueError(f"{what}: a 2-D array (rows, d) is required, got shape {shp}")
    return shp


def _num_obs_total(kwargs, default=None):
    for k in ("num_obs_total", "N"):
        if kwargs.get(k) is not None:
            return int(kwargs[k])
    return default


def _check_plate(total, rows):
    if total is not None and int(total) != int(rows):
        raise NotImplementedError(f"num_obs_total = {total} differs from the {rows} rows: numpyro's plate would subsample and consume a "
                                  "key; predictive sampling here covers full plates only")


def _reject_unsupported(model):
    if isinstance(model, GaussianMixtureModel):
        raise NotImplementedError("GaussianMixtureModel: predictive sampling needs the guide's Dirichlet and InverseGamma draws and "
                                  "GaussianMixture.sample's categorical on the device -- a follow-up (DESIGN.md section 9)")
    if not isinstance(model, (LogisticRegression, GaussianMean, VAEModel)):
        raise TypeError(f"predictive sampling: unsupported model {type(model).__name__}")


def _param(params, name, size):
    if not isinstance(params, dict) or name not in params:
        raise ValueError(f"params: '{name}' is missing")
    v = params[name]
    if _numel(v) != size:
        raise ValueError(f"params['{name}']: {size} values expected, got {_numel(v)}")
    return v


def _guide_param_names(guide, model, d):
    """[(param name, size, role)] the guide reads; role: loc / scale of a guide site."""
    D = d + (1 if getattr(model, "intercept", False) else 0)
    if isinstance(guide, AutoDiagonalNormal):
        return [("auto_loc", D), ("auto_scale", D)]
    if isinstance(guide, DiagonalNormalGuide):
        return [(guide.site + "_loc", D), (guide.site + "_std_log", D)]
    if isinstance(guide, MeanFieldGuide):
        return [("w_loc", d), ("w_std_log", d), ("intercept_loc", 1), ("intercept_std_log", 1)]
    raise TypeError(f"predictive sampling: unsupported guide {type(guide).__name__} for {type(model).__name__}")


def _check_guide(model, guide):
    ok = {LogisticRegression: (AutoDiagonalNormal, DiagonalNormalGuide, MeanFieldGuide),
          GaussianMean: (AutoDiagonalNormal, DiagonalNormalGuide),
          VAEModel: (VAEGuide,)}
    for m, gs in ok.items():
        if isinstance(model, m):
            if not isinstance(guide, gs):
                raise TypeError(f"predictive sampling: guide {type(guide).__name__} is not supported with {m.__name__}")
            return


# ------------------------------------------------------------------------------------------------ family parsing
def _logreg_shape(model, model_args, kwargs):
    if len(model_args) < 1 or model_args[0] is None:
        raise ValueError("LogisticRegression: model_args = (X,) with X of shape (rows, d)")
    rows, d = _rows_of(model_args[0], "X")
    if model.d is not None and int(model.d) != d:
        raise ValueError(f"X has {d} columns, the model {model.d}")
    total = _num_obs_total(kwargs, model_args[2] if len(model_args) >= 3 else None)
    _check_plate(total, rows)
    if rows < 1 or d < 1:
        raise ValueError("X: at least one row and one column")
    return rows, d


def _gauss_shape(model, model_args, kwargs):
    obs = model_args[0] if len(model_args) >= 1 else None
    total = _num_obs_total(kwargs, model_args[1] if len(model_args) >= 2 else None)
    if obs is not None:
        rows, d = _rows_of(obs, "obs")
        _check_plate(total, rows)
    else:
        if total is None:
            raise ValueError("GaussianMean: model_args = (obs_or_None, num_obs_total[, d]); without obs, num_obs_total is required")
        rows = int(total)
        d = kwargs.get("d") or (model_args[2] if len(model_args) >= 3 else None) or model.d
        if d is None:
            raise ValueError("GaussianMean: the dimension d is needed when obs is None (model_args[2] or GaussianMean(d=))")
        d = int(d)
    if rows < 1 or d < 1:
        raise ValueError("GaussianMean: at least one row and one dimension")
    return rows, d, obs


def _vae_dims(model, model_args, kwargs):
    """(B, batch or None, Z, H, H2, D) from (batch_or_batch_size, z_dim, hidden_dim, out_dim) and the VAEModel attributes."""
    a = list(model_args) + [None] * (4 - len(model_args))
    first, z, h, D = a[0], a[1] or kwargs.get("z_dim"), a[2] or kwargs.get("hidden_dim"), a[3] or kwargs.get("out_dim")
    z = z or model.z_dim
    h = h or model.hidden_dim
    h2 = model.hidden_dim2
    if isinstance(h, (tuple, list)):
        h, h2 = h[0], (h[1] if len(h) > 1 else h2)
    batch = None
    if isinstance(first, (int, np.integer)):
        B = int(first)
    elif first is not None:
        batch = first
        B = int(first.shape[0])
        D = int(np.prod(tuple(first.shape[1:])))
    else:
        raise ValueError("VAEModel: model_args[0] must be a batch or a batch size")
    if z is None or h is None or D is None:
        raise ValueError("VAEModel: z_dim, hidden_dim and out_dim must be given (arguments or VAEModel attributes)")
    _check_plate(_num_obs_total(kwargs), B)
    if B < 1:
        raise ValueError("VAEModel: batch size >= 1")
    return B, batch, int(z), int(h), int(h2 or 0), int(D)


def _vae_flat_params(tree_or_flat, vm, which):
    """The flat parameter vector of the VAE (d3p_vae_model's layout: decoder leaves, then encoder leaves and heads).  `tree_or_flat`:
    {'decoder$params': .., 'encoder$params': ..} as DPSVI.get_params returns it (either tree may be missing when `which` does not
    need it: its part is zero) or the flat vector itself."""
    shapes, n_dec = _vae_leaf_shapes(vm)
    P = sum(int(np.prod(s)) for s in shapes)
    if isinstance(tree_or_flat, dict):
        parts = []
        for key, lo, hi in (("decoder$params", 0, n_dec), ("encoder$params", n_dec, len(shapes))):
            want = sum(int(np.prod(s)) for s in shapes[lo:hi])
            if key in tree_or_flat:
                leaves = [x for x in _tree_leaves(tree_or_flat[key])]
                if [tuple(x.shape) for x in leaves] != [tuple(s) for s in shapes[lo:hi]]:
                    raise ValueError(f"params['{key}']: leaf shapes {[tuple(x.shape) for x in leaves]} do not match the network "
                                     f"{[tuple(s) for s in shapes[lo:hi]]}")
                parts += [_f32(x, key).reshape(-1) for x in leaves]
            elif key in which:
                raise ValueError(f"params: '{key}' is missing")
            else:
                parts.append(torch.zeros(want, dtype=torch.float32, device=_device()))
        return torch.cat(parts)
    if _numel(tree_or_flat) != P:
        raise ValueError(f"VAE params: {P} values expected, got {_numel(tree_or_flat)}")
    return _f32(tree_or_flat, "params").reshape(-1)


def _vae_leaf_shapes(vm):
    """Leaf shapes of the VAE's parameter trees in tree_flatten order and how many belong to the decoder (DPSVI._vae_tree)."""
    hs = [vm.H] + ([vm.H2] if vm.H2 else [])
    dec_dims, enc_dims = [vm.Z] + hs[::-1] + [vm.D], [vm.D] + hs
    shapes = []
    for i, o in zip(dec_dims[:-1], dec_dims[1:]):
        shapes += [(i, o), (o,)]
    n_dec = len(shapes)
    for i, o in zip(enc_dims[:-1], enc_dims[1:]):
        shapes += [(i, o), (o,)]
    return shapes + [(hs[-1], vm.Z), (vm.Z,), (hs[-1], vm.Z), (vm.Z,)], n_dec


def _tree_leaves(t):
    """jax.tree_util.tree_leaves for the nested lists / tuples of stax.serial (empty tuples are parameter-free layers)."""
    if isinstance(t, (list, tuple)):
        out = []
        for x in t:
            out += _tree_leaves(x)
        return out
    if isinstance(t, dict):
        out = []
        for k in sorted(t):
            out += _tree_leaves(t[k])
        return out
    return [t]


# ------------------------------------------------------------------------------------------------ the sampler
def _draw_sites(key, n, multi, posterior, sites, obs_site, latent_cols, dev):
    """One d3p_predict_draws launch: sites = [(Site, loc tensor or None, scale tensor or None, scale_kind, loc_c, scale_c, value)];
    returns (latent (n, latent_cols), obs keys (n, 2) or None)."""
    lib = _lib.load()
    latent = torch.empty((n, max(latent_cols, 1)), dtype=torch.float32, device=dev)
    arr = (_lib.PredictSite * max(len(sites), 1))()
    keep = []
    off = 0
    for j, (st, loc, scale, kind, loc_c, scale_c, value) in enumerate(sites):
        keep += [loc, scale, value]
        arr[j] = _lib.PredictSite(st.size, off, 1 if st.chain == "guide" else 0, -1 if st.key_index is None else st.key_index,
                                  kind, float(loc_c), float(scale_c), ptr(loc).value, ptr(scale).value, ptr(value).value)
        off += st.size
    obs_keys = None
    obs_chain, obs_index = 0, 0
    if obs_site is not None and obs_site.key_index is not None:
        obs_keys = torch.empty((n, 2), dtype=torch.uint32, device=dev)
        obs_chain, obs_index = (1 if obs_site.chain == "guide" else 0), obs_site.key_index
    check(lib.d3p_predict_draws(stream_ptr(), ptr(key), n, int(multi), int(posterior), arr, len(sites), obs_chain, obs_index,
                                ptr(latent), latent.shape[1], ptr(obs_keys)))
    return latent, obs_keys


def _predict(rng_key, n, model, model_args, guide, guide_args, params, substitutes, with_intermediates, kwargs):
    """Single form when n is None, else the multi form with a leading n axis."""
    _reject_unsupported(model)
    posterior = guide is not None
    if posterior:
        _check_guide(model, guide)
    substitutes = dict(substitutes or {})
    multi = n is not None
    nn = int(n) if multi else 1
    if nn < 1:
        raise ValueError("n must be >= 1")
    if isinstance(model, VAEModel):
        out = _predict_vae(rng_key, nn, multi, model, model_args, guide, guide_args, params, substitutes, kwargs)
    else:
        out = _predict_latent_family(rng_key, nn, multi, model, model_args, guide, params, substitutes, kwargs)
    if not multi:
        out = {k: v[0] for k, v in out.items()}
    if with_intermediates:
        out = {k: (v, []) for k, v in out.items()}   # Normal and Bernoulli sites have no intermediates in numpyro
    return out


def _predict_latent_family(rng_key, n, multi, model, model_args, guide, params, substitutes, kwargs):
    posterior = guide is not None
    if isinstance(model, LogisticRegression):
        rows, d = _logreg_shape(model, model_args, kwargs)
        observed = None
    else:
        rows, d, observed = _gauss_shape(model, model_args, kwargs)
    # validate everything before the device is touched
    gparams = []
    if posterior:
        if not isinstance(params, dict):
            raise ValueError("params: the dict DPSVI.get_params returns is required")
        gparams = [(name, _param(params, name, size)) for name, size in _guide_param_names(guide, model, d)]
    model_names = [nm for nm, _ in _model_sites(model, d, rows)]
    for k in substitutes:
        if k not in model_names:
            raise ValueError(f"substitutes: '{k}' is not a sample site of {type(model).__name__} ({model_names})")
    subst = set(substitutes)
    if observed is not None:
        subst.add("obs")
    plan = site_plan(model, guide, subst, d=d, rows=rows)
    for st in plan:
        if st.substituted and st.name in substitutes and _numel(substitutes[st.name]) != st.size:
            raise ValueError(f"substitutes['{st.name}']: {st.size} values expected, got {_numel(substitutes[st.name])}")
    key = _check_key(rng_key)   # (last of the checks: everything above runs without a device)
    _lib.require_device()
    dev = key.device
    with torch.cuda.device(dev):
        gp = {name: _f32(v, f"params['{name}']") for name, v in gparams}
        latent_sites = []   # the sites the kernel writes: [(Site, loc, scale, kind, loc_c, scale_c, value)]
        if posterior:
            loc_name, sc_name = {AutoDiagonalNormal: ("auto_loc", "auto_scale")}.get(type(guide), (None, None))
            kind = _lib.D3P_PREDICT_SCALE_GIVEN if isinstance(guide, AutoDiagonalNormal) else _lib.D3P_PREDICT_SCALE_EXP
            for st in plan:
                if st.chain != "guide":
                    continue
                if isinstance(guide, MeanFieldGuide):
                    loc, sc = gp[st.name + "_loc"], gp[st.name + "_std_log"]
                elif isinstance(guide, DiagonalNormalGuide):
                    loc, sc = gp[guide.site + "_loc"], gp[guide.site + "_std_log"]
                else:
                    loc, sc = gp[loc_name], gp[sc_name]
                latent_sites.append((st, loc, sc, kind, 0.0, 1.0, None))
        else:
            for st in plan:
                if st.name == "obs":
                    continue
                prior = model.intercept_prior_scale if st.name == "intercept" else model.prior_scale
                value = _f32(substitutes[st.name], f"substitutes['{st.name}']").reshape(-1) if st.substituted else None
                latent_sites.append((st, None, None, _lib.D3P_PREDICT_SCALE_CONST, 0.0, prior, value))
        obs_site = next(st for st in plan if st.name == "obs")
        D_lat = sum(st.size for st, *_ in latent_sites)
        latent, obs_keys = _draw_sites(key, n, multi, posterior, latent_sites, obs_site, D_lat, dev)
        out = {}
        off = 0
        for st, *_ in latent_sites:
            out[st.name] = latent[:, off:off + st.size]
            off += st.size
        # the model's view of the latent row: w / intercept (logistic regression) or mu -- views, no copies
        if isinstance(model, LogisticRegression):
            if posterior and not isinstance(guide, MeanFieldGuide):   # one guide site over [w | intercept]
                w_cols, b_idx = _latent_layout(d, model.intercept)
                out["w"] = latent[:, w_cols]
                if b_idx is not None:
                    out["intercept"] = latent[:, b_idx]
            elif model.intercept:
                out["intercept"] = out["intercept"].reshape(n)
            w_off = out["w"].storage_offset() - latent.storage_offset()
            b_col = (out["intercept"].storage_offset() - latent.storage_offset()) if model.intercept else -1
        elif posterior:
            out["mu"] = latent[:, :d]
        if obs_site.substituted:
            val = observed if observed is not None else substitutes["obs"]
            o = torch.as_tensor(val).to(dev)
            out["obs"] = o.reshape((1,) + tuple(o.shape)).expand((n,) + tuple(o.shape))
        elif isinstance(model, LogisticRegression):
            X = _f32(model_args[0], "X")
            obs = torch.empty((n, rows), dtype=torch.int32, device=dev)
            check(_lib.load().d3p_predict_logreg(stream_ptr(), ptr(X), rows, d, ptr(latent), latent.shape[1], w_off, b_col, n,
                                                 ptr(obs_keys), ptr(obs)))
            out["obs"] = obs
        else:
            obs = torch.empty((n, rows, d), dtype=torch.float32, device=dev)
            mu = out["mu"]
            check(_lib.load().d3p_predict_gauss(stream_ptr(), ptr(mu), latent.shape[1], d, rows, n, float(model.obs_scale),
                                                ptr(obs_keys), ptr(obs)))
            out["obs"] = obs
        return out


def _predict_vae(rng_key, n, multi, model, model_args, guide, guide_args, params, substitutes, kwargs):
    from ._lib import VaeModel
    posterior = guide is not None
    B, batch, Z, H, H2, D = _vae_dims(model, model_args, kwargs)
    if batch is not None:
        raise NotImplementedError("VAEModel with an observed batch: the 'obs' site would be observed; pass the batch size instead "
                                  "(examples/vae.py:294)")
    vm = VaeModel(D, H, Z, 1.0, 1.0, H2)
    for k in substitutes:
        if k not in ("z", "obs", "decoder$params"):
            raise ValueError(f"substitutes: '{k}' is not a site of VAEModel (z, obs) nor 'decoder$params'")
    X = None
    if posterior:
        if not guide_args or guide_args[0] is None:
            raise ValueError("VAEGuide: guide_args = (batch, z_dim, hidden_dim)")
        X = guide_args[0]
        if int(X.shape[0]) != B or int(np.prod(tuple(X.shape[1:]))) != D:
            raise ValueError(f"VAEGuide: the guide's batch has shape {tuple(X.shape)}, the model expects {B} images of {D} values")
        if params is None:
            raise ValueError("params: the dict DPSVI.get_params returns is required")
        flat = _vae_flat_params(params, vm, ("decoder$params", "encoder$params"))
    else:
        src = dict(params or {})
        src.update({k: v for k, v in substitutes.items() if k == "decoder$params"})
        if "decoder$params" not in src:
            raise ValueError("VAEModel prior predictive: the decoder's weights come in through substitutes['decoder$params']")
        flat = _vae_flat_params({"decoder$params": src["decoder$params"]}, vm, ("decoder$params",))
    z_sub = substitutes.get("z")
    if z_sub is not None and _numel(z_sub) != B * Z:
        raise ValueError(f"substitutes['z']: {B * Z} values expected")
    if posterior and z_sub is not None:
        raise ValueError("substitutes are a prior-predictive argument")
    key = _check_key(rng_key)
    _lib.require_device()
    lib = _lib.load()
    dev = key.device
    with torch.cuda.device(dev):
        flat = flat.to(dev)
        Xd = _f32(X, "batch").reshape(B, D) if posterior else None
        zs = _f32(z_sub, "substitutes['z']").reshape(-1) if z_sub is not None else None
        z = torch.empty((n, B, Z), dtype=torch.float32, device=dev)
        obs = torch.empty((n, B, D), dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.d3p_predict_vae_workspace(C.byref(vm), B, n)), dtype=torch.uint8, device=dev)
        check(lib.d3p_predict_vae(stream_ptr(), C.byref(vm), ptr(flat), ptr(Xd), B, ptr(key), n, int(multi), ptr(zs), ptr(z), ptr(obs),
                                  ptr(ws), ws.numel()))
        out = {"z": z, "obs": obs}
        if "obs" in substitutes:
            o = torch.as_tensor(substitutes["obs"]).to(dev)
            out["obs"] = o.reshape((1,) + tuple(o.shape)).expand((n,) + tuple(o.shape))
        return out


# ------------------------------------------------------------------------------------------------ public API (modelling.py:39-223)
def sample_prior_predictive(rng_key, model, model_args, substitutes=None, with_intermediates=False, **kwargs):
    """d3p/modelling.py:39-78: one draw from the prior predictive; `substitutes` freezes sites to given values."""
    return _predict(rng_key, None, model, model_args, None, None, None, substitutes, with_intermediates, kwargs)


def sample_posterior_predictive(rng_key, model, model_args, guide, guide_args, params, with_intermediates=False, **kwargs):
    """d3p/modelling.py:81-131: one draw from the posterior predictive; `params` as DPSVI.get_params returns them."""
    return _predict(rng_key, None, model, model_args, guide, guide_args, params, None, with_intermediates, kwargs)


def sample_multi_prior_predictive(rng_key, n, model, model_args, substitutes=None, with_intermediates=False, **kwargs):
    """d3p/modelling.py:139-180: n draws (draw i from split(rng_key, n)[i]), a leading n axis on every site."""
    return _predict(rng_key, int(n), model, model_args, None, None, None, substitutes, with_intermediates, kwargs)


def sample_multi_posterior_predictive(rng_key, n, model, model_args, guide, guide_args, params, with_intermediates=False, **kwargs):
    """d3p/modelling.py:183-223: n posterior-predictive draws, a leading n axis on every site."""
    return _predict(rng_key, int(n), model, model_args, guide, guide_args, params, None, with_intermediates, kwargs)

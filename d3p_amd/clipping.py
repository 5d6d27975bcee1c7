"""Clipping diagnostics: the per-example gradient norms of a whole table and their profile against clipping thresholds (DESIGN.md
section 4n).

    gradient_norms(svi, svi_state, X, y, rng_key=None, return_losses=False, slab_bytes=64 << 20)  -> (N,) float32 on the GPU
    clipping_profile(svi, svi_state, X, y, thresholds=None, probs=(0.5, 0.9, 0.95, 0.99), rng_key=None) -> ClippingProfile
    norm_profile(norms, thresholds, probs)                                                        -> ClippingProfile
    suggest_clipping_threshold(profile, prob=0.5)                                                 -> float

PRIVACY.  Every number here is computed from the PRIVATE table, without noise.  Releasing a profile, or choosing the clipping
threshold ``C`` by looking at it, is NOT covered by the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps
of training and nothing else.  Tune ``C`` on public or synthetic data of the same shape, or account for the release of the profile
separately.  The functions are a diagnostic for the person who holds the data.

Every DP-VI step is "per-example gradient -> joint L2 clip at C -> sum -> noise proportional to dp_scale C".
``gradient_norms`` returns the norms that step clips, at the parameters of ``svi_state``, for every row of the table taken as ONE
batch of ``N`` rows without a mask: ``norms[r]`` is the float32 L2 norm over all ``2 D`` entries of row ``r`` of what
``svi._compute_per_example_gradients(svi_state, rng_key, X, y)`` returns, with the same model struct (``observation_scale``,
``lik_scale = num_obs_total``) and the same guide draw (keyed by the row's position in the table), computed by
``d3p_logreg_grad_norms`` (``d3p_amd/csrc/d3p_grad_norms.hip``) without the ``N x 2 D`` tensor.  ``svi`` is a ``DPSVI`` over
``LogisticRegression``, ``LinearRegression`` or ``PoissonRegression`` with ``AutoDiagonalNormal``, ``DiagonalNormalGuide`` or
(logistic only) ``MeanFieldGuide``, one particle, ``d <= 2048``.  ``rng_key`` is a key of the ``svi``'s ``rng_suite``; the default is
the gradient key the next ``svi.update`` from ``svi_state`` would use.  ``svi_state`` is read and never advanced.  With
``return_losses=True`` the result is ``(norms, losses)``, the per-example losses of the same call.

``MeanFieldGuide`` draws every sample site from its own key: its eps is written per row slab by ``d3p_px_eps_sites`` -- at most
``slab_bytes`` of it alive at a time -- and read by the kernel; the result does not depend on ``slab_bytes``.

``norm_profile`` is model-free (``d3p_norm_profile``): ``norms`` is any 1-D float32 CUDA tensor with unit stride, ``thresholds`` up to
8 finite floats > 0 and ``probs`` up to 8 floats in [0, 1].  ``ClippingProfile`` holds Python numbers only:

    n, n_nonfinite       rows, and rows whose norm is inf or NaN (the step clips those to 0)
    mean, rms, max       over the finite norms (float64 sums; NaN when there is none)
    probs, quantiles     numpy's ``method='linear'`` over the FINITE norms, on exactly selected order statistics, float32 values
    thresholds           as given
    clipped_fraction     per threshold: the share of ALL rows with norm > C (compared in float32) or a non-finite norm
    mean_clip_factor     per threshold: the mean over ALL rows of min(1, C / norm) -- 0 for a non-finite norm, 1 for a zero norm

``suggest_clipping_threshold`` returns the profile's quantile at ``prob`` (the median by default, as Abadi et al. 2016 suggest); it
is pure host code.  Every host check runs before the device is touched; there is no CPU fallback.
"""
import ctypes as C
import math
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _lib
from .intervals import positions
from ._lib import check, ptr, stream_ptr
from .models import (AutoDiagonalNormal, DiagonalNormalGuide, LinearRegression, LogisticRegression, MeanFieldGuide,
                     PoissonRegression)

__all__ = ["ClippingProfile", "gradient_norms", "clipping_profile", "norm_profile", "suggest_clipping_threshold"]

MAX_THRESHOLDS = 8
MAX_PROBS = 8
MAX_D = 2048
_OUT_WORDS = 29


class ClippingProfile(NamedTuple):
    n: int
    n_nonfinite: int
    mean: float
    rms: float
    max: float
    probs: Tuple[float, ...]
    quantiles: Tuple[float, ...]
    thresholds: Tuple[float, ...]
    clipped_fraction: Tuple[float, ...]
    mean_clip_factor: Tuple[float, ...]


def _check_thresholds(thresholds):
    try:
        ts = tuple(float(c) for c in thresholds)
    except TypeError:
        raise ValueError("thresholds: a sequence of at most 8 finite floats > 0 is required") from None
    if len(ts) > MAX_THRESHOLDS:
        raise ValueError(f"thresholds: at most {MAX_THRESHOLDS} thresholds per call, got {len(ts)}")
    for c in ts:
        with np.errstate(over="ignore"):
            c32 = float(np.float32(c))
        if not (math.isfinite(c32) and c32 > 0.0):   # (a NaN fails the comparison; the device compares in float32)
            raise ValueError(f"thresholds: every threshold must be finite and > 0 in float32, got {c!r}")
    return ts


def _check_probs(probs):
    try:
        ps = tuple(float(p) for p in probs)
    except TypeError:
        raise ValueError("probs: a sequence of at most 8 floats in [0, 1] is required") from None
    if len(ps) > MAX_PROBS:
        raise ValueError(f"probs: at most {MAX_PROBS} probabilities per call, got {len(ps)}")
    for p in ps:
        if not 0.0 <= p <= 1.0:   # (a NaN fails both comparisons)
            raise ValueError(f"probs: every probability must lie in [0, 1], got {p!r}")
    return ps


def _check_svi(svi, what):
    """The host refusals of ``gradient_norms``: model, guide, particles."""
    from .svi import DPSVI
    if not isinstance(svi, DPSVI):
        raise TypeError(f"{what}: svi must be a d3p_amd.svi.DPSVI, got {type(svi).__name__}")
    if not isinstance(svi.model, (LogisticRegression, LinearRegression, PoissonRegression)):
        raise TypeError(f"{what}: unsupported model {type(svi.model).__name__} (LogisticRegression, LinearRegression and PoissonRegression "
                        "have per-example gradient norms)")
    ok = (AutoDiagonalNormal, DiagonalNormalGuide) + ((MeanFieldGuide,) if isinstance(svi.model, LogisticRegression) else ())
    if not isinstance(svi.guide, ok):
        raise TypeError(f"{what}: guide {type(svi.guide).__name__} is not supported with {type(svi.model).__name__}")
    if svi._num_particles > 1:
        raise NotImplementedError(f"{what}: Trace_ELBO(num_particles={svi._num_particles}) is not built; one particle only")


def _check_width(d, what):
    if d > MAX_D:
        raise _lib.D3PError(f"{what}: d = {d} exceeds the kernel's limit d <= {MAX_D}")


def _slab_rows(slab_bytes, D):
    if isinstance(slab_bytes, bool) or not isinstance(slab_bytes, int) or slab_bytes < 1:
        raise ValueError(f"slab_bytes must be an int >= 1, got {slab_bytes!r}")
    return max(1, slab_bytes // (4 * D))


def gradient_norms(svi, svi_state, *model_args, rng_key=None, return_losses=False, slab_bytes=64 << 20, **kwargs):
    """The float32 L2 norms of the per-example gradients of every row of ``model_args = (X, y)`` at the parameters of ``svi_state``:
    an ``(N,)`` CUDA tensor, or ``(norms, losses)`` with ``return_losses=True`` (module docstring)."""
    from .svi import _batch_array
    what = "gradient_norms"
    _check_svi(svi, what)
    if len(model_args) < 2:
        raise ValueError(f"{what}: model_args = (X, y) is required")
    shape = np.shape(model_args[0])
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{what}: X must be (N, d) with N >= 1 and d >= 1, got shape {tuple(shape)}")
    N, d = int(shape[0]), int(shape[1])
    _check_width(d, what)
    if N > 0xffffffff:
        raise _lib.D3PError(f"{what}: N = {N} rows exceed the kernel's limit N < 2^32")
    D = svi.model.latent_dim(d)
    multi = isinstance(svi.guide, MeanFieldGuide)
    chunk = _slab_rows(slab_bytes, D) if multi else N
    _lib.require_device()   # (every check above runs without a device)
    lib = _lib.load()
    X = _batch_array(model_args[0])
    y = svi._labels(model_args)
    if rng_key is None:
        rng_key = svi._rng_suite.split(svi_state.rng_key, 3)[1]   # (next, GRADIENT, perturbation): DPSVI.update's split
    with torch.cuda.device(X.device):
        jax_key = svi._rng_suite.convert_to_jax_rng_key(rng_key).contiguous()
        params = svi.optim.get_params(svi_state.optim_state).contiguous()
        svi._require_sizes(params.numel(), 2 * D, N, y)
        model = svi._model_struct(d, kwargs, svi_state.observation_scale)
        if multi:   # tree order (four leaves) -> [loc (D) | unconstrained scale (D)] with the intercept last
            perm = MeanFieldGuide.tree_from_kernel(d, X.device)
            kern = torch.empty_like(params)
            kern[perm] = params
            params = kern
        norms = torch.empty(N, dtype=torch.float32, device=X.device)
        losses = torch.empty(N, dtype=torch.float32, device=X.device) if return_losses else None
        ws = svi._workspace(lib.d3p_logreg_grad_norms_workspace(C.byref(model), min(chunk, N)), X.device, "grad_norms")
        if not multi:
            check(lib.d3p_logreg_grad_norms(stream_ptr(), C.byref(model), ptr(params), ptr(X), ptr(y), N, 0, N, None, ptr(jax_key),
                                            ptr(norms), ptr(losses), ptr(ws), ws.numel()))
        else:
            sizes = (C.c_int32 * 2)(d, 1)
            eps = torch.empty((min(chunk, N), D), dtype=torch.float32, device=X.device)
            for lo in range(0, N, chunk):
                count = min(chunk, N - lo)
                check(lib.d3p_px_eps_sites(stream_ptr(), ptr(jax_key), N, lo, count, sizes, 2, ptr(eps)))
                check(lib.d3p_logreg_grad_norms(stream_ptr(), C.byref(model), ptr(params), ptr(X[lo:lo + count]), ptr(y[lo:lo + count]), N, lo,
                                                count, ptr(eps), None, ptr(norms[lo:]), None if losses is None else ptr(losses[lo:]),
                                                ptr(ws), ws.numel()))
    return (norms, losses) if return_losses else norms


def _profile_call(lib, norms, n, ts, pos, out, ws):
    m, Q = len(ts), len(pos)
    thr = (C.c_float * max(m, 1))(*ts)
    lo = (C.c_uint64 * max(Q, 1))(*[p[0] for p in pos])
    g = (C.c_double * max(Q, 1))(*[p[1] for p in pos])
    check(lib.d3p_norm_profile(stream_ptr(), ptr(norms), n, m, thr, Q, lo, g, ptr(out), ptr(ws), ws.numel()))
    return out.cpu()   # (waits for the stream)


def norm_profile(norms, thresholds, probs):
    """The ``ClippingProfile`` of a 1-D float32 CUDA tensor of norms against ``thresholds`` at ``probs`` (module docstring)."""
    ts = _check_thresholds(thresholds)
    ps = _check_probs(probs)
    if not isinstance(norms, torch.Tensor) or norms.dim() != 1 or norms.dtype != torch.float32 or not norms.is_cuda:
        raise ValueError("norm_profile: a 1-D float32 CUDA tensor of norms is required")
    n = int(norms.shape[0])
    if n < 1:
        raise ValueError("norm_profile: at least one norm")
    if n > 1 and norms.stride(0) != 1:
        raise ValueError("norm_profile: the norms must have unit stride")
    _lib.require_device()   # (every check above runs without a device)
    lib = _lib.load()
    with torch.cuda.device(norms.device):
        out = torch.empty(_OUT_WORDS, dtype=torch.int64, device=norms.device)
        ws = torch.empty(int(lib.d3p_norm_profile_workspace(n)), dtype=torch.uint8, device=norms.device)
        host = _profile_call(lib, norms, n, ts, [], out, ws)
        n_finite = int(host[0])
        if ps and n_finite:   # the positions are taken over the FINITE norms: their count has to be known first
            host = _profile_call(lib, norms, n, ts, positions(ps, n_finite), out, ws)
    f = host.view(torch.float64)
    m, Q = len(ts), len(ps)
    quant = tuple(float(f[21 + q]) for q in range(Q)) if n_finite else (math.nan,) * Q
    mean_sq = float(f[3])
    return ClippingProfile(n=n, n_nonfinite=int(host[1]), mean=float(f[2]), rms=math.sqrt(mean_sq) if mean_sq == mean_sq else math.nan,
                           max=float(f[4]), probs=ps, quantiles=quant, thresholds=ts,
                           clipped_fraction=tuple(int(host[5 + k]) / n for k in range(m)),
                           mean_clip_factor=tuple(float(f[13 + k]) for k in range(m)))


def clipping_profile(svi, svi_state, *model_args, thresholds=None, probs=(0.5, 0.9, 0.95, 0.99), rng_key=None, **kwargs):
    """``norm_profile(gradient_norms(svi, svi_state, *model_args, rng_key=rng_key), thresholds, probs)``; ``thresholds=None`` stands for
    the ``svi``'s own clipping threshold."""
    _check_svi(svi, "clipping_profile")
    ts = _check_thresholds((svi._clipping_threshold,) if thresholds is None else thresholds)
    ps = _check_probs(probs)
    return norm_profile(gradient_norms(svi, svi_state, *model_args, rng_key=rng_key, **kwargs), ts, ps)


def suggest_clipping_threshold(profile, prob=0.5):
    """The profile's quantile at ``prob`` as a clipping threshold (Abadi et al. 2016 take the median of the unclipped norms).
    ``prob`` must be one of ``profile.probs`` and the quantile finite and > 0 (``ValueError`` otherwise).  The suggestion is a
    function of the private table (module docstring)."""
    if not isinstance(profile, ClippingProfile):
        raise TypeError(f"suggest_clipping_threshold: a ClippingProfile is required, got {type(profile).__name__}")
    prob = float(prob)
    for p, q in zip(profile.probs, profile.quantiles):
        if p == prob:
            if not (math.isfinite(q) and q > 0.0):
                raise ValueError(f"suggest_clipping_threshold: the quantile at {prob} is {q!r}; a threshold must be finite and > 0")
            return float(q)
    raise ValueError(f"suggest_clipping_threshold: prob = {prob} is not among the profile's probs {profile.probs}")

"""Importance-weighted held-out log-likelihood of the VAE and the per-image Pareto k of its amortised guide.

    log_importance_weights(rng_key, n, model, guide, params, X, ...) -> (n, B) float32 [, sites]
    held_out_density(rng_key, n, model, guide, params, X, ..., pareto_k=True) -> VAEDensity

For draw ``i < n`` and image ``b < B`` of the held-out batch ``X``, with ``(zl_b, zs_b)`` the encoder's heads (``zs`` the log of the
guide's scale) and ``a_ib`` the decoder's output pre-activation at ``z_ib``:

    z_ib       the z ``sample_multi_posterior_predictive`` draws for (rng_key, n), bit for bit
    log_px     = sum_c x_bc a_ibc - softplus(a_ibc)                       Bernoulli(logits).log_prob
    log_pz     = sum_j -z^2 / 2 - log(2 pi) / 2
    log_qz     = sum_j -u^2 / 2 - zs_bj - log(2 pi) / 2,  u = (z_ibj - zl_bj) exp(-zs_bj)
    log_w[i,b] = log_px + log_pz - log_qz

All of it is UNSCALED: neither ``handlers.scale`` (``VAEModel.scale``) nor ``num_obs_total`` enters.  The terms are float32, their
sums float64 in a fixed order, every output rounded to float32 once (``d3p_vae_log_weights``, include/d3p_hip.h); the outputs do not
depend on how the draws are cut into slabs to fit ``max_workspace_bytes``.

``held_out_density`` reduces the columns of ``log_w`` in float64 (``d3p_col_stats``): per image the ELBO (the mean over the draws),
its between-draw variance, the importance-weighted bound ``logsumexp_i log_w - log n`` on ``log p(x_b)`` (Burda, Grosse &
Salakhutdinov 2016; >= the ELBO, equal at n = 1) and the effective sample size of the weights; and, with ``pareto_k=True``, the Pareto
shape of each image's weights (Yao, Vehtari, Simpson & Gelman 2018) from ``d3p_psis_loo`` on the negated matrix, with
``d3p_amd.diagnostics``' conventions: ``n > 65535`` raises ``ValueError``, ``n <= 20`` leaves no tail (``+inf``), a column whose draws
are all equal gives ``-inf``, a NaN column NaN.  Totals are sums over the images with ``se = sqrt(B Var_b)`` (NaN at B = 1).

Only ``VAEModel`` with ``VAEGuide`` is accepted (``TypeError`` otherwise); every host check runs before the device is touched; there
is no CPU fallback."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import modelling as M
from ._lib import check, ptr, stream_ptr
from .models import VAEGuide, VAEModel

__all__ = ["log_importance_weights", "held_out_density", "VAEDensity"]

_DEFAULT_WORKSPACE = 256 << 20


@dataclass
class VAEDensity:
    elbo: torch.Tensor              # (B,) float64: mean_i log_w[i, b]
    elbo_draw_var: torch.Tensor     # (B,) float64: sample variance over the draws (ddof 1; one draw: NaN)
    log_px_is: torch.Tensor         # (B,) float64: logsumexp_i log_w[i, b] - log n
    ess: torch.Tensor               # (B,) float64: (sum r)^2 / sum r^2, r = exp(log_w - max)
    pareto_k: Optional[torch.Tensor]  # (B,) float64, or None with pareto_k=False
    elbo_total: torch.Tensor        # 0-d float64
    elbo_total_se: torch.Tensor
    log_px_is_total: torch.Tensor
    log_px_is_total_se: torch.Tensor
    k_threshold: float              # min(1 - 1 / log10(n_draws), 0.7)
    n_high_k: Optional[torch.Tensor]  # 0-d int64: images whose k is not <= k_threshold; None with pareto_k=False
    n_draws: int
    n_images: int


def _check_pair(model, guide, what):
    if not isinstance(model, VAEModel):
        raise TypeError(f"{what}: unsupported model {type(model).__name__} (VAEModel with VAEGuide)")
    if not isinstance(guide, VAEGuide):
        raise TypeError(f"{what}: guide {type(guide).__name__} is not supported with VAEModel (VAEGuide)")


def _prepare(what, rng_key, n, model, guide, params, X, z_dim, hidden_dim, multi):
    """Every host check; returns (n, B, vm, flat parameter source, key)."""
    _check_pair(model, guide, what)
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    if not multi and n != 1:
        raise ValueError("multi=False is the single form: n must be 1")
    if X is None or len(tuple(X.shape)) < 2:
        raise ValueError("X: a batch of images (B, ...) is required")
    B = int(X.shape[0])
    D = int(np.prod(tuple(X.shape[1:])))
    B, _, Z, H, H2, D = M._vae_dims(model, (B, z_dim, hidden_dim, D), {})
    if B * n >= 2 ** 31:
        raise ValueError(f"n B = {B * n}: n B < 2^31 is required")
    if params is None:
        raise ValueError("params: the dict DPSVI.get_params returns is required")
    vm = _lib.VaeModel(D, H, Z, 1.0, 1.0, H2)
    key = M._check_key(rng_key)
    return n, B, vm, key


def _draws_per_slab(lib, vm, B, n, max_workspace_bytes):
    """The largest draws_per_slab in [1, n] whose workspace fits the byte cap (1 when none does)."""
    size = lambda k: int(lib.d3p_vae_log_weights_workspace(C.byref(vm), B, k))   # noqa: E731
    lo, hi = 1, n
    if size(hi) <= max_workspace_bytes:
        return hi
    while lo < hi:   # size is monotone in the slab
        mid = (lo + hi + 1) // 2
        if size(mid) <= max_workspace_bytes:
            lo = mid
        else:
            hi = mid - 1
    return lo


def log_importance_weights(rng_key, n, model, guide, params, X, *, z_dim=None, hidden_dim=None, multi=True, return_sites=False,
                           max_workspace_bytes=_DEFAULT_WORKSPACE, draws_per_slab=None):
    """``(n, B)`` float32 log importance weights of ``n`` guide draws per image of ``X`` (module docstring); ``params`` as
    ``DPSVI.get_params`` returns them (or the flat vector), ``rng_key`` a threefry (jax) key as for ``d3p_amd.modelling``.  With
    ``return_sites`` also a dict ``{"z": (n, B, Z), "log_px", "log_pz", "log_qz": (n, B)}`` (float32).  ``draws_per_slab`` overrides
    the slab picked from ``max_workspace_bytes``; the result does not depend on either."""
    n, B, vm, key = _prepare("log_importance_weights", rng_key, n, model, guide, params, X, z_dim, hidden_dim, multi)
    if draws_per_slab is not None and int(draws_per_slab) < 1:
        raise ValueError("draws_per_slab must be >= 1")
    flat = M._vae_flat_params(params, vm, ("decoder$params", "encoder$params"))
    _lib.require_device()
    lib = _lib.load()
    dev = key.device
    with torch.cuda.device(dev):
        flat = flat.to(dev)
        Xd = M._f32(X, "X").reshape(B, vm.D)
        dps = int(draws_per_slab) if draws_per_slab is not None else _draws_per_slab(lib, vm, B, n, int(max_workspace_bytes))
        dps = min(dps, n)
        z = torch.empty((n, B, vm.Z), dtype=torch.float32, device=dev)
        logw = torch.empty((n, B), dtype=torch.float32, device=dev)
        parts = torch.empty((3, n, B), dtype=torch.float32, device=dev) if return_sites else None
        ws = torch.empty(int(lib.d3p_vae_log_weights_workspace(C.byref(vm), B, dps)), dtype=torch.uint8, device=dev)
        check(lib.d3p_vae_log_weights(stream_ptr(), C.byref(vm), ptr(flat), ptr(Xd), B, ptr(key), n, int(bool(multi)), dps, ptr(z), ptr(logw),
                                      ptr(parts), ptr(ws), ws.numel()))
    if return_sites:
        return logw, {"z": z, "log_px": parts[0], "log_pz": parts[1], "log_qz": parts[2]}
    return logw


def col_stats(m):
    """(mean, var, lse, ess), each ``(cols,)`` float64, of the columns of the float32 ``(draws, cols)`` matrix ``m`` (rows may be
    strided: a leading dimension): ``d3p_col_stats``."""
    if m.dim() != 2 or m.dtype != torch.float32 or not m.is_cuda or (m.shape[1] > 1 and m.stride(1) != 1):
        raise ValueError("col_stats: a float32 CUDA matrix (draws, cols) with unit column stride is required")
    n, cols = int(m.shape[0]), int(m.shape[1])
    if n < 1:
        raise ValueError("col_stats: at least one draw")
    ld = int(m.stride(0)) if n > 1 else cols
    out = torch.empty((4, cols), dtype=torch.float64, device=m.device)
    with torch.cuda.device(m.device):
        check(_lib.load().d3p_col_stats(stream_ptr(), ptr(m), ld, n, cols, ptr(out)))
    return out[0], out[1], out[2], out[3]


def _pareto_k(logw, n, B):
    """(B,) float64: d3p_psis_loo's k_rows on the negated matrix, with diagnostics.py's conventions for the degenerate columns."""
    neg = (-logw).contiguous()
    out = torch.empty((3, B), dtype=torch.float32, device=logw.device)
    check(_lib.load().d3p_psis_loo(stream_ptr(), ptr(neg), B, n, B, ptr(out[0]), ptr(out[1]), ptr(out[2])))
    k = out[2].to(torch.float64)
    if n >= 2:
        mx, mn = logw.max(dim=0).values, logw.min(dim=0).values
        k = torch.where((mx == mn) & torch.isfinite(mx), torch.full_like(k, -math.inf), k)   # every weight equal: no tail at all
    return k


def _total_and_se(v):
    B = v.shape[0]
    total = v.sum()
    se = torch.sqrt(B * v.var(correction=1)) if B > 1 else torch.full_like(total, math.nan)
    return total, se


def held_out_density(rng_key, n, model, guide, params, X, *, z_dim=None, hidden_dim=None, multi=True, pareto_k=True,
                     max_workspace_bytes=_DEFAULT_WORKSPACE, draws_per_slab=None):
    """Per-image ELBO, importance-weighted bound on ``log p(x)``, effective sample size and Pareto k of ``n`` guide draws per image of
    the held-out batch ``X``: a ``VAEDensity`` (module docstring).  Arguments as for ``log_importance_weights``."""
    from .criteria import _k_threshold
    _check_pair(model, guide, "held_out_density")
    if pareto_k and int(n) > 65535:
        raise ValueError(f"{int(n)} draws: the Pareto fit (d3p_psis_loo) runs at most 65535 draws (n <= 65535, or pareto_k=False)")
    logw = log_importance_weights(rng_key, n, model, guide, params, X, z_dim=z_dim, hidden_dim=hidden_dim, multi=multi,
                                  max_workspace_bytes=max_workspace_bytes, draws_per_slab=draws_per_slab)
    n, B = int(logw.shape[0]), int(logw.shape[1])
    thr = _k_threshold(n)
    with torch.cuda.device(logw.device):
        mean, var, lse, ess = col_stats(logw)
        k = _pareto_k(logw, n, B) if pareto_k else None
        high = torch.logical_not(k <= thr).sum() if pareto_k else None
        et, ese = _total_and_se(mean)
        lt, lse_se = _total_and_se(lse)
    return VAEDensity(mean, var, lse, ess, k, et, ese, lt, lse_se, thr, high, n, B)

"""Whole-table log joint, ELBO and the PSIS Pareto-k diagnostic of the Gaussian mixture model's guide: the
mixture's counterpart of ``d3p_amd.diagnostics``, which keeps refusing ``GaussianMixtureModel`` -- as ``d3p_amd.mixture_density``
stands beside ``d3p_amd.infer_util``.

    log_likelihood_total(model, posterior_samples, obs)                                   -> (n,) float64   sum_r ll[s, r]
    log_joint(model, posterior_samples, obs)                                              -> (n,) float64   + log prior of draw s
    guide_diagnostic(rng_key, n, model, model_args, guide, params, pointwise=False, **kw) -> diagnostics.GuideDiagnostic

``ll[s, r] = log p(obs[r] | pis_s, mus_s, sigs_s)`` is the UNSCALED float32 value of ``mixture_density.log_likelihood``, bit for bit;
``log_likelihood_total[s]`` adds a draw's values over the table in float64 in the fixed order ``include/d3p_hip.h`` states
(``d3p_gmm_loglik_draw_sums``), without the ``n x rows`` matrix.  Samples, shapes, packing (samples that are views of one packed
buffer are read in place) and limits are ``mixture_density``'s; ``model_args = (k, obs, num_obs_total, d)`` as ``d3p_amd.mixture``
reads them, with ``obs`` REQUIRED, and a ``num_obs_total`` that is given must equal the number of rows (``ValueError``): this is the
log joint of the WHOLE table, not a subsample estimate.  ``guide_diagnostic`` draws the latents with the one
``d3p_predict_gmm_draws`` launch on the multi form's key rule: they are the latents ``mixture.posterior_predictive_samples(rng_key,
n, ...)`` returns for the same key.  ``n <= 65535`` as in ``d3p_amd.diagnostics``.  Every host check runs before the device is
touched; there is no CPU fallback; nothing synchronises with the host.

Densities, per draw in float64 torch on the device from the float32 latents and parameters (O(n k d)); alpha = exp(alpha_log) in
float64, tau = prior_mu_scale, xlogy(a, p) = a log p with 0 where a == 0:

    log p(pis)  = lgamma(k)                                                  Dirichlet(1, ..., 1)
    log p(mus)  = - sum mus^2 / (2 tau^2) - k d (log tau + log(2 pi) / 2)
    log p(sigs) = sum_jc (-2 log sigs_jc - 1 / sigs_jc)                      InverseGamma(1, 1)
    log q(pis)  = lgamma(sum_j alpha_j) - sum_j lgamma(alpha_j) + sum_j xlogy(alpha_j - 1, pis_j)
    log q(mus)  = - sum (mus - mus_loc)^2 / 2 - k d log(2 pi) / 2
    log q(sigs) = log p(sigs)                                                the guide draws sigs from the prior
    log_joint[s] = log_likelihood_total[s] + log p(pis) + log p(mus) + log p(sigs)
    log r_s      = log_likelihood_total[s] + log p(pis) + log p(mus) - log q(pis) - log q(mus)

The ``sigs`` terms are LEFT OUT of ``log r_s`` rather than added and subtracted, so that they cancel exactly.
``pointwise["log_joint"]`` and ``pointwise["log_q"]`` include them: ``pointwise["log_ratio"]`` is therefore NOT bitwise
``log_joint - log_q`` (it differs by the rounding of the two ``sigs`` terms).

From the ratios to the ``GuideDiagnostic`` everything is ``d3p_amd.diagnostics``' (its docstring): ``elbo``, ``elbo_se``,
``log_evidence_is``, ``ess``, the float32 hand-over of ``max - log r`` to ``d3p_psis_loo`` with the ``-inf`` / equal-ratios / NaN rules
(``diagnostics._pareto_k``) and ``criteria._k_threshold``.

A zero weight.  ``pis_j == 0`` in a draw happens (a Gamma draw of 1e-317 underflows to it).  The likelihood drops that component.
In ``log q(pis)`` it gives ``xlogy(alpha_j - 1, 0)``: ``+inf`` at ``alpha_j < 1``, so ``log q = +inf`` and ``log r_s = -inf`` -- the rule of
a ``-inf`` ratio: ``elbo = -inf``, ``pareto_k = +inf``, ``log_evidence_is`` finite; nothing (0) at ``alpha_j == 1``; ``-inf`` at
``alpha_j > 1``, so ``log q = -inf`` and ``log r_s = +inf``: one draw carries all the weight, ``elbo = +inf``, ``log_evidence_is = +inf``,
``elbo_se`` and ``ess`` NaN, and ``pareto_k = +inf`` (set here: the shifted column ``max - log r`` is not defined).  A NaN ratio makes
every total NaN.

Label switching.  The mixture's posterior has k! label-switched modes and this guide covers ONE of them.  ``log_evidence_is`` can
therefore sit up to ``log k!`` below the evidence while ``pareto_k`` is fine: k-hat judges the guide's tails around the mode it found,
not its coverage of the other modes.  Out of scope: relabelling across modes, PSIS-smoothed weights, a learned scale of ``mus`` or
``sigs`` in the guide, subsampled estimates.
"""
import math

import torch

from . import _lib
from . import diagnostics as DG
from . import mixture as MX
from . import mixture_density as MD
from . import modelling as M
from ._lib import check, ptr, stream_ptr
from .diagnostics import GuideDiagnostic

__all__ = ["log_likelihood_total", "log_joint", "guide_diagnostic", "GuideDiagnostic"]

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_WHOLE = "this is the log joint of the whole table, not a subsample estimate"


def _draw_sums(x, rows, d, latent, ld, k, n):
    """(n,) float64: d3p_gmm_loglik_draw_sums over the latent rows at `latent`'s data pointer."""
    if rows == 0:   # (the empty sum; an empty obs has no address to hand over)
        return torch.zeros((n,), dtype=torch.float64, device=x.device)
    lib = _lib.load()
    out = torch.empty((n,), dtype=torch.float64, device=x.device)
    nbytes = int(lib.d3p_gmm_loglik_draw_sums_workspace(rows, d, k, n))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    check(lib.d3p_gmm_loglik_draw_sums(stream_ptr(), ptr(x), rows, d, ptr(latent), ld, k, n, ptr(out), ptr(ws), nbytes))
    return out


def _sites(latent, ld, k, d, n):
    """float64 copies (pis (n, k), mus (n, k d), sigs (n, k d)) of the latent rows at `latent`'s data pointer."""
    base, kd = latent.storage_offset(), k * d
    cols = lambda off, width: torch.as_strided(latent, (n, width), (ld, 1), base + off).to(torch.float64)   # noqa: E731
    return cols(0, k), cols(k, kd), cols(k + kd, kd)


def _log_p_pis(k):
    return math.lgamma(k)


def _log_p_mus(mus, tau):
    return (mus * mus).sum(1) / (-2.0 * tau ** 2) - mus.shape[1] * (math.log(tau) + _HALF_LOG_2PI)


def _log_p_sigs(sigs):
    return (-2.0 * torch.log(sigs) - 1.0 / sigs).sum(1)


def _log_q_pis(pis, alpha):
    return torch.lgamma(alpha.sum()) - torch.lgamma(alpha).sum() + torch.xlogy(alpha - 1.0, pis).sum(1)


def _log_q_mus(mus, loc):
    dev = mus - loc
    return (dev * dev).sum(1) * -0.5 - mus.shape[1] * _HALF_LOG_2PI


def _from_samples(joint, model, posterior_samples, obs):
    MD._check_model(model)
    n, k, d = MD._sample_shapes(posterior_samples)
    if obs is None:
        raise ValueError("obs is required")
    rows, d_obs = M._rows_of(obs, "obs")
    if int(d_obs) != d:
        raise ValueError(f"obs: shape (rows, {d}) expected, got {tuple(obs.shape)}")
    rows = int(rows)
    MX._check_limits(k, d, rows)
    if joint and not (model.prior_mu_scale > 0):
        raise ValueError("GaussianMixtureModel: prior_mu_scale must be > 0")
    _lib.require_device()   # (every check above runs without a device)
    dev = obs.device if isinstance(obs, torch.Tensor) and obs.is_cuda else M._device()
    with torch.cuda.device(dev):
        x = M._f32(obs, "obs")
        latent, ld = MD._pack(posterior_samples, n, k, d)
        out = _draw_sums(x, rows, d, latent, ld, k, n)
        if joint:
            _, mus, sigs = _sites(latent, ld, k, d, n)
            out = out + (_log_p_pis(k) + _log_p_mus(mus, float(model.prior_mu_scale))) + _log_p_sigs(sigs)
    return out


def log_likelihood_total(model, posterior_samples, obs):
    """``(n,)`` float64: ``[s] = sum_r log p(obs[r] | draw s)`` over the whole table, the row sums of
    ``mixture_density.log_likelihood``'s matrix without that matrix (module docstring)."""
    return _from_samples(False, model, posterior_samples, obs)


def log_joint(model, posterior_samples, obs):
    """``(n,)`` float64: ``log_likelihood_total`` plus the log prior density of draw s over its three sites -- numpyro's
    ``log_density`` of the model on the whole table at each draw (module docstring)."""
    return _from_samples(True, model, posterior_samples, obs)


def _check_whole_table(model_args, kwargs):
    """A num_obs_total that is given must be the row count of obs (before mixture._shape, which reads a differing one as a plate)."""
    if not isinstance(model_args, (tuple, list)):
        return
    a = list(model_args) + [None] * (4 - len(model_args))
    obs = a[1] if a[1] is not None else kwargs.get("obs")
    total = a[2] if a[2] is not None else M._num_obs_total(kwargs)
    if obs is None or total is None:
        return
    rows, _ = M._rows_of(obs, "obs")
    if int(total) != int(rows):
        raise ValueError(f"num_obs_total = {total} differs from the {int(rows)} rows: {_WHOLE}")


def guide_diagnostic(rng_key, n, model, model_args, guide, params, pointwise=False, **kwargs):
    """ELBO, importance-sampling evidence and the Pareto k of ``n`` draws from the mixture guide at ``params = {"alpha_log": (k,),
    "mus_loc": (k, d)}`` (as ``DPSVI.get_params`` returns them) on the whole table ``model_args = (k, obs[, num_obs_total, d])``: a
    ``diagnostics.GuideDiagnostic`` (module docstring).  ``rng_key`` is a threefry (jax) key; the draws are those
    ``mixture.posterior_predictive_samples(rng_key, n, ...)`` returns.  ``pointwise=True`` keeps ``{"log_ratio", "log_joint", "log_q",
    "log_likelihood"}``, each ``(n,)`` float64; ``log_ratio`` is not bitwise ``log_joint - log_q`` (the ``sigs`` terms are left out of
    it)."""
    from .criteria import _k_threshold

    def host_checks(nn):
        if nn > 65535:
            raise ValueError(f"{nn} draws: the Pareto fit (d3p_psis_loo) runs at most 65535 draws (n <= 65535)")
        _check_whole_table(model_args, kwargs)
        if isinstance(model, MD.GaussianMixtureModel) and not (model.prior_mu_scale > 0):
            raise ValueError("GaussianMixtureModel: prior_mu_scale must be > 0")
    x, rows, d, latent, ld, k, n = MD._posterior_latents(rng_key, n, model, model_args, guide, params, kwargs, host_checks)
    with torch.cuda.device(x.device):
        ll = _draw_sums(x, rows, d, latent, ld, k, n)
        pis, mus, sigs = _sites(latent, ld, k, d, n)
        alpha = torch.exp(M._f32(params["alpha_log"], "params['alpha_log']").reshape(k).to(torch.float64))
        loc = M._f32(params["mus_loc"], "params['mus_loc']").reshape(k * d).to(torch.float64)
        lp = _log_p_pis(k) + _log_p_mus(mus, float(model.prior_mu_scale))
        lq = _log_q_pis(pis, alpha) + _log_q_mus(mus, loc)
        lr = ll + lp - lq                                                # (the sigs terms cancel by being left out)
        elbo = lr.sum() / n
        dev_ = lr - elbo
        se = torch.sqrt((dev_ * dev_).sum() / (n - 1) / n)               # (one draw: 0 / 0 = NaN)
        mx, mn = lr.max(), lr.min()
        r = torch.exp(lr - mx)
        ess = r.sum() ** 2 / (r * r).sum()
        lis = torch.logsumexp(lr, 0) - math.log(n)
        kh = DG._pareto_k(lr, mx, mn, n)
        # a +inf ratio (pis_j == 0 at alpha_j > 1): max - log r is not defined; one draw carries all the weight
        kh = torch.where(torch.isposinf(lr).any() & ~torch.isnan(lr).any(), torch.full_like(kh, math.inf), kh)
        keep = None
        if pointwise:
            ps = _log_p_sigs(sigs)
            keep = {"log_ratio": lr, "log_joint": ll + lp + ps, "log_q": lq + ps, "log_likelihood": ll}
    return GuideDiagnostic(elbo, se, lis, kh, _k_threshold(n), ess, n, rows, keep)

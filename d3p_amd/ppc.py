"""Posterior predictive checks for the regression family: does the fitted model reproduce a statistic of the
data it was fitted to?  (Gelman, Meng & Stern 1996; bayesplot's ``ppc_stat``, ArviZ's ``plot_bpv``.)

    replicate_stats(matrix, shift=0.0)                                              -> ReplicateStats
    predictive_stats(rng_key, model, posterior_samples, X[, y[, N]], shift=0.0)     -> ReplicateStats
    posterior_predictive_stats(rng_key, n, model, (X[, y[, N]]), guide, params, shift=0.0)
                                                                                    -> ({"w"[, "intercept"]}, ReplicateStats)
    posterior_predictive_check(rng_key, n, model, (X, y[, N]), guide, params, statistics=("mean", "sd", "min", "max", "zeros"))
                                                                                    -> PPCResult

Every other reduction of this package over a draws x rows matrix (intervals, HPDI, CRPS / PIT, WAIC, LOO, stacking) runs over the
draws, once per row.  These run over the ROWS, once per draw: for replicated data set ``s`` and a shift ``c``

    sum[s] = sum_r (v[s, r] - c)      sumsq[s] = sum_r (v[s, r] - c)^2      min[s], max[s]      zeros[s] = #{r : v[s, r] == 0}

as float64, in the fixed summation order ``include/d3p_hip.h`` states (``d3p_rep_stats``), so the numbers are a function of the
arguments alone.  ``mean``, ``var``, ``sd``, ``zero_share`` and ``dispersion`` (variance over mean: 1 for a Poisson sample, above 1
for overdispersed counts) follow from them; a shift near the data's mean keeps ``var`` from cancelling.

``replicate_stats`` reduces a matrix that exists (the outcomes of the mixture model or the VAE, or the observed ``y`` itself).
``predictive_stats`` and ``posterior_predictive_stats`` are ``predictive_samples`` / ``posterior_predictive_samples`` with the outcome
rule's result REDUCED instead of stored (``d3p_predict_stats``: the draws x rows product on the matrix cores, the same outcome rule
and keys, bit for bit the values the sampling kernels store): they equal ``replicate_stats`` of that call's ``obs`` by value, and the
n x rows matrix -- 512 MB at 10^6 rows and 128 draws -- is never written.  There is no CPU fallback.

Poisson's markers (``-1`` for a NaN predictor, ``2147483647`` for a saturated rate) are values like any other; they show up in
``min`` / ``max``, and ``posterior_predictive_check`` counts the draws that carry one (``n_marked``) and warns.
"""
import ctypes as C
import math
import warnings
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import modelling as M
from . import predictive as P
from ._lib import check, ptr, stream_ptr
from .infer_util import _check_guide, _model_struct, _pack, _sample_shape

__all__ = ["replicate_stats", "predictive_stats", "posterior_predictive_stats", "posterior_predictive_check", "ReplicateStats", "PPCResult",
           "STATISTICS"]

STATISTICS = ("mean", "sd", "var", "min", "max", "zeros", "zero_share", "dispersion")
_INT_MAX = 2147483647


def _scalar(x, like):
    """x as a float64 operand of `like`: a 0-d tensor beside a tensor -- torch divides by a Python number by multiplying with its
    reciprocal on the GPU, which is not the correctly rounded quotient the statistics are defined as."""
    return torch.tensor(float(x), dtype=torch.float64, device=like.device) if isinstance(like, torch.Tensor) else float(x)


def _derive(name, s, n_rows, shift, ddof=1):
    """Statistic `name` from the five sums, one IEEE float64 operation per step; `s` = (sum, sumsq, min, max, zeros) as torch tensors
    or numpy arrays."""
    total, sumsq, lo, hi, zeros = s
    rows = _scalar(n_rows, total)
    if name == "mean":
        return shift + total / rows
    if name == "var":
        centred = sumsq - total * total / rows
        return centred / _scalar(n_rows - ddof, total) if n_rows != ddof else centred * float("nan")   # (one row and ddof = 1: undefined)
    if name == "sd":
        return _derive("var", s, n_rows, shift, ddof) ** 0.5
    if name == "min":
        return lo
    if name == "max":
        return hi
    if name == "zeros":
        return zeros
    if name == "zero_share":
        return zeros / rows
    if name == "dispersion":
        return _derive("var", s, n_rows, shift, ddof) / _derive("mean", s, n_rows, shift)
    raise ValueError(f"unknown statistic '{name}' (one of {STATISTICS})")


class ReplicateStats(namedtuple("ReplicateStats", ["sum", "sumsq", "min", "max", "zeros", "n_rows", "shift"])):
    """Per replicated data set, float64 on the GPU: ``sum`` and ``sumsq`` of ``v - shift``, ``min``, ``max`` and the number of
    ``zeros``, over ``n_rows`` rows.  Shape ``(n,)``, or ``()`` for a single row vector."""
    __slots__ = ()

    def _five(self):
        return self.sum, self.sumsq, self.min, self.max, self.zeros

    @property
    def mean(self):
        return _derive("mean", self._five(), self.n_rows, self.shift)

    def var(self, ddof=1):
        return _derive("var", self._five(), self.n_rows, self.shift, ddof)

    @property
    def sd(self):
        return _derive("sd", self._five(), self.n_rows, self.shift)

    @property
    def zero_share(self):
        return _derive("zero_share", self._five(), self.n_rows, self.shift)

    @property
    def dispersion(self):
        return _derive("dispersion", self._five(), self.n_rows, self.shift)


class PPCResult(namedtuple("PPCResult", ["statistic", "observed", "replicated", "p_ge", "p_le", "n_draws", "n_rows", "n_marked"])):
    """``statistic``: the names asked for; ``observed[name]`` = T(y); ``replicated[name]`` = T(y_rep_s), ``n_draws`` float64 values (a
    numpy array); ``p_ge[name]`` = #{T_rep >= T_obs} / n and ``p_le[name]`` = #{T_rep <= T_obs} / n, by value; ``n_marked``: the
    Poisson draws that hold a marker (-1 or 2147483647) -- their statistics describe the marker, not a count."""
    __slots__ = ()

    def lines(self):
        """One line per statistic: observed, the replicated mean and central 90 % range, p_ge, p_le."""
        out = []
        for name in self.statistic:
            rep = self.replicated[name]
            with np.errstate(all="ignore"):
                lo, hi = (np.nanquantile(rep, [0.05, 0.95]) if np.isfinite(rep).any() else (float("nan"),) * 2)
                mid = np.nanmean(rep) if np.isfinite(rep).any() else float("nan")
            out.append(f"ppc {name:<10s} observed {self.observed[name]:12.5g}   replicated {mid:12.5g} [{lo:.5g}, {hi:.5g}]   "
                       f"p_ge {self.p_ge[name]:.3f}   p_le {self.p_le[name]:.3f}")
        return out


def _tail_shares(rep, obs):
    """(p_ge, p_le) = (#{rep >= obs}, #{rep <= obs}) / n by value (a NaN counts on neither side)."""
    rep = np.asarray(rep, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return float((rep >= obs).sum()) / rep.size, float((rep <= obs).sum()) / rep.size


def _check_statistics(statistics):
    if isinstance(statistics, str):
        statistics = (statistics,)
    names = tuple(statistics)
    if not names:
        raise ValueError(f"statistics: at least one of {STATISTICS}")
    for name in names:
        if name not in STATISTICS:
            raise ValueError(f"unknown statistic '{name}' (one of {STATISTICS})")
    return names


def _check_shift(shift):
    shift = float(shift)
    if not math.isfinite(shift):
        raise ValueError("shift must be finite")
    return shift


def _result(out, rows, shift, single=False):
    five = tuple(out[k, 0] if single else out[k] for k in range(5))
    return ReplicateStats(*five, int(rows), shift)


def replicate_stats(matrix, shift=0.0):
    """The five per-draw statistics of a matrix of outcomes that exists: ``matrix`` is a float32 or int32 CUDA tensor ``(n, rows)``,
    one replicated data set per row, or a single data set ``(rows,)`` (the fields then have shape ``()``).  It is read in place when
    its last stride is 1 and its rows do not overlap, otherwise copied once."""
    shift = _check_shift(shift)
    if not isinstance(matrix, torch.Tensor):
        raise TypeError("replicate_stats: a float32 or int32 CUDA tensor (n, rows) or (rows,) is required")
    if matrix.dtype not in (torch.float32, torch.int32):
        raise TypeError(f"replicate_stats: float32 or int32 values, got {matrix.dtype}")
    if matrix.dim() not in (1, 2):
        raise ValueError(f"replicate_stats: shape (n, rows) or (rows,) expected, got {tuple(matrix.shape)}")
    single = matrix.dim() == 1
    n, rows = (1, matrix.shape[0]) if single else tuple(matrix.shape)
    if n < 1 or rows < 1:
        raise ValueError("replicate_stats: at least one draw and one row (the minimum and maximum of nothing are undefined)")
    if not matrix.is_cuda:
        raise TypeError("replicate_stats: the matrix must be a CUDA tensor (there is no CPU fallback)")
    _lib.require_device()
    m = matrix.detach().reshape(n, rows)
    if (rows > 1 and m.stride(1) != 1) or (n > 1 and m.stride(0) < rows):
        m = m.contiguous()
    ld = m.stride(0) if n > 1 else rows
    lib = _lib.load()
    with torch.cuda.device(m.device):
        out = torch.empty((5, n), dtype=torch.float64, device=m.device)
        nbytes = int(lib.d3p_rep_stats_workspace(rows, n))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=m.device)
        check(lib.d3p_rep_stats(stream_ptr(), ptr(m), 0 if m.dtype == torch.float32 else 1, ld, n, rows, shift, ptr(out), ptr(ws), nbytes))
    return _result(out, rows, shift, single)


def _stats(model, fam, X, rows, d, n, latent, obs_keys, shift):
    """d3p_predict_stats over latent = (tensor at the first latent row, ld, w_off, b_col): (5, n) float64 on the current GPU."""
    first, ld, w_off, b_col = latent
    X = M._f32(X, "X")
    lib = _lib.load()
    out = torch.empty((5, n), dtype=torch.float64, device=X.device)
    nbytes = int(lib.d3p_rep_stats_workspace(rows, n))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=X.device)
    ms = _model_struct(model, fam, d)
    check(lib.d3p_predict_stats(stream_ptr(), C.byref(ms), ptr(X), rows, d, ptr(first), ld, w_off, b_col, n, ptr(obs_keys), shift, ptr(out),
                                ptr(ws), nbytes))
    return out


def predictive_stats(rng_key, model, posterior_samples, *model_args, shift=0.0, **kwargs):
    """``replicate_stats(predictive_samples(rng_key, model, posterior_samples, *model_args), shift)`` by value, without the ``(n,
    rows)`` matrix: the same samples, the same ``obs`` keys (``split(rng_key, n)[s]``), the same outcome rule.  A single sample (``w``
    of shape ``(d,)``) gives fields of shape ``()``."""
    fam = P._family(model)
    shift = _check_shift(shift)
    rows, d = P._data(model, model_args, kwargs)
    n, single = _sample_shape(model, posterior_samples, d)
    key = M._check_key(rng_key)
    _lib.require_device()   # (every check above runs without a device)
    dev = key.device
    with torch.cuda.device(dev):
        obs_keys = torch.empty((n, 2), dtype=torch.uint32, device=dev)
        check(_lib.load().d3p_tf_split(stream_ptr(), ptr(key), n, ptr(obs_keys)))
        out = _stats(model, fam, model_args[0], rows, d, n, _pack(model, posterior_samples, n, d), obs_keys, shift)
    return _result(out, rows, shift, single)


def _posterior_checks(rng_key, n, model, model_args, guide, params, kwargs):
    """The refusals of posterior_predictive_samples, in its order, without a device: (fam, n, rows, d, gparams)."""
    fam = P._family(model)
    _check_guide(model, guide)
    n = P._count(n)
    rows, d = P._data(model, model_args, kwargs)
    if not isinstance(params, dict):
        raise ValueError("params: the dict DPSVI.get_params returns is required")
    gparams = [(name, M._param(params, name, size)) for name, size in M._guide_param_names(guide, model, d)]
    return fam, n, rows, d, gparams


def _posterior_stats(key, fam, n, rows, d, gparams, model, X, guide, shift):
    dev = key.device
    with torch.cuda.device(dev):
        latents, latent, obs_keys, _ = P._latents(key, n, model, rows, d, guide, gparams, {})
        out = _stats(model, fam, X, rows, d, n, latent, obs_keys, shift)
    return latents, _result(out, rows, shift)


def posterior_predictive_stats(rng_key, n, model, model_args, guide, params, shift=0.0, **kwargs):
    """``posterior_predictive_samples`` with ``obs`` reduced instead of stored: ``({"w": (n, d)[, "intercept": (n,)]}, ReplicateStats)``.
    The latents are that call's, bit for bit (the same key rule, the same launch), and the statistics equal ``replicate_stats`` of its
    ``obs`` by value.  Guides: ``AutoDiagonalNormal``, ``DiagonalNormalGuide``; ``MeanFieldGuide`` for logistic regression."""
    fam, n, rows, d, gparams = _posterior_checks(rng_key, n, model, model_args, guide, params, kwargs)
    shift = _check_shift(shift)
    key = M._check_key(rng_key)
    _lib.require_device()
    return _posterior_stats(key, fam, n, rows, d, gparams, model, model_args[0], guide, shift)


def _observed(model, fam, y, rows):
    """y as the one-row matrix of its family's outcome type: float32 (linear) or int32 (counts, 0 / 1 labels; integral values only)."""
    t = y.detach() if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
    if t.numel() != rows:
        raise ValueError(f"y: {rows} values expected (one per row of X), got {t.numel()}")
    t = t.reshape(rows)
    if fam == _lib.D3P_FAMILY_LINREG:
        return t.to(torch.float32)
    if t.is_floating_point():
        if not bool((t == torch.floor(t)).all()) or not bool((t.abs() <= _INT_MAX).all()):
            raise ValueError(f"y: {type(model).__name__} outcomes are integers (counts or 0 / 1 labels); got non-integral values")
    elif t.dtype == torch.bool:
        pass
    elif not bool((t.to(torch.int64).abs() <= _INT_MAX).all()):
        raise ValueError("y: values beyond int32")
    return t.to(torch.int32)


def posterior_predictive_check(rng_key, n, model, model_args, guide, params, statistics=("mean", "sd", "min", "max", "zeros"), **kwargs):
    """Compare ``T(y)`` with ``T(y_rep_s)`` over ``n`` data sets replicated from the posterior predictive at ``params``:
    ``model_args = (X, y[, N])``, ``statistics`` names from ``STATISTICS``.  ``T(y)`` comes from ``replicate_stats`` on ``y`` as a
    one-row matrix (float32 for ``LinearRegression``, int32 for counts and 0 / 1 labels: non-integral ``y`` raises ``ValueError``), the
    replicated values from ``posterior_predictive_stats`` on the same key rule; both use the shift ``float32(mean(y))``.  A tail share
    near 0 or 1 says the model does not reproduce that statistic (``zeros`` and ``dispersion`` are the ones a Poisson fit to
    zero-inflated or overdispersed counts fails).  Returns a ``PPCResult``."""
    names = _check_statistics(statistics)
    fam, n, rows, d, gparams = _posterior_checks(rng_key, n, model, model_args, guide, params, kwargs)
    if len(model_args) < 2 or model_args[1] is None:
        raise ValueError("y is missing: model_args = (X, y[, N]); a posterior predictive check compares with the observed outcomes")
    y = _observed(model, fam, model_args[1], rows)
    key = M._check_key(rng_key)
    _lib.require_device()
    dev = key.device
    with torch.cuda.device(dev):
        y = y.to(dev).contiguous()
        shift = float(y.to(torch.float32).mean())   # once; float32, so that a caller can restate it
        if not math.isfinite(shift):
            shift = 0.0
        obs = replicate_stats(y.reshape(1, rows), shift)
        _, rep = _posterior_stats(key, fam, n, rows, d, gparams, model, model_args[0], guide, shift)
        o5 = [np.asarray(t.cpu().numpy(), np.float64).reshape(-1) for t in obs._five()]
        r5 = [np.asarray(t.cpu().numpy(), np.float64).reshape(-1) for t in rep._five()]
    observed, replicated, p_ge, p_le = {}, {}, {}, {}
    with np.errstate(all="ignore"):
        for name in names:
            observed[name] = float(_derive(name, o5, rows, shift)[0])
            replicated[name] = np.asarray(_derive(name, r5, rows, shift), np.float64)
            p_ge[name], p_le[name] = _tail_shares(replicated[name], observed[name])
    n_marked = int(((r5[2] == -1) | (r5[3] == _INT_MAX)).sum()) if fam == _lib.D3P_FAMILY_POISSON else 0
    if n_marked:
        warnings.warn(f"posterior_predictive_check: {n_marked} of {n} replicated data sets hold a Poisson marker (-1: NaN predictor, "
                      f"{_INT_MAX}: saturated rate); their statistics describe the marker", RuntimeWarning, stacklevel=2)
    return PPCResult(names, observed, replicated, p_ge, p_le, n, rows, n_marked)

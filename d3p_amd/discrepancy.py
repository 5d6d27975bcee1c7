"""Realized-discrepancy predictive checks and the Bayesian R^2 of the regression family.

    predictive_discrepancy(rng_key, model, posterior_samples, X, y[, N], shift=None)                    -> DiscrepancySums
    posterior_predictive_discrepancy(rng_key, n, model, (X, y[, N]), guide, params, shift=None)         -> ({"w"[, "intercept"]}, DiscrepancySums)
    discrepancy_check(rng_key, n, model, (X, y[, N]), guide, params)                                    -> DiscrepancyResult

``d3p_amd.ppc`` compares a statistic of the data, ``T(y)``, with ``T(y_rep_s)``.  The check Gelman, Meng & Stern (1996) define takes a
discrepancy ``D(y, theta)`` that depends on the parameters too: it is evaluated per posterior draw ``s``, once on the observed data
and once on that draw's own replicate, and the p-value is the share of draws with ``D(y_rep_s, theta_s) >= D(y, theta_s)``.  Here ``D``
is the Pearson chi-square, with ``mu`` the float32 conditional mean ``d3p_predict_mean_rows`` stores and ``v`` the outcome
``predictive_samples`` stores, all further arithmetic in float64 with one rounding per operation:

    M = mu[s, r]      V = sigma^2 (linear, sigma = float32(obs_scale)) | M (Poisson) | M (1 - M) (logistic)
    q(x) = 0 if x == M else (x - M)^2 / V
    chi2_obs[s] = sum_r q(y_r)                  chi2_rep[s] = sum_r q(v[s, r])
    mu_sum[s]   = sum_r (M - shift)             mu_sumsq[s]  = sum_r (M - shift)^2
    res_sum[s]  = sum_r (y_r - M)               res_sumsq[s] = sum_r (y_r - M)^2

One convention (``include/d3p_hip.h``, ``d3p_predict_discrepancy``): a row that is matched exactly contributes nothing, even where
``V == 0``; otherwise nothing is clamped -- a mismatch at ``V == 0`` (a rate that underflowed to 0 against a count of 1, a sigmoid that
saturated against the other label) gives ``+inf``, a NaN mean NaN, and ``discrepancy_check`` counts such draws (``n_nonfinite``) and
warns.  The sums are added in the fixed order of ``d3p_rep_stats``, so the numbers are a function of the arguments alone; neither the
``n x rows`` outcome matrix nor the ``n x rows`` mean matrix is written.  There is no CPU fallback.

The four sums beside the chi-squares give, per draw, the Bayesian R^2 (Gelman, Goodrich, Gabry & Vehtari 2019; rstanarm's
``bayes_R2``), the RMSE and the bias: ``DiscrepancySums.bayes_r2``, ``rmse``, ``bias``.
"""
import ctypes as C
import math
import warnings
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import modelling as M
from . import ppc as _ppc
from . import predictive as P
from ._lib import check, ptr, stream_ptr
from .infer_util import _model_struct, _pack, _sample_shape
from .ppc import _scalar

__all__ = ["predictive_discrepancy", "posterior_predictive_discrepancy", "discrepancy_check", "DiscrepancySums", "DiscrepancyResult",
           "R2_KINDS"]

R2_KINDS = ("residual", "model")


def _sqrt(x):
    return torch.sqrt(x) if isinstance(x, torch.Tensor) else np.sqrt(x)


def _centred_var(total, sumsq, n_rows, ddof):
    """(sumsq - total total / rows) / (rows - ddof), one IEEE float64 operation per step (ppc._derive's "var")."""
    centred = sumsq - total * total / _scalar(n_rows, total)
    return centred / _scalar(n_rows - ddof, total) if n_rows != ddof else centred * float("nan")   # (one row and ddof = 1: undefined)


class DiscrepancySums(namedtuple("DiscrepancySums", ["chi2_obs", "chi2_rep", "mu_sum", "mu_sumsq", "res_sum", "res_sumsq", "n_rows", "shift"])):
    """Per posterior draw, float64 on the GPU: the realized and the replicated chi-square, the sums of ``mu - shift`` and of its
    square, the sums of ``y - mu`` and of its square, over ``n_rows`` rows.  Shape ``(n,)``, or ``()`` for a single sample.  The
    derived values take one IEEE float64 operation per step, the row count entering as a 0-d tensor (``ppc._derive``'s rule); they
    work on numpy arrays as well.  ``model``: the model the sums were computed for (what ``bayes_r2("model")`` reads), set by the
    functions of this module; ``None`` on a hand-made instance."""
    model = None

    @property
    def mean_mu(self):
        """``shift + mu_sum / rows``: the mean over the rows of the conditional mean."""
        return self.shift + self.mu_sum / _scalar(self.n_rows, self.mu_sum)

    def var_fit(self, ddof=1):
        """The variance over the rows of the conditional mean: ``(mu_sumsq - mu_sum mu_sum / rows) / (rows - ddof)``."""
        return _centred_var(self.mu_sum, self.mu_sumsq, self.n_rows, ddof)

    def var_res(self, ddof=1):
        """The variance over the rows of the residual ``y - mu``: ``(res_sumsq - res_sum res_sum / rows) / (rows - ddof)``."""
        return _centred_var(self.res_sum, self.res_sumsq, self.n_rows, ddof)

    @property
    def bias(self):
        """``res_sum / rows``: the mean residual."""
        return self.res_sum / _scalar(self.n_rows, self.res_sum)

    @property
    def rmse(self):
        """``sqrt(res_sumsq / rows)``."""
        return _sqrt(self.res_sumsq / _scalar(self.n_rows, self.res_sumsq))

    @property
    def dispersion(self):
        """``chi2_obs / rows``: near 1 where the model's variance matches the data's, above 1 for overdispersed outcomes."""
        return self.chi2_obs / _scalar(self.n_rows, self.chi2_obs)

    def expected_var_res(self, model=None):
        """The residual variance the MODEL expects at this draw (Gelman et al. 2019, section 2), in these exact steps:

            LinearRegression     sigma sigma,  sigma = float64(float32(model.obs_scale))        (a Python float)
            PoissonRegression    mean_mu                                                        (the mean over the rows of Var = mu)
            LogisticRegression   mean_mu - (mu_sumsq / rows + (2.0 (mean_mu - shift)) shift + shift shift)
                                 (the mean of mu (1 - mu) = mean(mu) - mean(mu^2), mean(mu^2) from the two shifted sums)
        """
        model = self.model if model is None else model
        if model is None:
            raise ValueError("bayes_r2('model'): the model is required (DiscrepancySums.model is None on a hand-made instance: pass model=...)")
        fam = P._family(model)
        if fam == _lib.D3P_FAMILY_LINREG:
            sigma = float(np.float32(model.obs_scale))
            return sigma * sigma
        mean_mu = self.mean_mu
        if fam == _lib.D3P_FAMILY_POISSON:
            return mean_mu
        mean_sq = self.mu_sumsq / _scalar(self.n_rows, self.mu_sumsq) + (2.0 * (mean_mu - self.shift)) * self.shift + self.shift * self.shift
        return mean_mu - mean_sq

    def bayes_r2(self, kind="residual", model=None):
        """The Bayesian R^2 per draw, ``var_fit / (var_fit + var_e)`` with ``var_fit = var_fit(ddof=1)`` and

            kind "residual"   var_e = var_res(ddof=1): the variance of this draw's residuals, rstanarm's ``bayes_R2`` rule
            kind "model"      var_e = expected_var_res(model): the residual variance the model expects (Gelman et al. 2019)

        In [0, 1] wherever both variances are >= 0 and not both 0."""
        if kind not in R2_KINDS:
            raise ValueError(f"unknown R^2 kind '{kind}' (one of {R2_KINDS})")
        fit = self.var_fit()
        return fit / (fit + (self.var_res() if kind == "residual" else self.expected_var_res(model)))

    def _six(self):
        return self.chi2_obs, self.chi2_rep, self.mu_sum, self.mu_sumsq, self.res_sum, self.res_sumsq


class DiscrepancyResult(namedtuple("DiscrepancyResult", ["chi2_obs", "chi2_rep", "p_ge", "p_le", "dispersion", "r2", "rmse", "bias", "n_draws",
                                                         "n_rows", "n_nonfinite"])):
    """``chi2_obs[s]`` = D(y, theta_s) and ``chi2_rep[s]`` = D(y_rep_s, theta_s), ``n_draws`` float64 values each (numpy arrays);
    ``p_ge`` = #{s : chi2_rep[s] >= chi2_obs[s]} / n and ``p_le`` likewise, PAIRED per draw, by value, a NaN counting on neither side;
    ``dispersion`` = chi2_obs / rows; ``r2`` = {"residual": ..., "model": ...}, ``rmse`` and ``bias`` per draw; ``n_nonfinite``: the
    draws whose realized or replicated chi-square is not finite."""
    __slots__ = ()

    def lines(self):
        """The p-values, then one line per per-draw quantity: its mean and central 90 % range over the draws."""
        out = [f"discrepancy chi2     p_ge {self.p_ge:.3f}   p_le {self.p_le:.3f}   ({self.n_draws} draws, {self.n_rows} rows, "
               f"{self.n_nonfinite} not finite)"]
        for name, x in (("chi2_obs", self.chi2_obs), ("chi2_rep", self.chi2_rep), ("dispersion", self.dispersion),
                        ("r2_residual", self.r2["residual"]), ("r2_model", self.r2["model"]), ("rmse", self.rmse), ("bias", self.bias)):
            x = np.asarray(x, np.float64).reshape(-1)
            fin = x[np.isfinite(x)]
            mid, lo, hi = (fin.mean(), *np.quantile(fin, [0.05, 0.95])) if fin.size else (float("nan"),) * 3
            out.append(f"discrepancy {name:<12s} {mid:12.5g} [{lo:.5g}, {hi:.5g}]")
        return out


def _paired_tail_shares(rep, obs):
    """(p_ge, p_le) = (#{s : rep[s] >= obs[s]}, #{s : rep[s] <= obs[s]}) / n by value (a NaN on either side counts on neither)."""
    rep, obs = np.asarray(rep, np.float64).reshape(-1), np.asarray(obs, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return float((rep >= obs).sum()) / rep.size, float((rep <= obs).sum()) / rep.size


def _check_shift(shift):
    return None if shift is None else _ppc._check_shift(shift)


def _outcome_arg(model, model_args):
    if len(model_args) < 2 or model_args[1] is None:
        raise ValueError("y is missing: model_args = (X, y[, N]); a realized discrepancy compares with the observed outcomes")
    return model_args[1]


def _y_and_shift(y, shift, dev):
    """y as float32 on `dev` and the shift: the given one, or float32(mean(y)) (0.0 where that is not finite)."""
    y = y.to(dev).to(torch.float32).contiguous()
    if shift is None:
        shift = float(y.mean())   # once; float32, so that a caller can restate it
        if not math.isfinite(shift):
            shift = 0.0
    return y, shift


def _sums(model, fam, X, y, rows, d, n, latent, obs_keys, shift):
    """d3p_predict_discrepancy over latent = (tensor at the first latent row, ld, w_off, b_col): (6, n) float64 on the current GPU."""
    first, ld, w_off, b_col = latent
    X = M._f32(X, "X")
    lib = _lib.load()
    out = torch.empty((6, n), dtype=torch.float64, device=X.device)
    nbytes = int(lib.d3p_predict_discrepancy_workspace(rows, n))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=X.device)
    ms = _model_struct(model, fam, d)
    check(lib.d3p_predict_discrepancy(stream_ptr(), C.byref(ms), ptr(X), ptr(y), rows, d, ptr(first), ld, w_off, b_col, n, ptr(obs_keys), shift,
                                      ptr(out), ptr(ws), nbytes))
    return out


def _result(out, rows, shift, model, single=False):
    res = DiscrepancySums(*(out[k, 0] if single else out[k] for k in range(6)), int(rows), shift)
    res.model = model
    return res


def predictive_discrepancy(rng_key, model, posterior_samples, *model_args, shift=None, **kwargs):
    """The six sums over given samples: ``model_args = (X, y[, N])``, ``posterior_samples`` as for ``predictive_samples``, whose key
    rule the replicated outcomes follow (draw ``s`` uses the ``obs`` key ``split(rng_key, n)[s]``): ``chi2_rep`` is the chi-square of
    that call's ``obs``.  ``y`` is validated as ``posterior_predictive_check`` does (integral for counts and labels) and read as
    float32.  ``shift=None``: ``float32(mean(y))``, or 0.0 where that is not finite.  A single sample (``w`` of shape ``(d,)``) gives
    fields of shape ``()``."""
    fam = P._family(model)
    shift = _check_shift(shift)
    rows, d = P._data(model, model_args, kwargs)
    n, single = _sample_shape(model, posterior_samples, d)
    y = _ppc._observed(model, fam, _outcome_arg(model, model_args), rows)
    key = M._check_key(rng_key)
    _lib.require_device()   # (every check above runs without a device)
    dev = key.device
    with torch.cuda.device(dev):
        y, shift = _y_and_shift(y, shift, dev)
        obs_keys = torch.empty((n, 2), dtype=torch.uint32, device=dev)
        check(_lib.load().d3p_tf_split(stream_ptr(), ptr(key), n, ptr(obs_keys)))
        out = _sums(model, fam, model_args[0], y, rows, d, n, _pack(model, posterior_samples, n, d), obs_keys, shift)
    return _result(out, rows, shift, model, single)


def _posterior_sums(key, fam, n, rows, d, gparams, model, X, y, guide, shift):
    dev = key.device
    with torch.cuda.device(dev):
        y, shift = _y_and_shift(y, shift, dev)
        latents, latent, obs_keys, _ = P._latents(key, n, model, rows, d, guide, gparams, {})
        out = _sums(model, fam, X, y, rows, d, n, latent, obs_keys, shift)
    return latents, _result(out, rows, shift, model)


def _posterior_args(rng_key, n, model, model_args, guide, params, kwargs):
    """The refusals of posterior_predictive_samples, then y's, then the key's: all without a device."""
    fam, n, rows, d, gparams = _ppc._posterior_checks(rng_key, n, model, model_args, guide, params, kwargs)
    y = _ppc._observed(model, fam, _outcome_arg(model, model_args), rows)
    return fam, n, rows, d, gparams, y


def posterior_predictive_discrepancy(rng_key, n, model, model_args, guide, params, shift=None, **kwargs):
    """``posterior_predictive_samples`` with ``obs`` and the conditional mean reduced against ``y`` instead of stored:
    ``({"w": (n, d)[, "intercept": (n,)]}, DiscrepancySums)``.  The latents are that call's, bit for bit (the same key rule, the same
    launch), and ``chi2_rep`` is the chi-square of its ``obs``.  ``model_args = (X, y[, N])``.  Guides: ``AutoDiagonalNormal``,
    ``DiagonalNormalGuide``; ``MeanFieldGuide`` for logistic regression."""
    fam, n, rows, d, gparams, y = _posterior_args(rng_key, n, model, model_args, guide, params, kwargs)
    shift = _check_shift(shift)
    key = M._check_key(rng_key)
    _lib.require_device()
    return _posterior_sums(key, fam, n, rows, d, gparams, model, model_args[0], y, guide, shift)


def discrepancy_check(rng_key, n, model, model_args, guide, params, **kwargs):
    """The chi-square check of Gelman, Meng & Stern (1996) over ``n`` posterior draws at ``params``, with the Bayesian R^2 (both
    kinds), the RMSE and the bias per draw: ``posterior_predictive_discrepancy`` at the shift ``float32(mean(y))``, brought to the host.
    ``p_ge`` near 0 says the data are further from the model's mean, in units of the model's variance, than the model's own
    replicates are: overdispersion for a Poisson fit, an ``obs_scale`` too small for a linear one.  Returns a ``DiscrepancyResult``;
    warns (``RuntimeWarning``) when a draw's chi-square is not finite."""
    fam, n, rows, d, gparams, y = _posterior_args(rng_key, n, model, model_args, guide, params, kwargs)
    key = M._check_key(rng_key)
    _lib.require_device()
    _, sums = _posterior_sums(key, fam, n, rows, d, gparams, model, model_args[0], y, guide, None)
    host = DiscrepancySums(*(np.asarray(t.cpu().numpy(), np.float64).reshape(-1) for t in sums._six()), rows, sums.shift)
    host.model = model
    with np.errstate(all="ignore"):
        p_ge, p_le = _paired_tail_shares(host.chi2_rep, host.chi2_obs)
        r2 = {kind: np.asarray(host.bayes_r2(kind), np.float64) for kind in R2_KINDS}
        res = DiscrepancyResult(host.chi2_obs, host.chi2_rep, p_ge, p_le, host.dispersion, r2, host.rmse, host.bias, n, rows,
                                int((~(np.isfinite(host.chi2_obs) & np.isfinite(host.chi2_rep))).sum()))
    if res.n_nonfinite:
        warnings.warn(f"discrepancy_check: the chi-square of {res.n_nonfinite} of {n} draws is not finite (a mean that is NaN, or a "
                      "variance of 0 against an outcome the mean does not match)", RuntimeWarning, stacklevel=2)
    return res

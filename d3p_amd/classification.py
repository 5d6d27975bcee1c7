"""Classification metrics of a fitted logistic regression: accuracy, confusion counts, ROC, AUC, calibration.

    predictive_confusion(rng_key, model, posterior_samples, X, y[, N], thresholds=(0.5,))            -> ConfusionCounts
    posterior_predictive_confusion(rng_key, n, model, (X, y[, N]), guide, params, thresholds=(0.5,)) -> ({"w"[, "intercept"]}, ConfusionCounts)
    binary_curve(p, y, bins=10)                                                                      -> BinaryCurve
    classification_report(rng_key, n, model, (X, y[, N]), guide, params, thresholds=(0.5,), bins=10) -> ClassificationReport

The reference's logistic-regression example reports ``estimate_accuracy``: the agreement of posterior-predictive label draws with the
test labels.  ``posterior_predictive_confusion`` computes that number per draw -- and the true / false positives of the predicted
probability at up to four thresholds -- in the kernel that forms the draws x rows product, so neither the ``n x rows`` label matrix nor
the ``n x rows`` probability matrix is written.  With ``mu`` the float32 probability ``d3p_predict_mean_rows`` stores and ``v`` the label
``predictive_samples`` stores, per draw ``s``:

    agree[s]  = #{r : v[s, r] == y_r}                  n_nan[s] = #{r : mu[s, r] is NaN}
    tp[s, j]  = #{r : mu[s, r] >= tau_j and y_r == 1}  fp[s, j] = #{r : mu[s, r] >= tau_j and y_r == 0}      (float32 >=)

``binary_curve`` is model-free: a ROC histogram of one score vector at 11 mantissa bits of ``min(p, 1 - p)`` (0x7E001 bins, ordered as
the scores are), from which the AUC comes with a CERTIFICATE ``auc_lo <= AUC <= auc_hi`` -- every pair of a positive and a negative
that the histogram cannot order lies in one bin and is counted in ``pairs_same_bin`` -- and a reliability table over ``bins`` equal
bins with exact fixed-point sums of the scores.  Everything the device computes is an integer, so every number is a function of the
arguments alone and is tested by value.  Models: ``LogisticRegression``; guides: ``AutoDiagonalNormal``, ``DiagonalNormalGuide``.  There
is no CPU fallback.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import modelling as M
from . import prediction as PR
from . import predictive as P
from . import ppc as _ppc
from ._lib import check, ptr, stream_ptr
from .infer_util import _model_struct, _pack, _sample_shape
from .models import AutoDiagonalNormal, DiagonalNormalGuide
from .ppc import _scalar

__all__ = ["predictive_confusion", "posterior_predictive_confusion", "binary_curve", "classification_report", "ConfusionCounts",
           "BinaryCurve", "ClassificationReport"]

MAX_THRESHOLDS = 4           # D3P_CONF_THRESHOLDS
CURVE_BINS = 0x7E001         # D3P_CURVE_BINS
MAX_CURVE_ROWS = 1 << 27     # the fixed-point sums of the reliability table stay below 2^63
_FIXED = float(1 << 36)
_SUMMARY = 6                 # D3P_CURVE_SUMMARY


def _f64(x):
    return x.to(torch.float64) if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


class ConfusionCounts(namedtuple("ConfusionCounts", ["agree", "n_nan", "tp", "fp", "n_pos", "n_neg", "n_rows", "thresholds"])):
    """Per posterior draw, int64 on the GPU: ``agree`` and ``n_nan`` of shape ``(n,)``, ``tp`` and ``fp`` of shape ``(n, T)`` (``()`` and
    ``(T,)`` for a single sample); ``n_pos``, ``n_neg``, ``n_rows``: the class totals of ``y`` and the rows (Python ints);
    ``thresholds``: the ``T`` float32 thresholds as Python floats.  The derived values are float64, one IEEE operation per step on exact
    integers (sums and differences of counts are exact); 0 / 0 gives NaN and nothing is clamped.  They work on numpy arrays as well."""
    __slots__ = ()

    @property
    def fn(self):
        """``n_pos - tp``"""
        return self.n_pos - self.tp

    @property
    def tn(self):
        """``n_neg - fp``"""
        return self.n_neg - self.fp

    @property
    def sampled_accuracy(self):
        """``agree / rows`` per draw; its mean over the draws is the reference's ``estimate_accuracy``."""
        a = _f64(self.agree)
        return a / _scalar(self.n_rows, a)

    @property
    def accuracy(self):
        """``(tp + tn) / rows``"""
        a = _f64(self.tp + self.tn)
        return a / _scalar(self.n_rows, a)

    @property
    def tpr(self):
        """``tp / n_pos`` (recall, sensitivity)"""
        a = _f64(self.tp)
        return a / _scalar(self.n_pos, a)

    @property
    def fpr(self):
        """``fp / n_neg``"""
        a = _f64(self.fp)
        return a / _scalar(self.n_neg, a)

    @property
    def tnr(self):
        """``tn / n_neg`` (specificity)"""
        a = _f64(self.tn)
        return a / _scalar(self.n_neg, a)

    @property
    def precision(self):
        """``tp / (tp + fp)``"""
        return _f64(self.tp) / _f64(self.tp + self.fp)

    @property
    def f1(self):
        """``2 tp / (2 tp + fp + fn)``"""
        return _f64(2 * self.tp) / _f64(2 * self.tp + self.fp + self.fn)

    @property
    def balanced_accuracy(self):
        """``(tpr + tnr) / 2``"""
        return (self.tpr + self.tnr) / 2.0


class BinaryCurve(namedtuple("BinaryCurve", ["hist", "calib", "n_pos", "n_neg", "pairs_concordant", "pairs_same_bin", "auc", "auc_lo",
                                             "auc_hi", "ks", "ece", "mce", "bins"])):
    """``hist``: ``(2, CURVE_BINS)`` int32 on the GPU, class x bin (bin 0: a score of 0, the last bin: a score of 1); ``calib``: ``(3,
    bins)`` int64 on the GPU (count, positives, sum of ``(uint64)(p 2^36)``); ``n_pos``, ``n_neg``, ``pairs_concordant``,
    ``pairs_same_bin``: Python ints; the rest Python floats, float64:

        auc_lo = conc / (P N)      auc_hi = (conc + same) / (P N)      auc = (conc + same / 2) / (P N)         (NaN where P N == 0)
        ks  = max over the bin edges of |tpr - fpr| = max_k |b_k P - a_k N| / (P N), a_k / b_k the positives / negatives of the bins 0..k
        ece = sum_b (count_b / rows) |pos_b / count_b - sum_b / 2^36 / count_b|      mce = the largest of those gaps (empty bins left out)

    ``auc_lo <= AUC <= auc_hi`` holds for the exact (Mann-Whitney) AUC of the scores; ``pairs_same_bin == 0`` makes all three exact."""
    __slots__ = ()

    def roc(self, compact=True):
        """``(fpr, tpr)``: float64 tensors on the GPU from ``torch.cumsum`` of ``hist`` from the top bin down, starting at (0, 0) and
        ending at (1, 1); point ``k`` thresholds at the lower edge of the ``k``-th bin from the top.  ``compact``: only the points
        after an occupied bin (the others repeat their predecessor)."""
        top = torch.flip(self.hist.to(torch.int64), dims=(1,))
        if compact:
            top = top[:, (top[0] + top[1]) > 0]
        cum = torch.cumsum(top, dim=1).to(torch.float64)
        zero = torch.zeros((1,), dtype=torch.float64, device=cum.device)
        fpr = torch.cat([zero, cum[0] / _scalar(self.n_neg, cum)])
        tpr = torch.cat([zero, cum[1] / _scalar(self.n_pos, cum)])
        return fpr, tpr


class ClassificationReport(namedtuple("ClassificationReport", ["counts", "sampled_accuracy", "accuracy", "curve", "mean_probability", "latents",
                                                               "n_draws", "n_rows"])):
    """``counts``: the ``ConfusionCounts`` of the ``n_draws`` posterior draws; ``sampled_accuracy``: ``(mean, sd, lo, hi)`` over the draws
    of ``counts.sampled_accuracy`` -- the sample sd (NaN for one draw) and the 90 % equal-tailed interval (numpy's linear quantiles at
    0.05 and 0.95); ``accuracy``: one such tuple per threshold of ``counts.accuracy``; ``curve``: the ``BinaryCurve`` of
    ``mean_probability``, the float32 posterior mean probability per row (``posterior_predictive_moments``' mean); ``latents``: the
    draws' ``{"w"[, "intercept"]}``."""
    __slots__ = ()

    def lines(self):
        c, out = self.curve, []
        m, sd, lo, hi = self.sampled_accuracy
        out.append(f"classification report ({self.n_rows} rows, {self.n_draws} draws): sampled accuracy {m:.4f} +- {sd:.4f} [{lo:.4f}, {hi:.4f}]")
        for j, tau in enumerate(self.counts.thresholds):
            am, asd, _, _ = self.accuracy[j]
            col = lambda x: float(np.nanmean(_host(x).reshape(self.n_draws, -1)[:, j]))   # noqa: E731
            out.append(f"at threshold {tau:g}: accuracy {am:.4f} +- {asd:.4f}, TPR {col(self.counts.tpr):.4f}, FPR {col(self.counts.fpr):.4f}, "
                       f"F1 {col(self.counts.f1):.4f}")
        out.append(f"auc {c.auc:.6f} [{c.auc_lo:.6f}, {c.auc_hi:.6f}], KS {c.ks:.4f}, ECE {c.ece:.4f} (MCE {c.mce:.4f}, {c.bins} bins)")
        return out


def _host(x):
    return np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64)


# ------------------------------------------------------------------------------------------------ the host checks
def _family(model):
    fam = P._family(model)   # (TypeError for a model without a linear predictor, in that module's wording)
    if fam != _lib.D3P_FAMILY_LOGREG:
        raise TypeError(f"classification: unsupported model {type(model).__name__} (LogisticRegression has the 0 / 1 outcomes a confusion "
                        "count compares)")
    return fam


def _check_guide(model, guide):
    if not isinstance(guide, (AutoDiagonalNormal, DiagonalNormalGuide)):
        raise TypeError(f"classification: guide {type(guide).__name__} is not supported with {type(model).__name__} (AutoDiagonalNormal, "
                        "DiagonalNormalGuide)")


def _thresholds(thresholds):
    """The thresholds as a tuple of at most four float32 values (held as Python floats); a NaN is accepted and counts nothing."""
    if isinstance(thresholds, (int, float)) and not isinstance(thresholds, bool):
        thresholds = (thresholds,)
    try:
        tau = np.asarray(list(thresholds), dtype=np.float32).reshape(-1)
    except (TypeError, ValueError) as e:
        raise ValueError("thresholds: a sequence of numbers is required") from e
    if tau.size > MAX_THRESHOLDS:
        raise ValueError(f"thresholds: {tau.size} given; one launch counts at most {MAX_THRESHOLDS} (T <= {MAX_THRESHOLDS})")
    return tuple(float(t) for t in tau)


def _binary(y, rows, what):
    """((rows,) int32 labels in {0, 1} on whatever device they lie, the number of ones): scoring._observations' reading of y, with
    the one check a label needs -- every value 0 or 1, which a NaN, a fraction and a value beyond int32 all fail -- and the class total
    in ONE read-back."""
    if not isinstance(y, torch.Tensor):
        try:
            y = torch.as_tensor(np.asarray(y))
        except (TypeError, ValueError, RuntimeError) as e:
            raise ValueError(f"{what}: y is not an array of numbers") from e
    y = y.detach()
    if y.numel() != rows:
        raise ValueError(f"{what}: y: {rows} labels expected (one per row), got {y.numel()}")
    if y.is_complex():
        raise ValueError(f"{what}: y must hold 0 / 1 labels, got {y.dtype}")
    y = y.reshape(rows)
    one = y == 1
    ok, n_pos = torch.stack([((y == 0) | one).all().to(torch.int64), one.sum()]).tolist()
    if not ok:
        raise ValueError(f"{what}: y: the labels must be 0 or 1")
    return y.to(torch.int32), int(n_pos)


def _labels(model, model_args, rows, what):
    if not isinstance(model_args, (tuple, list)) or len(model_args) < 2 or model_args[1] is None:
        raise ValueError("y is missing: model_args = (X, y[, N]); a confusion count compares with the observed labels")
    return _binary(model_args[1], rows, what)


def _bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= 64:
        raise ValueError(f"bins must be an int in 1..64, got {bins!r}")
    return int(bins)


# ------------------------------------------------------------------------------------------------ the confusion counts
def _counts(model, fam, X, y, rows, d, n, latent, obs_keys, tau):
    """d3p_predict_confusion over latent = (tensor at the first latent row, ld, w_off, b_col): (10, n) int64 on the current GPU (the
    entry's uint64 counts, all below 2^32).  y: int32 labels; read by the kernel as float32."""
    first, ld, w_off, b_col = latent
    X = M._f32(X, "X")
    yf = y.to(X.device).to(torch.float32).contiguous()
    out = torch.empty((2 + 2 * MAX_THRESHOLDS, n), dtype=torch.int64, device=X.device)
    ms = _model_struct(model, fam, d)
    taus = (C.c_float * MAX_THRESHOLDS)(*tau)
    check(_lib.load().d3p_predict_confusion(stream_ptr(), C.byref(ms), ptr(X), ptr(yf), rows, d, ptr(first), ld, w_off, b_col, n, ptr(obs_keys),
                                            taus, len(tau), ptr(out)))
    return out


def _result(out, n_pos, rows, tau, single=False):
    T = len(tau)
    tp = out[2:2 + 2 * T:2].t().contiguous() if T else out.new_zeros((out.shape[1], 0))
    fp = out[3:3 + 2 * T:2].t().contiguous() if T else out.new_zeros((out.shape[1], 0))
    if single:
        return ConfusionCounts(out[0, 0], out[1, 0], tp[0], fp[0], n_pos, rows - n_pos, int(rows), tau)
    return ConfusionCounts(out[0], out[1], tp, fp, n_pos, rows - n_pos, int(rows), tau)


def predictive_confusion(rng_key, model, posterior_samples, *model_args, thresholds=(0.5,), **kwargs):
    """The counts over given samples: ``model_args = (X, y[, N])``, ``posterior_samples`` as for ``predictive_samples``, whose key rule
    the sampled labels follow (draw ``s`` uses the ``obs`` key ``split(rng_key, n)[s]``): ``agree[s]`` equals ``(obs[s] == y).sum()`` of
    that call by value, and ``tp`` / ``fp`` those of the matrix ``d3p_predict_mean_rows`` stores.  ``y``: 0 / 1 labels (integral values;
    anything else raises ``ValueError``).  ``thresholds``: at most four numbers, compared as float32.  A single sample (``w`` of shape
    ``(d,)``) gives ``agree`` of shape ``()`` and ``tp`` of shape ``(T,)``."""
    what = "predictive_confusion"
    fam = _family(model)
    tau = _thresholds(thresholds)
    rows, d = P._data(model, model_args, kwargs)
    y, n_pos = _labels(model, model_args, rows, what)
    n, single = _sample_shape(model, posterior_samples, d)
    key = M._check_key(rng_key)
    _lib.require_device()   # (every check above runs without a device)
    dev = key.device
    with torch.cuda.device(dev):
        obs_keys = torch.empty((n, 2), dtype=torch.uint32, device=dev)
        check(_lib.load().d3p_tf_split(stream_ptr(), ptr(key), n, ptr(obs_keys)))
        out = _counts(model, fam, model_args[0], y, rows, d, n, _pack(model, posterior_samples, n, d), obs_keys, tau)
    return _result(out, n_pos, rows, tau, single)


def _posterior_args(rng_key, n, model, model_args, guide, params, thresholds, kwargs, what):
    """Every refusal of the posterior forms, without a device: (fam, n, rows, d, gparams, (y, n_pos), tau)."""
    fam = _family(model)
    _check_guide(model, guide)
    tau = _thresholds(thresholds)
    fam, n, rows, d, gparams = _ppc._posterior_checks(rng_key, n, model, model_args, guide, params, kwargs)
    return fam, n, rows, d, gparams, _labels(model, model_args, rows, what), tau


def _posterior_counts(key, fam, n, rows, d, gparams, model, X, labels, guide, tau):
    y, n_pos = labels
    dev = key.device
    with torch.cuda.device(dev):
        latents, latent, obs_keys, _ = P._latents(key, n, model, rows, d, guide, gparams, {})
        out = _counts(model, fam, X, y, rows, d, n, latent, obs_keys, tau)
    return latents, _result(out, n_pos, rows, tau)


def posterior_predictive_confusion(rng_key, n, model, model_args, guide, params, thresholds=(0.5,), **kwargs):
    """``posterior_predictive_samples`` with ``obs`` and the probability compared with ``y`` instead of stored:
    ``({"w": (n, d)[, "intercept": (n,)]}, ConfusionCounts)``.  The latents are that call's, bit for bit (the same key rule, the same
    launch), the sampled labels use its obs keys and row indices, so ``agree[s]`` equals ``(obs[s] == y).sum()`` of that call by value --
    and ``agree.sum() / (n rows)`` is the example's ``estimate_accuracy`` for the same key.  ``model_args = (X, y[, N])``."""
    fam, n, rows, d, gparams, labels, tau = _posterior_args(rng_key, n, model, model_args, guide, params, thresholds, kwargs,
                                                            "posterior_predictive_confusion")
    key = M._check_key(rng_key)
    _lib.require_device()
    return _posterior_counts(key, fam, n, rows, d, gparams, model, model_args[0], labels, guide, tau)


# ------------------------------------------------------------------------------------------------ the curve of one score vector
def binary_curve(p, y, bins=10):
    """ROC histogram, AUC with its certificate, KS statistic and reliability table (ECE, MCE over ``bins`` equal bins, 1..64) of the
    scores ``p`` -- a 1-D float32 CUDA tensor of at most 2^27 probabilities in [0, 1] -- against the 0 / 1 labels ``y`` (a tensor or an
    array of as many values).  A score that is NaN or outside [0, 1] raises ``ValueError``, as a label outside {0, 1} does.  The
    tables stay on the GPU; the 48-byte summary and the reliability table come to the host in one copy."""
    what = "binary_curve"
    if not isinstance(p, torch.Tensor):
        raise TypeError(f"{what}: p must be a CUDA tensor (there is no CPU path), got {type(p).__name__}")
    if p.dtype != torch.float32:
        raise TypeError(f"{what}: p must be float32, got {p.dtype}")
    if p.dim() != 1 or p.numel() < 1:
        raise ValueError(f"{what}: p: shape (rows,) with at least one score expected, got {tuple(p.shape)}")
    rows = p.numel()
    if rows > MAX_CURVE_ROWS:
        raise ValueError(f"{what}: {rows} scores; the exact fixed-point sums of the reliability table hold up to 2^27 = {MAX_CURVE_ROWS} rows")
    bins = _bins(bins)
    if not p.is_cuda:
        raise TypeError(f"{what}: p must be a CUDA tensor (there is no CPU path), got a {p.device.type} tensor")
    y, _ = _binary(y, rows, what)
    _lib.require_device()
    lib = _lib.load()
    with torch.cuda.device(p.device):
        p = p.detach().contiguous()
        y = y.to(p.device).contiguous()
        hist = torch.empty((2, CURVE_BINS), dtype=torch.int32, device=p.device)
        both = torch.empty((_SUMMARY + 3 * bins,), dtype=torch.int64, device=p.device)   # (one buffer: one read-back)
        summary, calib = both[:_SUMMARY], both[_SUMMARY:].view(3, bins)
        nbytes = int(lib.d3p_binary_curve_workspace())
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=p.device)
        check(lib.d3p_binary_curve(stream_ptr(), ptr(p), ptr(y), rows, bins, ptr(hist), ptr(calib), ptr(summary), ptr(ws), nbytes))
        host = both.cpu().numpy()
    n_invalid, P_, N_, conc, same, ks_num = (int(v) for v in host[:_SUMMARY])
    if n_invalid:
        raise ValueError(f"{what}: {n_invalid} of {rows} scores are NaN or outside [0, 1]")
    cal = host[_SUMMARY:].reshape(3, bins)
    pn = float(P_) * float(N_)   # (exact: both below 2^27)
    nan = float("nan")
    auc_lo, auc_hi, auc = (conc / pn, (conc + same) / pn, (conc + same / 2) / pn) if pn else (nan, nan, nan)
    ks = ks_num / pn if pn else nan
    ece, mce = _calibration_errors(cal, rows)
    return BinaryCurve(hist, calib, P_, N_, conc, same, auc, auc_lo, auc_hi, ks, ece, mce, bins)


def _calibration_errors(cal, rows):
    """(ece, mce) from the (3, B) table: gap_b = |pos_b / count_b - (sum_b / 2^36) / count_b| over the occupied bins, float64, one
    operation per step; ece = sum_b (count_b / rows) gap_b in ascending bin order, mce = max_b gap_b."""
    cal = np.asarray(cal).astype(np.int64)
    ece, mce = 0.0, 0.0
    for b in range(cal.shape[1]):
        count, pos, total = (int(v) for v in cal[:, b])
        if count == 0:
            continue
        gap = abs(pos / count - (total / _FIXED) / count)
        ece = ece + (count / rows) * gap
        mce = max(mce, gap)
    return ece, mce


# ------------------------------------------------------------------------------------------------ the report
def _over_draws(x):
    """(mean, sd, lo, hi) of a per-draw vector: the sample sd (NaN for one draw), numpy's linear quantiles at 0.05 and 0.95."""
    x = np.asarray(x, np.float64).reshape(-1)
    sd = float(x.std(ddof=1)) if x.size > 1 else float("nan")
    lo, hi = np.quantile(x, [0.05, 0.95])
    return float(x.mean()), sd, float(lo), float(hi)


def classification_report(rng_key, n, model, model_args, guide, params, thresholds=(0.5,), bins=10, **kwargs):
    """The confusion counts of ``n`` posterior draws at ``params``, their summaries over the draws, and the ``binary_curve`` of the
    posterior mean probability.  The ONE key is not split between the two calls: ``posterior_predictive_confusion(rng_key, n, ...)``
    and ``posterior_predictive_moments(rng_key, n, ...)`` both receive ``rng_key`` itself, and both draw the latents of draw ``i`` on
    ``split(rng_key, n)[i]`` through the guide's chain -- the latents of the two calls are IDENTICAL, so the per-draw counts and the
    mean probability describe the same ``n`` draws (``ClassificationReport.latents`` are the first call's; a test compares the
    second call's mean with ``d3p_predict_mean_rows`` of them).  The obs keys of the sampled labels come from the model's chain of the
    same split and touch no latent."""
    what = "classification_report"
    fam, n, rows, d, gparams, labels, tau = _posterior_args(rng_key, n, model, model_args, guide, params, thresholds, kwargs, what)
    bins = _bins(bins)
    if rows > MAX_CURVE_ROWS:
        raise ValueError(f"{what}: {rows} rows; binary_curve runs at most 2^27 = {MAX_CURVE_ROWS}")
    key = M._check_key(rng_key)
    _lib.require_device()
    latents, counts = _posterior_counts(key, fam, n, rows, d, gparams, model, model_args[0], labels, guide, tau)
    mean = PR.posterior_predictive_moments(rng_key, n, model, model_args, guide, params)["mean"]
    curve = binary_curve(mean, labels[0], bins)
    acc = _host(counts.accuracy).reshape(n, len(tau))
    return ClassificationReport(counts, _over_draws(_host(counts.sampled_accuracy)), [_over_draws(acc[:, j]) for j in range(len(tau))], curve,
                                mean, latents, n, rows)

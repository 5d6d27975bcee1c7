"""Credible and predictive intervals for the regression models, and a summary of the latent draws: per-row quantiles over the
posterior draws.

    quantiles(matrix, probs)                                                                      -> (Q, cols) float32
    hpdi(matrix, prob=0.9)                                                   -> (2, cols) float32, or (Q, 2, cols) for Q probabilities
    credible_interval(model, posterior_samples, X[, y[, N]], prob=0.9, probs=None, slab_bytes=64 << 20, kind="equal_tailed")
    posterior_credible_interval(rng_key, n, model, model_args, guide, params, prob=0.9, probs=None, slab_bytes=64 << 20, kind="equal_tailed")
    predictive_interval(rng_key, model, posterior_samples, X[, y[, N]], prob=0.9, probs=None, slab_bytes=64 << 20, kind="equal_tailed")
    posterior_predictive_interval(rng_key, n, model, model_args, guide, params, prob=0.9, probs=None, slab_bytes=64 << 20, kind="equal_tailed")
    latent_summary(posterior_samples, prob=0.9, interval="equal_tailed")    -> {site: {"mean", "std", "median", "lower", "upper"}}

The interval functions return ``{"lower": (rows,), "median": (rows,), "upper": (rows,)}`` float32 on the GPU at the probabilities
``((1 - prob) / 2, 0.5, (1 + prob) / 2)``, the equal-tailed interval; with ``probs`` (1 to 8 floats in [0, 1]) they return
``{"quantiles": (Q, rows)}`` at those probabilities instead.

``quantiles`` is the model-free reduction (``d3p_col_quantiles``, ``d3p_amd/csrc/d3p_quantiles.hip``): the quantiles of every column
of a float32 or int32 ``(draws, cols)`` CUDA matrix with unit column stride and any row stride.  The quantile rule is numpy's
``method='linear'``: with ``h = (n - 1) p`` in float64, ``lo = floor(h)`` and ``g = h - lo`` -- computed HERE, in Python floats, so
that the device does no arithmetic on ``p`` -- the result lies between the (lo+1)-th smallest value ``a`` and the next ``b``:
``a + (b - a) g`` where ``g < 0.5``, else ``b - (b - a) (1 - g)``, in float64 on the exactly selected values, rounded to float32 once
(an int32 count above 2^24 therefore rounds).  -0 and +0 are one value; a NaN in a column makes the column's outputs NaN; between
``-inf`` and ``+inf`` the result is NaN, between a finite value and an infinity that infinity.  ``n <= 65535``.

``hpdi`` is the highest-density interval (``d3p_col_hpdi``, ``d3p_amd/csrc/d3p_hpdi.hip``), the rule of
``numpyro.diagnostics.hpdi(x, prob, axis=0)`` and so the "5.0%" / "95.0%" columns of numpyro's ``print_summary``: with the column sorted
ascending as ``s`` and ``L = int(prob * n)`` -- computed HERE, in Python floats -- the narrowest window ``(s[i], s[i + L])``, the first
of equal ones.  Both ends are stored values (an int32 count is cast to float32 once); a float32 width is the float32 difference, an int32
width the exact one; a NaN width (``inf - inf``) is the narrowest, as for ``np.argmin``; -0 and +0 are one value; a NaN in a column
makes both ends NaN.  The column is sorted in LDS, which bounds the draws: ``n <= d3p_col_hpdi_max_n()`` = 18432, a ``ValueError``
above.  The four interval functions take ``kind="hpdi"`` and then return ``{"lower", "upper"}`` at ``prob`` (``probs`` is refused);
``latent_summary`` takes ``interval="hpdi"``: ``lower`` and ``upper`` from ``d3p_col_hpdi``, ``median`` still from
``d3p_col_quantiles``.  Slabs are as below: the reducer is the only difference.

``credible_interval`` is over ``mu[s, r] = E[y | x_r, draw s] = sigmoid(t) | t | exp(t)``, the uncertainty of the regression function
(``LogisticRegression | LinearRegression | PoissonRegression``; ``t`` and the link exactly as ``d3p_amd.prediction`` forms them).
``predictive_interval`` is over draws of ``obs``: ``LinearRegression`` (float32 outcomes) and ``PoissonRegression`` (int32 counts),
the outcomes ``d3p_amd.predictive.predictive_samples`` returns for the same key; ``LogisticRegression`` raises ``TypeError`` there,
since an outcome in {0, 1} has no useful quantiles -- ``credible_interval`` gives the interval of its probability.  Every other
model raises ``TypeError``.

Slabs.  The credible forms write the ``n x rows`` matrix in row slabs exactly as ``criteria.loo`` does: chunks of ``max(128,
(slab_bytes // (4 n)) // 128 * 128)`` rows, each written by ``d3p_predict_mean_rows`` on the row range into one reused buffer and
reduced by ``d3p_col_quantiles`` into the rows' part of the output on the same stream; the latents are packed once and the result
does not depend on ``slab_bytes``.  The predictive forms are NOT cut into slabs: ``d3p_predict_glm`` indexes a draw's random stream
by ``(rows, r)`` -- the whole table's row count and the row's index in it -- and has no row offset, so a row range would receive other
outcomes than the whole-table call of ``predictive_samples``.  The entry is left as it is: the predictive matrix is written whole
when its ``4 n rows`` bytes fit ``slab_bytes``, and a ``ValueError`` that names the required ``slab_bytes`` is raised when they do not.

Keys are those of ``d3p_amd.predictive``.  ``posterior_credible_interval`` draws the latents through ``infer_util._guide_latents``, the
draws ``posterior_predictive_moments`` and ``posterior_predictive_samples`` use for the same key and ``n``;
``posterior_predictive_interval`` reduces the ``obs`` of ``posterior_predictive_samples`` itself.  Every host check runs before the
device is touched; there is no CPU fallback.
"""
import ctypes as C
import math

import torch

from . import _lib
from . import infer_util as U
from . import modelling as M
from . import prediction as PM
from . import predictive as PS
from ._lib import check, ptr, stream_ptr

__all__ = ["quantiles", "hpdi", "credible_interval", "posterior_credible_interval", "predictive_interval", "posterior_predictive_interval",
           "latent_summary"]

MAX_PROBS = 8
MAX_DRAWS = 65535
KINDS = ("equal_tailed", "hpdi")


def _family(model, what):
    fam = U._FAMILY.get(type(model))
    if fam is None:
        raise TypeError(f"{what}: unsupported model {type(model).__name__} (LogisticRegression, LinearRegression and PoissonRegression "
                        "have intervals over a linear predictor)")
    return fam


def _prob(prob):
    if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0.0 < float(prob) < 1.0:
        raise ValueError(f"prob must be a float in (0, 1), got {prob!r}")
    return float(prob)


def _probs(probs):
    """`probs` as a tuple of 1 to 8 floats in [0, 1]."""
    try:
        ps = tuple(float(p) for p in probs)
    except TypeError:
        raise ValueError("probs: a sequence of 1 to 8 floats in [0, 1] is required") from None
    if not 1 <= len(ps) <= MAX_PROBS:
        raise ValueError(f"probs: 1 to {MAX_PROBS} probabilities per call, got {len(ps)}")
    for p in ps:
        if not 0.0 <= p <= 1.0:   # (a NaN fails both comparisons)
            raise ValueError(f"probs: every probability must lie in [0, 1], got {p!r}")
    return ps


def positions(probs, n):
    """[(lo, g)] of the probabilities over n draws: h = (n - 1) p in float64, lo = floor(h), g = h - lo."""
    out = []
    for p in probs:
        h = (n - 1) * float(p)
        lo = int(math.floor(h))
        out.append((lo, h - lo))
    return out


def window_lengths(probs, n):
    """[L] of the probabilities over n draws: L = int(prob n) in Python floats, numpyro.diagnostics.hpdi's window length."""
    return [int(float(p) * n) for p in probs]


def hpdi_max_draws():
    """d3p_col_hpdi_max_n(): the largest draw count whose column is sorted in LDS (host only: no device is touched)."""
    return int(_lib.load().d3p_col_hpdi_max_n())


def _check_draws(n, what):
    if n > MAX_DRAWS:
        raise ValueError(f"{what}: {n} draws; the quantile kernel runs at most {MAX_DRAWS} draws (n <= {MAX_DRAWS})")


def _check_hpdi_draws(n, what):
    most = hpdi_max_draws()
    if n > most:
        raise ValueError(f"{what}: {n} draws; the highest-density interval sorts a column in LDS and runs at most {most} draws (n <= {most})")


def _position_args(probs, n):
    pos = positions(probs, n)
    return (C.c_uint32 * len(pos))(*[p[0] for p in pos]), (C.c_double * len(pos))(*[p[1] for p in pos])


def _window_args(probs, n):
    return ((C.c_uint32 * len(probs))(*window_lengths(probs, n)),)


class _Rule:
    """One reduction of the columns of a (draws, cols) matrix, built once per call: the probabilities, the names of the result's rows
    (None: one "quantiles" matrix), the entry of libd3p_hip that reduces, the output rows it writes, its per-n host arrays (a function of
    (probs, n)) and its extra limit on the draws (None: the quantile kernel's alone)."""
    __slots__ = ("probs", "names", "entry", "out_rows", "per_n", "limit")

    def __init__(self, probs, names, entry, rows_per_prob, per_n, limit):
        self.probs, self.names, self.entry, self.per_n, self.limit = probs, names, entry, per_n, limit
        self.out_rows = rows_per_prob * len(probs)

    def check_draws(self, n, what):
        _check_draws(n, what)   # (the quantile kernel's limit is named first whatever the rule)
        if self.limit is not None:
            self.limit(n, what)

    def args(self, n):
        return self.per_n(self.probs, n)

    def reduce(self, first, dtype, ld, n, cols, args, out, out_ld):
        """The (n, cols) matrix that starts at tensor `first`, reduced into out (a tensor at the first output element): out_rows rows."""
        check(getattr(_lib.load(), self.entry)(stream_ptr(), ptr(first), 0 if dtype == torch.float32 else 1, ld, n, cols, len(self.probs), *args,
                                               ptr(out), out_ld))

    def result(self, q):
        return {"quantiles": q} if self.names is None else {name: q[i] for i, name in enumerate(self.names)}


def _equal_tailed(probs, names=None):     # one row per probability, from the positions (lo, g)
    return _Rule(probs, names, "d3p_col_quantiles", 1, _position_args, None)


def _highest_density(probs, names=None):  # lower and upper per probability, from the window lengths
    return _Rule(probs, names, "d3p_col_hpdi", 2, _window_args, _check_hpdi_draws)


def _rule(kind, prob, probs, name="kind"):
    """The rule of an interval function.  An unknown kind is an error, and so is `probs` with kind='hpdi'."""
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError(f"{name} must be one of {KINDS}, got {kind!r}")
    if kind == "hpdi":
        if probs is not None:
            raise ValueError(f"probs cannot be combined with {name}='hpdi': a highest-density interval is given by prob alone")
        return _highest_density((_prob(prob),), ("lower", "upper"))
    if probs is not None:
        return _equal_tailed(_probs(probs))
    prob = _prob(prob)
    return _equal_tailed(((1.0 - prob) / 2.0, 0.5, (1.0 + prob) / 2.0), ("lower", "median", "upper"))


def _row_stride(m, n, cols):
    return int(m.stride(0)) if n > 1 else cols


def _check_matrix(matrix, what, check_draws):
    """(n, cols, ld) of a reducer's matrix after the host checks; `what` names the caller in the messages."""
    if not isinstance(matrix, torch.Tensor) or matrix.dim() != 2 or matrix.dtype not in (torch.float32, torch.int32) or not matrix.is_cuda:
        raise ValueError(f"{what}: a 2-D float32 or int32 CUDA tensor (draws, cols) is required")
    n, cols = int(matrix.shape[0]), int(matrix.shape[1])
    if cols > 1 and matrix.stride(1) != 1:
        raise ValueError(f"{what}: the matrix's columns must have unit stride (rows may be strided)")
    if n < 1:
        raise ValueError(f"{what}: at least one draw")
    check_draws(n, what)
    ld = _row_stride(matrix, n, cols)
    if ld < cols:
        raise ValueError(f"{what}: the matrix's rows overlap (row stride below the column count)")
    return n, cols, ld


def _reduce_matrix(rule, matrix, what):
    """(rule.out_rows, cols) float32 on the matrix's device.  The draws are held to the reducer's own limit alone."""
    n, cols, ld = _check_matrix(matrix, what, rule.limit or _check_draws)
    args = rule.args(n)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(matrix.device):
        out = torch.empty((rule.out_rows, cols), dtype=torch.float32, device=matrix.device)
        if cols:
            rule.reduce(matrix, matrix.dtype, ld, n, cols, args, out, cols)
    return out


def quantiles(matrix, probs):
    """The quantiles of every column of ``matrix`` -- a 2-D CUDA tensor ``(draws, cols)``, float32 or int32, any row stride, unit column
    stride -- at ``probs`` (1 to 8 floats in [0, 1]): ``(Q, cols)`` float32 on the matrix's device, numpy's ``method='linear'`` on the
    exactly selected order statistics (module docstring)."""
    return _reduce_matrix(_equal_tailed(_probs(probs if probs is not None else ())), matrix, "quantiles")


def hpdi(matrix, prob=0.9):
    """The highest-density interval of every column of ``matrix`` -- as for ``quantiles``: a 2-D CUDA tensor ``(draws, cols)``, float32
    or int32, any row stride, unit column stride -- numpyro's ``hpdi(x, prob, axis=0)`` (module docstring).  A float ``prob`` in (0, 1)
    returns ``(2, cols)`` float32, lower and upper; a sequence of 1 to 8 such floats ``(Q, 2, cols)``, all from one sort."""
    if isinstance(prob, (int, float)):
        ps, single = (_prob(prob),), True
    else:
        try:
            ps = tuple(prob)
        except TypeError:
            raise ValueError(f"prob must be a float in (0, 1) or a sequence of 1 to {MAX_PROBS} of them, got {prob!r}") from None
        if not 1 <= len(ps) <= MAX_PROBS:
            raise ValueError(f"prob: 1 to {MAX_PROBS} probabilities per call, got {len(ps)}")
        ps, single = tuple(_prob(p) for p in ps), False
    out = _reduce_matrix(_highest_density(ps), matrix, "hpdi")
    return out if single else out.reshape(len(ps), 2, out.shape[1])


def _mean_slabs(model, fam, X, rows, d, n, latent, rule, chunk):
    """(rule.out_rows, rows) float32: mu[:, r] reduced over the draws, the n x rows matrix written and reduced in row slabs of `chunk`."""
    first, ld, w_off, b_col = latent
    X = M._f32(X, "X")
    lib = _lib.load()
    ms = U._model_struct(model, fam, d)
    args = None
    out = torch.empty((rule.out_rows, rows), dtype=torch.float32, device=X.device)
    buf = torch.empty((n * min(chunk, rows),), dtype=torch.float32, device=X.device)
    for lo in range(0, rows, chunk):
        count = min(chunk, rows - lo)
        check(lib.d3p_predict_mean_rows(stream_ptr(), C.byref(ms), ptr(X[lo:lo + count]), count, ptr(first), ld, w_off, b_col, n, ptr(buf), count))
        args = args or rule.args(n)   # (once, behind the first launch: the host builds them while the kernel runs)
        rule.reduce(buf, torch.float32, count, n, count, args, out[0, lo:], rows)
    return out


def credible_interval(model, posterior_samples, *model_args, prob=0.9, probs=None, slab_bytes=64 << 20, kind="equal_tailed", **kwargs):
    """The equal-tailed ``prob`` interval and the median of ``mu[s, r] = E[y | x_r, draw s]`` over given posterior draws, per row:
    ``{"lower", "median", "upper"}`` (or ``{"quantiles"}`` with ``probs``), float32 on the GPU (module docstring).

    ``model_args = (X[, y[, N]])``; ``y`` and ``N`` are accepted and not read.  ``posterior_samples = {"w": (n, d)[, "intercept":
    (n,) or (n, 1)]}`` as for ``predictive_moments``: packed views are read in place, everything else is packed once.
    ``kind="hpdi"``: the highest-density interval at ``prob`` instead, ``{"lower", "upper"}``."""
    fam = _family(model, "credible_interval")
    rule = _rule(kind, prob, probs)
    rows, d = PM._data(model, model_args)
    n, _ = U._sample_shape(model, posterior_samples, d)
    rule.check_draws(n, "credible_interval")
    chunk = U._loo_chunk(n, slab_bytes)
    if chunk is None:
        raise ValueError("slab_bytes must be an int >= 1, got None")
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(M._device()):
        q = _mean_slabs(model, fam, model_args[0], rows, d, n, U._pack(model, posterior_samples, n, d), rule, chunk)
    return rule.result(q)


def posterior_credible_interval(rng_key, n, model, model_args, guide, params, prob=0.9, probs=None, slab_bytes=64 << 20, kind="equal_tailed",
                                **kwargs):
    """``credible_interval`` over ``n`` draws from the guide at ``params`` (as ``DPSVI.get_params`` returns them), drawn on the device on
    ``posterior_predictive_moments``' key rule and consumed there.  Guides: ``AutoDiagonalNormal``, ``DiagonalNormalGuide``;
    ``MeanFieldGuide`` for logistic regression."""
    fam = _family(model, "posterior_credible_interval")
    U._check_guide(model, guide)
    rule = _rule(kind, prob, probs)
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    rule.check_draws(n, "posterior_credible_interval")
    rows, d = PM._data(model, model_args)
    chunk = U._loo_chunk(n, slab_bytes)
    if chunk is None:
        raise ValueError("slab_bytes must be an int >= 1, got None")
    if not isinstance(params, dict):
        raise ValueError("params: the dict DPSVI.get_params returns is required")
    gparams = [(name, M._param(params, name, size)) for name, size in M._guide_param_names(guide, model, d)]
    key = M._check_key(rng_key)
    _lib.require_device()
    dev = key.device
    with torch.cuda.device(dev):
        latent = U._guide_latents(key, n, model, guide, gparams, d, rows, dev)
        q = _mean_slabs(model, fam, model_args[0], rows, d, n, latent, rule, chunk)
    return rule.result(q)


def _predictive_family(model, what):
    fam = _family(model, what)
    if fam == _lib.D3P_FAMILY_LOGREG:
        raise TypeError(f"{what}: an outcome of LogisticRegression lies in {{0, 1}} and has no useful quantiles; credible_interval gives "
                        "the interval of its probability")
    return fam


def _check_whole(n, rows, slab_bytes, what):
    """The predictive matrix is written whole (module docstring): its 4 n rows bytes must fit slab_bytes."""
    U._check_slab_bytes(slab_bytes)
    need = 4 * n * rows
    if need > slab_bytes:
        raise ValueError(f"{what}: the {n} x {rows} predictive matrix is written whole (the outcome kernel has no row offset) and needs "
                         f"slab_bytes >= {need}, got {slab_bytes}")


def _reduce_obs(obs, n, rows, rule):
    obs = obs.reshape(n, rows)
    with torch.cuda.device(obs.device):
        q = torch.empty((rule.out_rows, rows), dtype=torch.float32, device=obs.device)
        rule.reduce(obs, obs.dtype, rows, n, rows, rule.args(n), q, rows)
    return rule.result(q)


def predictive_interval(rng_key, model, posterior_samples, *model_args, prob=0.9, probs=None, slab_bytes=64 << 20, kind="equal_tailed", **kwargs):
    """The equal-tailed ``prob`` interval and the median of the outcomes ``obs`` over given posterior draws, per row: the quantiles of
    what ``predictive_samples(rng_key, model, posterior_samples, *model_args)`` returns, without that matrix leaving the device.
    ``LinearRegression`` and ``PoissonRegression``; the matrix is written whole and must fit ``slab_bytes`` (module docstring).
    ``kind="hpdi"``: the highest-density interval at ``prob`` instead, ``{"lower", "upper"}``."""
    _predictive_family(model, "predictive_interval")
    rule = _rule(kind, prob, probs)
    rows, d = PS._data(model, model_args, kwargs)
    n, _ = U._sample_shape(model, posterior_samples, d)
    rule.check_draws(n, "predictive_interval")
    _check_whole(n, rows, slab_bytes, "predictive_interval")
    M._check_key(rng_key)
    obs = PS.predictive_samples(rng_key, model, posterior_samples, *model_args, **kwargs)
    return _reduce_obs(obs, n, rows, rule)


def posterior_predictive_interval(rng_key, n, model, model_args, guide, params, prob=0.9, probs=None, slab_bytes=64 << 20, kind="equal_tailed",
                                  **kwargs):
    """``predictive_interval`` over ``n`` draws from the posterior predictive at ``params``: the quantiles of the ``obs`` that
    ``posterior_predictive_samples(rng_key, n, model, model_args, guide, params)`` returns for the same key."""
    _predictive_family(model, "posterior_predictive_interval")
    U._check_guide(model, guide)
    rule = _rule(kind, prob, probs)
    n = PS._count(n)
    rule.check_draws(n, "posterior_predictive_interval")
    rows, d = PS._data(model, model_args, kwargs)
    _check_whole(n, rows, slab_bytes, "posterior_predictive_interval")
    obs = PS.posterior_predictive_samples(rng_key, n, model, model_args, guide, params, **kwargs)["obs"]
    return _reduce_obs(obs, n, rows, rule)


def latent_summary(posterior_samples, prob=0.9, interval="equal_tailed"):
    """Per site of ``posterior_samples`` (``w``, ``intercept``; each viewed as an ``n x D`` matrix of draws): ``{"mean", "std", "median",
    "lower", "upper"}``, each of the site's shape without the draw axis -- the columns of numpyro's ``print_summary`` without ``n_eff``
    and ``r_hat``, which are meaningless for independent draws from a guide.  ``mean`` and ``std`` are float64 from ``d3p_col_stats``
    (the ``n - 1`` variance: ``n == 1`` gives a NaN ``std``); the three quantiles are float32 from ``d3p_col_quantiles`` at ``((1 -
    prob) / 2, 0.5, (1 + prob) / 2)``.  ``interval="hpdi"``: ``lower`` and ``upper`` are the highest-density interval at ``prob`` from
    ``d3p_col_hpdi`` -- what ``print_summary`` reports -- and ``median`` still comes from ``d3p_col_quantiles``."""
    # hpdi: rows 0 and 1 are the interval's ends, row 2 the median
    rules = [_rule(interval, prob, None, "interval")] + ([_equal_tailed((0.5,), ("median",))] if interval == "hpdi" else [])
    if not isinstance(posterior_samples, dict) or not posterior_samples:
        raise ValueError("posterior_samples: a dict of sites (n draws each) is required")
    shapes = {}
    for name, v in posterior_samples.items():
        shp = tuple(v.shape) if hasattr(v, "shape") else ()
        if len(shp) < 1 or shp[0] < 1 or M._numel(v) == 0:
            raise ValueError(f"posterior_samples['{name}']: at least one draw along the first axis is required")
        rules[0].check_draws(shp[0], "latent_summary")
        shapes[name] = shp
    _lib.require_device()   # (every check above runs without a device)
    lib = _lib.load()
    out = {}
    for name, v in posterior_samples.items():
        shp = shapes[name]
        n = shp[0]
        with torch.cuda.device(M._device()):
            m = v.detach() if isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 else M._f32(v, f"posterior_samples['{name}']")
            m = m.reshape(n, -1)
            cols = int(m.shape[1])
            if cols > 1 and m.stride(1) != 1:
                m = m.contiguous()
            ld = _row_stride(m, n, cols)
            if ld < cols:
                m, ld = m.contiguous(), cols
            with torch.cuda.device(m.device):
                stats = torch.empty((4, cols), dtype=torch.float64, device=m.device)
                check(lib.d3p_col_stats(stream_ptr(), ptr(m), ld, n, cols, ptr(stats)))
                q = torch.empty((3, cols), dtype=torch.float32, device=m.device)
                site, row = {"mean": stats[0], "std": torch.sqrt(stats[1])}, 0
                for rule in rules:
                    rule.reduce(m, torch.float32, ld, n, cols, rule.args(n), q[row], cols)
                    site.update(rule.result(q[row:]))
                    row += rule.out_rows
        out[name] = {k: t.reshape(shp[1:]) for k, t in site.items()}
    return out

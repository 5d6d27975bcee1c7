"""Comparator of d3p_amd.infer_util (log_likelihood, log predictive density) for tests/test_loglik_host.py and
tests/test_gpu_loglik.py: float64 on the CPU.

    t[s, r]  = X64[r] . w64[s] + b[s]
    ll[s, r] = tests.glm_ref._loglik(family, t, y, sigma)             (torch.distributions in float64, UNSCALED)
    lppd[r]  = logsumexp_s ll[s, r] - log n                           (max-shifted sum in float64, no scipy)

The device works in float32 and does not clamp: a Poisson rate exp(t) beyond float32's largest number is inf there and the
log-likelihood -inf (as in float32 jax).  float64 would carry such a rate, so ``ll64`` applies float32's RANGE (nothing else of
float32): ll = -inf where exp(t) > 3.4028235e38.  -inf entries are compared by equality and NaN never passes (``assert_close``).

Per-element bound:  |ll_dev - ll64| <= |dll/dt| band_t + link_tol
  * band_t: the float32 product's bound (d + 2) 2^-23 (sum |x w| + |b|), taken from tests.predictive_ref.logreg_band (whose linear
    form is band_t / 4 + 2^-21);
  * |dll/dt| in float64: |sigmoid(t) - y| (logistic), |t - y| / sigma^2 (linear), |exp(t) - y| (Poisson);
  * link_tol = LINK_RTOL[family] (|ll64| + 0.1 max |ll64|), the maximum over the draw's finite entries: the link's own rounding in the form of the
    project's check.  It is not taken from the device.  ``float32_link_calibration`` evaluates the same likelihood through float32
    torch against float64 GIVEN THE SAME float32 t (formed in float32 on the CPU) over the inputs of this file's sweep
    (``sweep_cases``); LINK_RTOL is four times the smallest passing rtol, the margin tests/glm_ref.py and tests/predictive_ref.py use.
    Measured on the CPU (tests/test_loglik_host.py recomputes the figures and asserts that none has grown):

        logistic 4.133e-07  worst at (n, rows, d, intercept) = (257, 129, 31, True)
        linear   1.841e-07  worst at (128, 1, 32, True)
        poisson  3.662e-07  worst at (129, 128, 1, True)

lppd bound: the largest of its draws' ll bounds (finite draws) + 4 x 2^-23 max(1, |lppd|).  The second term is for the
log-sum-exp itself: per merged partial (at most 3 here: the sweep's largest n = 257 is three draw tiles of 128) one rounding of
the running sum and one exponential, and the final logarithm and subtraction.
"""
import math

import numpy as np
import torch

from tests import glm_ref as R
from tests import predictive_ref as P

FAMILIES = R.FAMILIES
SIGMA = R.SWEEP_SIGMA
F32_MAX = float(np.finfo(np.float32).max)
LINK_MEASURED = {"logistic": 4.133e-07, "linear": 1.841e-07, "poisson": 3.662e-07}
LINK_RTOL = {f: 4 * v for f, v in LINK_MEASURED.items()}
LPPD_EXTRA = 4 * 2.0 ** -23

# (n, rows, d): every value of n in {1, 31, 128, 129, 257}, rows in {1, 63, 128, 129, 300} and d in {1, 31, 32, 33, 513} -- the draw
# tile 128, the row tile 128, the K slice 32 and the half-wave 32, each from below, exactly and from above -- meets at least two
# values of each other axis; the corner (257, 300, 513) comes once per family (with an intercept).
SHAPES = [(1, 1, 1), (1, 63, 31), (31, 128, 32), (31, 129, 33), (128, 300, 513), (128, 1, 32), (129, 63, 33), (129, 128, 1),
          (257, 129, 31), (31, 300, 32), (129, 63, 513)]
CORNER = (257, 300, 513)


def sweep_cases():
    """(family, n, rows, d, intercept) of the tile-edge sweep."""
    out = []
    for family in FAMILIES:
        for n, rows, d in SHAPES:
            for intercept in (False, True):
                out.append((family, n, rows, d, intercept))
        out.append((family,) + CORNER + (True,))
    return out


def inputs(family, n, rows, d, intercept, seed=None):
    """(X (rows, d), y (rows,), W (n, d), b (n,) or None) float32: glm_ref.problem's features, labels and guide parameters, the n draws
    w_s = loc + softplus(unc) eps_s (|t| <= 4)."""
    seed = 7 + 1000 * d + 10 * rows + n + int(intercept) if seed is None else seed
    X, y, loc, unc = R.problem(family, rows, d, intercept, seed, SIGMA[family])
    D = d + int(intercept)
    eps = np.random.default_rng(seed + 1).normal(size=(n, D))
    Z = (loc.astype(np.float64) + np.logaddexp(0.0, unc.astype(np.float64)) * eps).astype(np.float32)
    return X, y, np.ascontiguousarray(Z[:, :d]), (np.ascontiguousarray(Z[:, d]) if intercept else None)


def linear_predictor(X, W, b):
    """t (n, rows) in float64."""
    t = W.astype(np.float64) @ X.astype(np.float64).T
    return t if b is None else t + np.asarray(b, np.float64).reshape(-1, 1)


def ll_of_t(family, t, y, sigma, dtype=torch.float64):
    """glm_ref._loglik at t (n, rows) in `dtype`, with float32's range for the Poisson rate (module docstring); float64 numpy."""
    tt = torch.as_tensor(np.asarray(t), dtype=dtype)
    yy = torch.as_tensor(np.asarray(y), dtype=dtype).reshape(1, -1)
    ll = R._loglik(family, tt, yy, sigma).to(torch.float64).numpy().copy()
    if family == "poisson":
        with np.errstate(over="ignore"):
            ll[np.exp(np.asarray(t, np.float64)) > F32_MAX] = -np.inf
    return ll


def ll64(family, X, y, W, b, sigma):
    return ll_of_t(family, linear_predictor(X, W, b), y, sigma)


def logsumexp_rows(ll):
    """logsumexp over axis 0 in float64; a column of -inf gives -inf (not NaN)."""
    ll = np.asarray(ll, np.float64)
    m = ll.max(axis=0)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), safe + np.log(np.exp(ll - safe).sum(axis=0)), m)


def lppd64(ll):
    return logsumexp_rows(ll) - math.log(np.asarray(ll).shape[0])


def dll_dt(family, t, y, sigma):
    t, y = np.asarray(t, np.float64), np.asarray(y, np.float64).reshape(1, -1)
    if family == "logistic":
        return np.abs(P.expit(t) - y)
    if family == "linear":
        return np.abs(t - y) / sigma ** 2
    with np.errstate(over="ignore"):
        return np.abs(np.exp(t) - y)


def product_band(X, W, b, d):
    """band_t (n, rows): predictive_ref.logreg_band's product bound, draw by draw (its linear form is band_t / 4 + 2^-21)."""
    X64 = X.astype(np.float64)
    return np.stack([4.0 * (P.logreg_band(X64, W[s].astype(np.float64), 0.0 if b is None else float(b[s]), d) - 2.0 ** -21)
                     for s in range(W.shape[0])])


def ll_bound(family, X, y, W, b, sigma, ll=None):
    """The per-element bound (n, rows); entries whose ll64 is not finite get 0 (they are compared by equality)."""
    t = linear_predictor(X, W, b)
    ll = ll64(family, X, y, W, b, sigma) if ll is None else ll
    fin = np.isfinite(ll)
    top = np.where(fin, np.abs(ll), 0.0).max(axis=1, keepdims=True)      # per draw: one draw's huge values do not loosen another's bound
    with np.errstate(invalid="ignore", over="ignore"):
        bound = dll_dt(family, t, y, sigma) * product_band(X, W, b, X.shape[1]) + LINK_RTOL[family] * (np.abs(ll) + 0.1 * top)
    return np.where(fin, bound, 0.0)


def lppd_bound(ll, bound, lppd):
    """Largest ll bound among the row's finite draws + LPPD_EXTRA max(1, |lppd|)."""
    fin = np.isfinite(ll)
    worst = np.where(fin, bound, 0.0).max(axis=0)
    return worst + LPPD_EXTRA * np.maximum(1.0, np.abs(np.where(np.isfinite(lppd), lppd, 0.0)))


def assert_close(dev, ref, bound, what):
    """-inf by equality, everything else within the bound, NaN never; prints the worst error / bound ratio."""
    dev, ref, bound = np.asarray(dev, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert dev.shape == ref.shape, f"{what}: shape {dev.shape} != {ref.shape}"
    assert not np.isnan(dev).any(), f"{what}: NaN at {np.argwhere(np.isnan(dev))[0]}"
    assert not np.isnan(ref).any(), f"{what}: the comparator has a NaN"
    inf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(dev), inf), f"{what}: -inf entries differ ({int(np.isneginf(dev).sum())} against {int(inf.sum())})"
    assert np.isfinite(dev[~inf]).all(), f"{what}: a non-finite value where the comparator is finite"
    err = np.abs(dev[~inf] - ref[~inf])
    ratio = err / bound[~inf]
    if err.size:
        print(f"{what}: max error {err.max():.3e}, largest error / bound {ratio.max():.3f}")
    assert np.all(err <= bound[~inf]), f"{what}: error {err[ratio.argmax()]:.3e} above the bound {bound[~inf][ratio.argmax()]:.3e}"


def float32_link_calibration(family):
    """The reference's OWN float32 error of the link on the sweep's inputs: float32 torch against float64 at the same float32 t, as
    the smallest passing rtol of the project's check.  Returns (rtol, (n, rows, d, intercept) of the worst case)."""
    worst, where = 0.0, None
    for fam, n, rows, d, intercept in sweep_cases():
        if fam != family:
            continue
        X, y, W, b = inputs(family, n, rows, d, intercept)
        t32 = torch.tensor(W) @ torch.tensor(X).T
        if b is not None:
            t32 = t32 + torch.tensor(b).reshape(-1, 1)
        t32 = t32.numpy()
        a, ref = ll_of_t(family, t32, y, SIGMA[family], torch.float32), ll_of_t(family, t32, y, SIGMA[family])
        r = max(R.smallest_passing_rtol(a[s], ref[s]) for s in range(n))      # draw by draw, as ll_bound takes its maximum
        if r > worst:
            worst, where = r, (n, rows, d, intercept)
    return worst, where

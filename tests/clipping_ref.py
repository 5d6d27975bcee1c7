"""Comparator of the clipping diagnostics (d3p_amd/clipping.py).

Norms.  ``norms_ref`` is ``np.linalg.norm(G, axis=1)`` of the float64 autograd rows of ``tests/glm_ref.py`` (``px_loss_grads``), the guide
noise from the oracle's streams (``glm_ref.px_eps``): nothing of the device's arithmetic is restated.

Profile.  ``profile_ref`` is plain numpy in float64: counts by comparison in float32, sums by ``math.fsum``, quantiles by
``np.quantile(..., method="linear")`` over the finite values, rounded to float32 once.

Bound on the norms.  It is not taken from the device.  ``float32_norm_calibration`` evaluates the same ELBO through float32 torch
autograd (rows AND the norm's sum of squares in float32) against the float64 one over the very inputs of the GPU sweep
(``entry_cases``: tests/test_gpu_clipping.py::test_entry_against_float64) and returns the smallest rtol at which the project's check
|a - b| <= rtol |b| + 0.1 rtol max|b| passes on every case's vector of norms.  On the CPU (tests/test_clipping_host.py recomputes the
figures and asserts that they do not exceed what is written here):

    logistic  3.882e-07  (worst at d = 1, no intercept, 257 rows, exp guide, key noise)     CALIBRATED["logistic"] = 3.9e-07
    linear    2.183e-06  (worst at d = 4, no intercept, 1 row, exp guide, key noise)        CALIBRATED["linear"]   = 2.2e-06
    poisson   4.473e-06  (worst at d = 512, no intercept, 1 row, exp guide, stored noise)   CALIBRATED["poisson"]  = 4.5e-06

(the constants are the figures rounded up to two digits; the largest |t| of the sweep is 3.48).  NORM_TOL[family] = 4 x the constant,
the margin tests/predictive_ref.py and glm_ref.POISSON_GRAD_TOL use.  Losses stay at the project's glm_ref.PX_TOL.  The Poisson
inputs keep |t| <= 20 (``glm_ref.problem``: |t| <= 4), asserted on the float64 side."""
import math

import numpy as np
import torch

from tests import glm_ref as R

FAMILIES = R.FAMILIES
CALIBRATED = {"logistic": 3.9e-07, "linear": 2.2e-06, "poisson": 4.5e-06}
NORM_TOL = {f: 4 * v for f, v in CALIBRATED.items()}

ENTRY_WIDTHS = (1, 4, 63, 64, 65, 129, 512, 2047, 2048)
ENTRY_ROWS = (1, 63, 65, 257)
ENTRY_N = R.SWEEP_N


def entry_hyper(family, d, intercept):
    return R.sweep_hyper(family, d, intercept)


def entry_cases(O, family, d):
    """(guide, intercept, rows, onchip, seed, X, y, loc, unc, eps) for {softplus, exp} x intercept {0, 1} x rows {1, 63, 65, 257} x both
    noise sources: ``onchip`` draws eps from the oracle's key stream at jax key ``convert_to_jax_rng_key(PRNGKey(seed))`` for ONE batch
    of ``rows`` examples, otherwise eps is stored noise."""
    for guide in ("softplus", "exp"):
        for intercept in (False, True):
            D = d + int(intercept)
            for rows in ENTRY_ROWS:
                for onchip in (False, True):
                    seed = 1000 * d + 10 * rows + 4 * int(intercept) + 2 * int(guide == "exp") + int(onchip)
                    X, y, loc, unc = R.problem(family, rows, d, intercept, seed, R.SWEEP_SIGMA[family])
                    eps = (R.px_eps(O, O.convert_to_jax_rng_key(O.PRNGKey(seed)), rows, D) if onchip
                           else np.random.default_rng(seed + 2).normal(size=(rows, D)).astype(np.float32))
                    yield guide, intercept, rows, onchip, seed, X, y, loc, unc, eps


def norms_ref(family, h, loc, unc, X, y, eps, guide="softplus", dtype=torch.float64, return_t=False):
    """(norms, losses[, max |t|]) of the rows of ONE unmasked batch.  float64: both in float64.  float32: the rows from float32
    autograd and the sum of squares accumulated in float32, as a float32 implementation forms it."""
    L, G, _, _, tmax = R.px_loss_grads(family, h, loc, unc, X, y, eps, None, guide, dtype=dtype, return_t=True)
    if dtype == torch.float32:
        G32 = G.astype(np.float32)
        norms = np.sqrt((G32 * G32).sum(axis=1, dtype=np.float32)).astype(np.float64)
    else:
        norms = np.linalg.norm(G, axis=1)
    return (norms, L, tmax) if return_t else (norms, L)


def float32_norm_calibration(O, family, widths=ENTRY_WIDTHS):
    """(smallest passing rtol of the float32 norms against the float64 ones over ``entry_cases``, where it is worst, the largest |t|)."""
    worst, where, tmax = 0.0, None, 0.0
    for d in widths:
        for guide, intercept, rows, onchip, seed, X, y, loc, unc, eps in entry_cases(O, family, d):
            h = entry_hyper(family, d, intercept)
            n64, _, t = norms_ref(family, h, loc, unc, X, y, eps, guide, return_t=True)
            n32, _ = norms_ref(family, h, loc, unc, X, y, eps, guide, dtype=torch.float32)
            r = R.smallest_passing_rtol(n32, n64)
            tmax = max(tmax, t)
            if r > worst:
                worst, where = r, (d, intercept, rows, guide, onchip)
    return worst, where, tmax


def check_norms(got, ref, family, what=""):
    tol = NORM_TOL[family]
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    print(f"{what}: smallest passing rtol {R.smallest_passing_rtol(got, ref):.3e} (bound {tol:.3e})")
    np.testing.assert_allclose(got, ref, rtol=tol, atol=0.1 * tol * np.abs(ref).max(), err_msg=what)


# ---------------------------------------------------------------- the profile
def positions(probs, n):
    """[(lo, g)] over n values: h = (n - 1) p in float64, lo = floor(h), g = h - lo -- stated here on its own, not imported."""
    out = []
    for p in probs:
        h = (n - 1) * float(p)
        lo = int(math.floor(h))
        out.append((lo, h - lo))
    return out


def profile_ref(norms, thresholds, probs):
    """The profile of a float32 vector as a dict of Python numbers and tuples (the fields of ClippingProfile plus n_finite, n_clipped
    and mean_sq)."""
    v = np.asarray(norms, np.float32).reshape(-1)
    n = int(v.size)
    fin = np.isfinite(v)
    vf = v[fin]
    f = vf.astype(np.float64)
    nf = int(fin.sum())
    nan = float("nan")
    mean = math.fsum(f.tolist()) / nf if nf else nan
    mean_sq = math.fsum((f * f).tolist()) / nf if nf else nan      # (the square of a float32 is exact in float64)
    quant = tuple(float(np.float32(np.quantile(f, p, method="linear"))) if nf else nan for p in probs)
    n_clipped, factor = [], []
    for c in thresholds:
        c32 = np.float32(c)
        over = vf > c32
        n_clipped.append(int(over.sum()) + (n - nf))
        ratio = np.ones(nf, np.float64)
        ratio[over] = np.float64(c32) / f[over]
        factor.append(math.fsum(ratio.tolist()) / n)
    return dict(n=n, n_finite=nf, n_nonfinite=n - nf, mean=mean, mean_sq=mean_sq, rms=math.sqrt(mean_sq) if nf else nan,
                max=float(vf.max()) if nf else nan, probs=tuple(float(p) for p in probs), quantiles=quant,
                thresholds=tuple(float(c) for c in thresholds), n_clipped=tuple(n_clipped),
                clipped_fraction=tuple(k / n for k in n_clipped), mean_clip_factor=tuple(factor))


PROFILE_SIZES = (1, 2, 255, 256, 257, 65537, 1000003)
PROFILE_KINDS = ("normal", "constant", "two_values", "zeros_denormals", "with_nonfinite", "all_nonfinite", "equal_to_threshold")
PROFILE_PROBS = (0.0, 0.25, 0.5, 0.9, 0.95, 0.99, 0.999, 1.0)


def profile_vector(kind, n, seed=0):
    """(vector, 8 thresholds) of a kind; the thresholds of ``equal_to_threshold`` are values of the vector."""
    r = np.random.default_rng(1000 * seed + n)
    thr = (0.05, 0.25, 0.5, 0.6744898, 1.0, 1.5, 2.5, 4.0)
    if kind == "normal":
        v = np.abs(r.normal(size=n)).astype(np.float32)
    elif kind == "constant":
        v = np.full(n, 0.75, np.float32)
    elif kind == "two_values":
        v = np.where(r.random(n) < 0.3, np.float32(0.25), np.float32(3.0)).astype(np.float32)
    elif kind == "zeros_denormals":
        v = np.abs(r.normal(size=n)).astype(np.float32)
        pick = r.integers(0, 4, size=n)
        v[pick == 0] = 0.0
        v[pick == 1] = np.float32(1e-42) * r.integers(1, 1000, size=n)[pick == 1].astype(np.float32)
        v[-1] = -0.0
    elif kind == "with_nonfinite":
        v = np.abs(r.normal(size=n)).astype(np.float32)
        pick = r.integers(0, 5, size=n)
        v[pick == 0] = np.inf
        v[pick == 1] = np.nan
        v[0] = np.inf                                   # (n = 1: the only value is not finite)
    elif kind == "all_nonfinite":
        v = np.where(r.random(n) < 0.5, np.float32(np.inf), np.float32(np.nan)).astype(np.float32)
    elif kind == "equal_to_threshold":
        v = r.choice(np.asarray(thr, np.float32), size=n).astype(np.float32)
        thr = tuple(float(np.float32(c)) for c in thr)
    else:
        raise ValueError(kind)
    return v, thr

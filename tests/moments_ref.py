"""Comparator of d3p_amd.prediction (posterior predictive mean and variance) for tests/test_moments_host.py and
tests/test_gpu_moments.py: float64 on the CPU from the float32 inputs, built on tests/loglik_ref.py (inputs, linear_predictor,
product_band, SHAPES).

    t[s, r]  = X64[r] . w64[s] + b[s]
    mu[s, r] = sigmoid(t) | t | exp(t),   v[s, r] = mu (1 - mu) | sigma^2 | mu          (logistic | linear | poisson)
    mean[r]  = (1/n) sum_s mu[s, r]
    var[r]   = (1/n) sum_s v[s, r] + (1/n) sum_s (mu[s, r] - mean[r])^2                 (law of total variance, population form)

For the logistic family var = pbar qbar with p = sigmoid(t), q = sigmoid(-t), pbar and qbar their means over the draws: the same
number ((1/n) sum p q + (1/n) sum p^2 - pbar^2 = pbar - pbar^2), without the cancellation (tests/test_moments_host.py holds the two
forms against each other).

The device works in float32 and does not clamp: a Poisson rate exp(t) beyond float32's largest number is +inf there, so
``conditional_moments`` applies float32's RANGE to it (nothing else of float32), as loglik_ref.ll64 does.  Non-finite rule: a NaN t
makes its row NaN; otherwise a +inf mu in any draw makes the row (+inf, +inf) (a linear t = -inf: (-inf, +inf); both signs: NaN);
a finite float64 result beyond float32's range is the infinity it rounds to.  ``assert_close`` compares non-finite entries by
their class (NaN, +inf, -inf), everything else within the bound; no entry is skipped.

Bounds, derived per row.  The device's mu[s, r] differs from the float64 one by at most

    e[s, r] = |dmu/dt| band_t[s, r] + link_tol[s, r]

  * band_t: the float32 product's bound (d + 2) 2^-23 (sum |x w| + |b|) (loglik_ref.product_band), which covers the intercept's add;
  * |dmu/dt| in float64: p q (logistic), 1 (linear), mu (Poisson);
  * link_tol = LINK_RTOL[family] (|mu| + 0.1 max |mu|), the maximum over the draw's finite entries: the link's own float32 rounding
    in the form of the project's check.  It is not taken from the device: ``float32_link_calibration`` evaluates the link through
    float32 torch against float64 GIVEN THE SAME float32 t over the inputs of this file's sweep (``sweep_cases``) -- for the
    logistic family both sigmoid(t) and sigmoid(-t), since the kernel forms both; LINK_RTOL is four times the smallest passing rtol,
    the margin tests/glm_ref.py, tests/predictive_ref.py and tests/loglik_ref.py use.  The linear link is the identity: 0.
    Measured on the CPU (tests/test_moments_host.py recomputes the figures and asserts that none has grown):

        logistic 1.032e-07  worst at (n, rows, d, intercept) = (64, 129, 33, False)
        linear   0          (mu = t: no link rounding)
        poisson  5.415e-08  worst at (257, 129, 31, False)

Mean: the mean is linear in the mu, and rounded to float32 once:

    |mean_dev - mean| <= (1/n) sum_s e[s, r] + 2^-23 |mean|

Variance, linear and Poisson: var is a quadratic polynomial of the mu, so its Taylor expansion ends after the second order.  With
eps_s the error of mu_s (|eps_s| <= e_s) and dvar/dmu_s = (dv/dmu + 2 (mu_s - mean)) / n (dv/dmu = 0 | 1; the derivative through
the mean vanishes because sum_s (mu_s - mean) = 0):

    var(mu + eps) - var(mu) = sum_s dvar/dmu_s eps_s + (1/n) sum_s eps_s^2 - ((1/n) sum_s eps_s)^2
    |var_dev - var| <= (1/n) sum_s |dv/dmu + 2 (mu_s - mean)| e_s + (1/n) sum_s e_s^2 + 2^-23 |var|

Variance, logistic: with Ep = (1/n) sum_s e^p_s and Eq = (1/n) sum_s e^q_s the errors of pbar and qbar (same band and |dmu/dt| = p q
for both, link_tol of p resp. q),

    |var_dev - var| <= qbar Ep + pbar Eq + Ep Eq + 2^-23 |var|

The float64 roundings of the accumulation (2^-53 per operation) are not listed: they are 2^-29 of a float32 rounding each.
"""
import numpy as np
import torch

from tests import glm_ref as R
from tests import loglik_ref as LR
from tests import predictive_ref as P

FAMILIES = LR.FAMILIES
SIGMA = LR.SIGMA
F32_MAX = LR.F32_MAX
LINK_MEASURED = {"logistic": 1.032e-07, "linear": 0.0, "poisson": 5.415e-08}
LINK_RTOL = {f: 4 * v for f, v in LINK_MEASURED.items()}
ROUND = 2.0 ** -23

# n = 64 and 65 on top of loglik_ref.SHAPES: the second wave of a row block (draws 64..127 of a tile) owns no draw, and one
EXTRA_SHAPES = [(64, 129, 33), (65, 129, 33)]
CORNER = LR.CORNER


def sweep_cases():
    """(family, n, rows, d, intercept) of the tile-edge sweep."""
    out = []
    for family in FAMILIES:
        for n, rows, d in LR.SHAPES + EXTRA_SHAPES:
            for intercept in (False, True):
                out.append((family, n, rows, d, intercept))
        out.append((family,) + CORNER + (True,))
    return out


def conditional_moments(family, t, sigma):
    """(mu, v, |dmu/dt|, dv/dmu) at t (n, rows) in float64, the Poisson rate with float32's range; the logistic family's `v` is p q."""
    t = np.asarray(t, np.float64)
    if family == "logistic":
        p, q = P.expit(t), P.expit(-t)
        return p, p * q, p * q, 1.0 - 2.0 * p
    if family == "linear":
        return t, np.full_like(t, float(sigma) ** 2), np.ones_like(t), np.zeros_like(t)
    with np.errstate(over="ignore"):
        mu = np.exp(t)
    mu = np.where(mu > F32_MAX, np.inf, mu)
    return mu, mu, mu, np.ones_like(t)


def total_variance(mu, v):
    """The general law-of-total-variance expression over axis 0 (finite inputs)."""
    mean = mu.mean(axis=0)
    return v.mean(axis=0) + ((mu - mean) ** 2).mean(axis=0)


def _float32_range(x):
    with np.errstate(over="ignore"):
        x32 = x.astype(np.float32).astype(np.float64)
    return np.where(np.isinf(x32), x32, x)


def moments_of_t(family, t, sigma):
    """(mean, var) per row in float64 with the non-finite rule of the module docstring."""
    t = np.asarray(t, np.float64)
    mu, v, _, _ = conditional_moments(family, t, sigma)
    nan = np.isnan(t).any(axis=0)
    pos, neg = np.isposinf(mu).any(axis=0), np.isneginf(mu).any(axis=0)
    fin = np.where(np.isfinite(mu), mu, 0.0)
    mean = fin.mean(axis=0)
    if family == "logistic":
        var = mean * np.where(np.isnan(t), 0.0, P.expit(-t)).mean(axis=0)
    else:
        var = np.where(np.isfinite(v), v, 0.0).mean(axis=0) + ((fin - mean) ** 2).mean(axis=0)
    mean, var = _float32_range(mean), _float32_range(var)
    mean = np.where(pos & neg, np.nan, np.where(pos, np.inf, np.where(neg, -np.inf, mean)))
    var = np.where(pos & neg, np.nan, np.where(pos | neg, np.inf, var))
    return np.where(nan, np.nan, mean), np.where(nan, np.nan, var)


def moments64(family, X, W, b, sigma):
    return moments_of_t(family, LR.linear_predictor(X, W, b), sigma)


def _link_tol(family, mu):
    top = np.where(np.isfinite(mu), np.abs(mu), 0.0).max(axis=1, keepdims=True)      # per draw, as loglik_ref.ll_bound
    return LINK_RTOL[family] * (np.abs(mu) + 0.1 * top)


def bounds(family, X, W, b, sigma):
    """(mean bound, variance bound) per row (module docstring); rows whose comparator value is not finite get 0 (compared by class)."""
    t = LR.linear_predictor(X, W, b)
    n = t.shape[0]
    mu, v, dmu, dv = conditional_moments(family, t, sigma)
    band = LR.product_band(X, W, b, X.shape[1])
    mean, var = moments_of_t(family, t, sigma)
    with np.errstate(invalid="ignore", over="ignore"):
        e = dmu * band + _link_tol(family, mu)
        b_mean = e.sum(axis=0) / n + ROUND * np.abs(mean)
        if family == "logistic":
            q = P.expit(-t)
            eq = dmu * band + _link_tol(family, q)
            Ep, Eq = e.sum(axis=0) / n, eq.sum(axis=0) / n
            b_var = q.mean(axis=0) * Ep + mu.mean(axis=0) * Eq + Ep * Eq + ROUND * np.abs(var)
        else:
            b_var = (np.abs(dv + 2.0 * (mu - mu.mean(axis=0))) * e).sum(axis=0) / n + (e * e).sum(axis=0) / n + ROUND * np.abs(var)
    return np.where(np.isfinite(mean), b_mean, 0.0), np.where(np.isfinite(var), b_var, 0.0)


def assert_close(dev, ref, bound, what):
    """NaN, +inf and -inf by equality of their class, everything else within the bound; prints the worst error / bound ratio."""
    dev, ref, bound = np.asarray(dev, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert dev.shape == ref.shape == bound.shape, f"{what}: shapes {dev.shape}, {ref.shape}, {bound.shape}"
    for name, cls in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        assert np.array_equal(cls(dev), cls(ref)), f"{what}: {name} entries differ ({int(cls(dev).sum())} against {int(cls(ref).sum())})"
    fin = np.isfinite(ref)
    err = np.abs(dev[fin] - ref[fin])
    if err.size:
        ratio = err / bound[fin]
        print(f"{what}: max error {err.max():.3e}, largest error / bound {np.nanmax(ratio):.3f}")
        assert np.all(err <= bound[fin]), f"{what}: error {err[np.nanargmax(ratio)]:.3e} above the bound {bound[fin][np.nanargmax(ratio)]:.3e}"


def check(got, family, X, W, b, sigma, what):
    """Both outputs of the device (a dict of tensors or arrays) against the comparator."""
    mean, var = moments64(family, X, W, b, sigma)
    b_mean, b_var = bounds(family, X, W, b, sigma)
    assert_close(np.asarray(got["mean"]), mean, b_mean, what + " mean")
    assert_close(np.asarray(got["variance"]), var, b_var, what + " variance")
    return mean, var, b_mean, b_var


def link32(family, t32, dtype):
    """The link(s) at the float32 t through torch in `dtype`: a list of (n, rows) float64 arrays (logistic: sigmoid(t), sigmoid(-t))."""
    t = torch.as_tensor(np.asarray(t32, np.float32)).to(dtype)
    if family == "logistic":
        outs = [torch.sigmoid(t), torch.sigmoid(-t)]
    elif family == "linear":
        outs = [t]
    else:
        outs = [torch.exp(t)]
    return [o.to(torch.float64).numpy() for o in outs]


def float32_link_calibration(family):
    """The reference's OWN float32 error of the link on the sweep's inputs: float32 torch against float64 at the same float32 t, as
    the smallest passing rtol of the project's check.  Returns (rtol, (n, rows, d, intercept) of the worst case)."""
    worst, where = 0.0, None
    for fam, n, rows, d, intercept in sweep_cases():
        if fam != family:
            continue
        X, _, W, b = LR.inputs(family, n, rows, d, intercept)
        t32 = torch.tensor(W) @ torch.tensor(X).T
        if b is not None:
            t32 = t32 + torch.tensor(b).reshape(-1, 1)
        t32 = t32.numpy()
        for a, ref in zip(link32(family, t32, torch.float32), link32(family, t32, torch.float64)):
            r = max(R.smallest_passing_rtol(a[s], ref[s]) for s in range(n))      # draw by draw, as _link_tol takes its maximum
            if r > worst:
                worst, where = r, (n, rows, d, intercept)
    return worst, where


# ---------------------------------------------------------------- the special problems of tests/test_gpu_moments.py
def identical_draws(family, n=130, rows=129, d=33):
    """Every draw the same latent row: the between-draw term is exactly 0."""
    X, _, W, b = LR.inputs(family, n, rows, d, True, seed=17)
    return X, np.ascontiguousarray(np.repeat(W[:1], n, axis=0)), np.ascontiguousarray(np.repeat(b[:1], n))


def cancellation_problem(n=130, rows=70, d=3):
    """Linear regression whose intercept draws lie near 1e4 with a between-draw standard deviation of about 1e-2 (the weights are
    one row for every draw): mu^2 is 1e8, where float32 resolves 8, against a between-draw variance of 1e-4."""
    X, _, W, _ = LR.inputs("linear", n, rows, d, True, seed=23)
    W = np.ascontiguousarray(np.repeat(W[:1], n, axis=0))
    b = (1.0e4 + 1.0e-2 * np.random.default_rng(24).normal(size=n)).astype(np.float32)
    return X, W, b


def float32_sum_of_squares_variance(t, sigma):
    """What a float32 sum of mu^2 would give for the linear family (sigma^2 + E mu^2 - mean^2): the form the kernel must not use."""
    mu = np.asarray(t, np.float64).astype(np.float32)
    s1, s2 = np.zeros(mu.shape[1], np.float32), np.zeros(mu.shape[1], np.float32)
    for s in range(mu.shape[0]):
        s1 = s1 + mu[s]
        s2 = s2 + mu[s] * mu[s]
    n = np.float32(mu.shape[0])
    return (np.float32(sigma) ** 2 + (s2 / n - (s1 / n) * (s1 / n))).astype(np.float64)


def overflow_problem(all_draws):
    """Poisson, d = 4, rows = 70, n = 5 (the construction of tests/test_gpu_loglik.py).  One draw: w of draw 2 is scaled so that its
    nine largest t reach 95 and above; the other rows of X are turned away from that w so that every other element stays moderate.
    Every draw: the first 10 rows of X are set to 200 u / |u|^2, u the mean draw, so that t is about 200 under each draw.
    Returns (X, W, t)."""
    n, rows, d = 5, 70, 4
    X, _, W, _ = LR.inputs("poisson", n, rows, d, False, seed=5)
    X, W = X.copy(), W.copy()
    if all_draws:
        u = W.astype(np.float64).mean(axis=0)
        X[:10] = (200.0 * u / (u @ u)).astype(np.float32)
    else:
        w2 = W[2].astype(np.float64)
        t = X.astype(np.float64) @ w2
        c = 95.0 / np.sort(t)[-9]
        low = (t < np.sort(t)[-9]) & (c * np.abs(t) > 4.0)
        X[low] = (X[low].astype(np.float64) - ((1.0 - 4.0 / (c * np.abs(t[low]))) * t[low] / (w2 @ w2))[:, None] * w2).astype(np.float32)
        W[2] = (W[2] * np.float32(c)).astype(np.float32)
    t = LR.linear_predictor(X, W, None)
    assert not ((t > 80.0) & (t < 89.0)).any()      # nothing near float32's overflow point 88.72: no element can fall on the other side
    return X, W, t

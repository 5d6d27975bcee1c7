"""Comparator of d3p_amd.diagnostics for tests/test_guide_diag_host.py and tests/test_gpu_guide_diag.py: a float64 numpy restatement.

    totals(ll)[s]      = sum_r ll[s, r]                         from a GIVEN (n, rows) matrix (the device's own float32 matrix in the
                                                                GPU tests: only the reduction is judged), numpy's pairwise float64 sum
    totals_bound(ll)   = rows 2^-53 sum_r |ll[s, r]|            the float64 reordering bound: any order of rows - 1 additions of exact
                                                                float32 values errs by at most (rows - 1) 2^-53 sum |terms| to first order
    log_prior(w, b, ..) = sum of Normal(0, scale).log_prob      per draw, element by element
    log_q(theta, loc, sigma) = sum of Normal(loc, sigma).log_prob
    stats(lr)          = elbo (mean), elbo_se (sqrt(sample variance / n); one draw: NaN), log_evidence_is (logsumexp - log n),
                         ess ((sum r)^2 / sum r^2 with r = exp(lr - max))
    k_column(lr)       = float32(max lr - lr)                   what d3p_psis_loo is handed: its x = min - ll are the shifted ratios
    pareto_k(lr)       = NaN with a NaN ratio; +inf with a -inf ratio; -inf where every ratio is equal (n >= 2); otherwise
                         tests/psis_ref.psis_column(k_column(lr))["k"] (+inf for n <= 20: no tail of 5 draws)

The closed forms of the host test: LinearRegression without an intercept on an orthogonal design (X^T X diagonal, a_j its diagonal),
prior scale tau, noise sigma.  The posterior is the diagonal normal with precision P_j = a_j / sigma^2 + 1 / tau^2 and mean m_j =
(X^T y)_j / (sigma^2 P_j), and
    log p(y | X) = -rows log(2 pi sigma^2) / 2 - y.y / (2 sigma^2) + sum_j (P_j m_j^2 - log(tau^2 P_j)) / 2
With the guide Normal(m_j, c / sqrt(P_j)) and theta_s = m + c z_s / sqrt(P):   log r_s - log p(y | X) = D log c + (1 - c^2) / 2 sum_j z_sj^2.
The upper tail of r is that of exp((1 - c^2) chi^2_D / 2): a Pareto tail of index 1 - c^2 for c < 1, a bounded ratio for c > 1.
"""
import math

import numpy as np

from tests import psis_ref as PR

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
U53 = 2.0 ** -53


def totals(ll):
    return np.asarray(ll).astype(np.float64).sum(axis=1)


def totals_bound(ll):
    ll = np.asarray(ll).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ll.shape[1] * U53 * np.abs(ll).sum(axis=1)


def _normal_logpdf(x, loc, scale):
    x, loc, scale = (np.asarray(v, np.float64) for v in (x, loc, scale))
    z = (x - loc) / scale
    return -0.5 * z * z - np.log(scale) - HALF_LOG_2PI


def log_prior(w, b, prior_scale, intercept_prior_scale):
    """(n,) float64 from w (n, d) and b (n,) or None (the float32 latents)."""
    lp = _normal_logpdf(w, 0.0, prior_scale).sum(axis=1)
    if b is not None:
        lp = lp + _normal_logpdf(np.asarray(b).reshape(-1), 0.0, intercept_prior_scale)
    return lp


def prior_bound(w, b, prior_scale, intercept_prior_scale):
    """Float64 rounding of the O(D) prior sum, for two evaluations in different orders: each errs by at most (D + 4) 2^-53 sum of the
    |terms| (the quadratic terms and the constants: D additions in any order and up to four roundings inside a term), so they differ
    by at most twice that."""
    w = np.asarray(w, np.float64)
    D = w.shape[1] + (b is not None)
    mag = (0.5 * w * w / prior_scale ** 2).sum(axis=1) + w.shape[1] * (abs(math.log(prior_scale)) + HALF_LOG_2PI)
    if b is not None:
        bb = np.asarray(b, np.float64).reshape(-1)
        mag = mag + 0.5 * bb * bb / intercept_prior_scale ** 2 + abs(math.log(intercept_prior_scale)) + HALF_LOG_2PI
    return (D + 4) * 2.0 * U53 * mag


def guide_loc_sigma(kind, params, d, intercept):
    """(loc, sigma) float64 (D,) in latent column order [w | intercept]; kind: "auto", "diagonal" (site w) or "meanfield"."""
    p = {k: np.asarray(v, np.float32).reshape(-1).astype(np.float64) for k, v in params.items()}
    if kind == "auto":
        return p["auto_loc"], p["auto_scale"]
    if kind == "meanfield":
        return np.concatenate([p["w_loc"], p["intercept_loc"]]), np.exp(np.concatenate([p["w_std_log"], p["intercept_std_log"]]))
    loc = [k for k in p if k.endswith("_loc")][0]
    return p[loc], np.exp(p[loc[:-4] + "_std_log"])


def log_q(theta, loc, sigma):
    return _normal_logpdf(theta, loc, sigma).sum(axis=1)


def stats(lr):
    """{"elbo", "elbo_se", "log_evidence_is", "ess"} of the float64 log ratios."""
    lr = np.asarray(lr, np.float64)
    n = lr.size
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        elbo = lr.sum() / n
        dev = lr - elbo
        se = np.sqrt(np.float64((dev * dev).sum()) / np.float64(n - 1) / n) if n > 1 else np.nan
        mx = lr.max()
        if np.isnan(lr).any():
            lis = ess = np.nan
        elif mx == -np.inf:
            lis, ess = -np.inf, np.nan
        else:
            r = np.exp(lr - mx)
            lis = mx + np.log(r.sum()) - math.log(n)
            ess = r.sum() ** 2 / (r * r).sum()
    return {"elbo": elbo, "elbo_se": se, "log_evidence_is": lis, "ess": ess}


def k_column(lr):
    lr = np.asarray(lr, np.float64)
    with np.errstate(invalid="ignore"):
        return (lr.max() - lr).astype(np.float32)


def pareto_k(lr, with_cond=False):
    lr = np.asarray(lr, np.float64)
    k, cond = None, 1.0
    if np.isnan(lr).any():
        k = np.nan
    elif np.isneginf(lr).any():
        k = np.inf
    elif lr.size >= 2 and lr.max() == lr.min():
        k = -np.inf
    else:
        out = PR.psis_column(k_column(lr))
        k, cond = out["k"], out["cond"]
    return (k, cond) if with_cond else k


# ------------------------------------------------------------------------------------------------ the orthogonal-design linear case
ORTHO_SIGMA, ORTHO_TAU = 0.7, 1.3


def orthogonal_problem(D, rows, seed=0):
    """{"X" (rows, D) float32 with X^T X diagonal in exact arithmetic, "y" (rows,) float32, and float64 "a", "P", "m", "log_evidence"
    computed from the float32 values}.  The columns have disjoint supports (row r belongs to column r % D), so X^T X is EXACTLY
    diagonal for the float32 values too."""
    r = np.random.default_rng([seed, D, rows])
    X = np.zeros((rows, D), np.float32)
    X[np.arange(rows), np.arange(rows) % D] = r.normal(size=rows).astype(np.float32)
    w0 = r.normal(size=D)
    y = (X.astype(np.float64) @ w0 + ORTHO_SIGMA * r.normal(size=rows)).astype(np.float32)
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    a = (X64 * X64).sum(axis=0)
    P = a / ORTHO_SIGMA ** 2 + 1.0 / ORTHO_TAU ** 2
    m = (X64.T @ y64) / (ORTHO_SIGMA ** 2 * P)
    ev_terms = np.concatenate([[-0.5 * rows * math.log(2.0 * math.pi * ORTHO_SIGMA ** 2)], -0.5 * y64 * y64 / ORTHO_SIGMA ** 2,
                               0.5 * P * m * m, -0.5 * np.log(ORTHO_TAU ** 2 * P)])
    return {"X": X, "y": y, "a": a, "P": P, "m": m, "log_evidence": ev_terms.sum(), "ev_mag": np.abs(ev_terms).sum()}


def linear_ll64(X, y, theta, sigma):
    """(n, rows) float64 log N(y_r; x_r . theta_s, sigma) from float64 copies of the inputs."""
    t = np.asarray(theta, np.float64) @ np.asarray(X, np.float64).T
    return _normal_logpdf(np.asarray(y, np.float64)[None, :], t, sigma)


def scaled_posterior_guide(prob, c):
    """(loc, sigma) of the guide Normal(m, c / sqrt(P))."""
    return prob["m"], c / np.sqrt(prob["P"])


def ratio_offsets(z, c):
    """log r_s - log p(y | X) = D log c + (1 - c^2) / 2 sum_j z_sj^2 for the guide's standard normals z (n, D)."""
    z = np.asarray(z, np.float64)
    return z.shape[1] * math.log(c) + 0.5 * (1.0 - c * c) * (z * z).sum(axis=1)

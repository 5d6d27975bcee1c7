"""CPU comparator of d3p_amd.predictive for the linear and Poisson families (tests/predictive_ref.py is the one of d3p_amd.modelling
and supplies the key chain, the latent check and the vacuity guard used here).

With t64[s, r] = X[r] . w_s + b_s in float64 from the DEVICE's returned latents, E = (d + 2) 2^-23 (sum |x w| + |b|) the product band
of predictive_ref.logreg_band (the float32 product summed in any order, the +b and the product roundings), and the obs key k_s:

Linear.  obs = fl(t + fl(eps sigma)) with eps = normal(k_s, (rows,)).  Against ref = t64 + eps sigma (the oracle's eps):
    |obs - ref| <= E + (2e-6 |eps| + 2e-7) sigma + 2^-24 (2 |eps sigma| + |t64| + E)
  the product band, predictive_ref.assert_latent's eps term (the device's normal against the oracle's) times sigma, and the two
  roundings (2^-24 relative each: of the product, and of the sum whose terms are bounded by |t| + E + |eps sigma|).  The two-rounding
  rule itself is checked bit for bit apart from this bound: with the device's own eps (read through a call with w = 0, no
  intercept, sigma = 1, where obs = eps exactly) the result at exactly representable t is float32(t) + float32(eps) * float32(sigma).

Poisson.  `poisson_rule` restates the device's rule (d3p_amd/csrc/d3p_predict_glm.hip) in float64 numpy on the oracle's uniforms, which
are bit-equal to the device's.  The one quantity the two sides do not share exactly is lam = expf(t): the device's value lies in
    [exp(t64 - E) (1 - 2^-22), exp(t64 + E) (1 + 2^-22)]                          (expf within 2 ulp; E = 0 for exact t)
  An outcome is JUDGED only where the restatement, run at the interval's two ends and at exp(t64), takes the same branch, makes the
  same comparisons with the same results in every iteration and reaches the same k at all three, AND every lam-dependent comparison
  keeps a margin: with g(L) = (one side) - (the other),
      min over the three points of |g|  >  2 |g(hi) - g(lo)| + 1e-12 + 1e-11 mag
  Derivation: every g is smooth in L on an interval of relative width <= 1e-3 -- U_0 - F_k(L) (monotone: a Poisson CDF falls in its
  rate), v_r(L) - V (monotone: v_r rises with b = 0.931 + 2.53 sqrt(L)), the distance of h(L) = A sqrt(L) + L + C to the next integer
  (for the floor; h is convex or concave on the whole interval) and the two sides of the log-acceptance test (sums of log L, L and
  lgamma terms).  A monotone g stays on one side of 0 when its ends do; the factor 2 on the end-to-end variation and the midpoint cover
  a g that turns inside the interval, whose excursion beyond its ends is second order in the width.  1e-12 absolute and 1e-11 of the
  largest term's magnitude (mag: 1 for the CDF and v_r, 1 + |h| for the floor, L + |k log L| + lgamma(k + 1) + |log V| for the
  log-acceptance test) are the float64 slack: the device's exp / log / lgamma / sqrt and numpy's agree to a few ulp (2^-52 relative)
  of each term, and at most 64 terms are accumulated.
  Calibrated on the CPU (tests/test_predictive_glm_host.py) with the device replaced by a numpy float32 lam (float32 matmul, float32
  exp): every judged outcome of the GPU tests' inputs is equal, and the unjudged share stays under the cap.
  Judged outcomes must be EQUAL.  The share left unjudged is returned and capped by predictive_ref.assert_not_vacuous (0.05 of the
  outcomes plus two).  The equality tests therefore keep to inputs whose share is small: generic random cases with d <= 33 and t in
  [-3, 4], larger rates (up to 8192) with exactly representable t (`exact_rate_problem`); above that only the distribution is checked.
  Special values: NaN t -> -1; lam == 0 -> 0 (a lam below 1e-30, float32's denormals included, is 0 here: the inversion gives 0 too,
  F = exp(-L) = 1 > U); lam above float32's largest finite value -> 2147483647, as any draw above 2^31 - 1.
"""
import numpy as np
from scipy.special import gammaln

from .predictive_ref import site_key  # noqa: F401  (re-exported for the tests)

INT_MAX = 2147483647
F32_MAX = float(np.finfo(np.float32).max)
SLACK_ABS, SLACK_REL = 1e-12, 1e-11


# ------------------------------------------------------------------------------- the uniforms
class ObsUniforms:
    """(U_j, V_j) of iteration j for every draw: elements [r] and [rows + r] of uniform(fold_in(obs_key_s, j), (2 rows,))."""

    def __init__(self, O, okeys, rows):
        self.O, self.okeys, self.rows = O, [np.asarray(k, np.uint32) for k in okeys], rows
        self.cache = {}

    def __call__(self, j, draws=None):
        n = len(self.okeys)
        U, V, have = self.cache.get(j) or (np.full((n, self.rows), 0.5), np.full((n, self.rows), 0.5), np.zeros(n, bool))
        for s in range(n):
            if have[s] or (draws is not None and not draws[s]):
                continue
            u = self.O.tf_uniform(self.O.tf_fold_in(self.okeys[s], j), 2 * self.rows).astype(np.float64)
            U[s], V[s], have[s] = u[:self.rows], u[self.rows:], True
        self.cache[j] = (U, V, have)
        return U, V


class GridUniforms:
    """Independent uniforms on the 2^-23 grid of jax.random.uniform from a numpy generator (the distribution self-checks)."""

    def __init__(self, rng, shape):
        self.rng, self.shape = rng, shape

    def __call__(self, j, draws=None):
        return tuple(self.rng.integers(0, 2 ** 23, size=self.shape) / 2.0 ** 23 for _ in range(2))


# ------------------------------------------------------------------------------- the rule
def _stable(g, mag):
    """The margin condition of the module docstring for g of shape (P, ...) along axis 0 (lo, mid, hi; P = 1: the slack alone)."""
    fin = np.isfinite(g).all(axis=0)
    var = np.where(fin, np.abs(np.where(fin, g[-1] - g[0], 0.0)), 0.0)
    same = (g > 0).all(axis=0) | (g < 0).all(axis=0)
    return same & (np.abs(g).min(axis=0) > 2 * var + SLACK_ABS + SLACK_REL * np.max(mag, axis=0))


def poisson_rule(L, unif):
    """The device's Poisson rule in float64 at the rates L of shape (P, n, rows) (NaN where t is NaN; P points of the lam interval).
    Returns (k (P, n, rows) int64, signature (P, n, rows) of the branch and of every iteration's comparison results, stable (n, rows):
    every lam-dependent comparison kept its margin across the P points, iterations used)."""
    L = np.asarray(L, np.float64)
    P, n, rows = L.shape
    with np.errstate(all="ignore"):
        k = np.zeros(L.shape)
        sig = np.zeros(L.shape, np.uint64)
        stable = np.ones((n, rows), bool)
        nan, zero, inf = np.isnan(L), L == 0, np.isposinf(L)
        small = ~nan & ~zero & ~inf & (L < 10)
        big = ~nan & ~zero & ~inf & (L >= 10)
        k[nan], k[inf] = -1, INT_MAX
        for code, m in enumerate((nan, zero, inf, small, big)):
            sig[m] = code + 1
        iters = 0
        U0, V0 = unif(0, (small | big).any(axis=(0, 2)))
        # ---- lam < 10: inversion on U_0
        if small.any():
            p = np.exp(-L)
            F = p.copy()
            kk = np.zeros(L.shape)
            active = small.copy()
            for _ in range(64):
                g = U0[None] - F
                stable &= _stable(g, np.ones(L.shape)) | ~active.any(axis=0)
                active = active & (g >= 0)
                if not active.any():
                    break
                kk[active] += 1
                p[active] *= L[active] / kk[active]
                F[active] += p[active]
            k[small] = kk[small]
        # ---- lam >= 10: PTRS
        if big.any():
            s = np.sqrt(L)
            b = 0.931 + 2.53 * s
            a = -0.059 + 0.02483 * b
            lia = np.log(1.1239 + 1.1328 / (b - 3.4))
            vr = 0.9277 - 3.6224 / (b - 2.0)
            logL = np.log(L)
            active = big.copy()
            for j in range(64):
                if not active.any():
                    break
                iters = j + 1
                U, V = (U0, V0) if j == 0 else unif(j, active.any(axis=(0, 2)))
                u = (U - 0.5)[None]
                V = V[None]
                us = 0.5 - np.abs(u)
                h = (2.0 * a / us + b) * u + L + 0.43
                kk = np.floor(h)
                c1 = (us >= 0.07) & (V <= vr)
                c2 = (kk < 0) | ((us < 0.013) & (V > us))
                lgam = gammaln(kk + 1.0)
                lhs = np.log(V) + lia - np.log(a / (us * us) + b)
                rhs = -L + kk * logL - lgam
                c3 = lhs <= rhs
                code = np.where(c1, 1, np.where(c2, 2, np.where(c3, 3, 4))).astype(np.uint64)
                sig[active] = sig[active] * np.uint64(8) + code[active]
                reached = active.any(axis=0)
                frac = h - kk
                hfin = np.isfinite(h).all(axis=0)
                floor_ok = np.where(hfin, _stable(np.minimum(frac, 1.0 - frac), 1.0 + np.abs(np.where(np.isfinite(h), h, 0.0)))
                                    & (kk == kk[0]).all(axis=0), (h == h[0]).all(axis=0))
                stable &= ~reached | floor_ok
                stable &= ~(reached & (us[0] >= 0.07)) | _stable(vr - V, np.ones(L.shape))
                need3 = (active & ~c1 & ~c2).any(axis=0)
                stable &= ~need3 | _stable(rhs - lhs, np.abs(L) + np.abs(kk * logL) + np.abs(lgam) + np.abs(np.log(V)))
                acc = active & (c1 | (~c2 & c3))
                k[acc] = kk[acc]
                active &= ~acc
            left = active.any(axis=0)          # 64 rejections: floor(L), judged only if it does not move
            fl = np.floor(L)
            k[active] = fl[active]
            stable &= ~left | (fl == fl[0]).all(axis=0)
        k = np.where(k > INT_MAX, INT_MAX, k)
        return k.astype(np.int64), sig, stable, iters


def lam_interval(t64, E):
    """(3, ...) float64: the device's lam = expf(t) lies between the first and the last; the middle is exp(t64).  Values a float32 does
    not hold are mapped to what expf returns: +inf above its largest finite value, 0 below 1e-30 (module docstring)."""
    with np.errstate(all="ignore"):
        pts = np.stack([np.exp(t64 - E) * (1 - 2.0 ** -22), np.exp(t64), np.exp(t64 + E) * (1 + 2.0 ** -22)])
    pts = np.where(pts > F32_MAX, np.inf, pts)
    return np.where(pts < 1e-30, 0.0, pts)


def judge_poisson(t64, E, unif):
    """(expected k (n, rows), judged (n, rows), iterations) of the restatement over the lam interval."""
    k, sig, stable, iters = poisson_rule(lam_interval(t64, E), unif)
    judged = stable & (k == k[0]).all(axis=0) & (sig == sig[0]).all(axis=0)
    return k[1], judged, iters


# ------------------------------------------------------------------------------- checks of device results
def linear_predictor(X, w, b, d):
    """(t64 (n, rows), E (n, rows)) from the device's latents w (n, d), b (n,) or None."""
    X64, w64 = X.astype(np.float64), np.asarray(w, np.float64).reshape(-1, d)
    b64 = np.zeros(len(w64)) if b is None else np.asarray(b, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        t = w64 @ X64.T + b64[:, None]
        E = (d + 2) * 2.0 ** -23 * (np.abs(w64) @ np.abs(X64).T + np.abs(b64)[:, None])
    return t, E


def check_linear(O, obs, X, w, b, sigma, okeys, d, what):
    t, E = linear_predictor(X, w, b, d)
    rows = X.shape[0]
    eps = np.stack([O.tf_normal(k, rows) for k in okeys]).astype(np.float64)
    ref = t + eps * sigma
    tol = E + (2e-6 * np.abs(eps) + 2e-7) * sigma + 2.0 ** -24 * (2 * np.abs(eps * sigma) + np.abs(t) + E) + 1e-30
    err = np.abs(np.asarray(obs, np.float64) - ref)
    assert obs.shape == ref.shape and np.all(err <= tol), f"{what}: max err {err.max()} (tol at argmax {tol.ravel()[err.argmax()]})"


def check_poisson(O, obs, X, w, b, okeys, d, what, exact=False):
    """Every judged outcome equal; returns the unjudged share (for predictive_ref.assert_not_vacuous)."""
    t, E = linear_predictor(X, w, b, d)
    exp, judged, _ = judge_poisson(t, np.zeros_like(E) if exact else E, ObsUniforms(O, okeys, X.shape[0]))
    obs = np.asarray(obs)
    assert obs.shape == exp.shape and obs.dtype == np.int32
    bad = judged & (obs != exp)
    assert not bad.any(), (f"{what}: {int(bad.sum())} judged outcomes differ (first at {np.argwhere(bad)[0]}: device "
                           f"{obs[tuple(np.argwhere(bad)[0])]}, expected {exp[tuple(np.argwhere(bad)[0])]})")
    assert np.all(obs >= -1)
    return float((~judged).mean())


def simulated_device_poisson(O, X, w, b, okeys, d):
    """What a device with a numpy float32 lam returns: float32 matmul, float32 exp, then the rule at that single lam."""
    t32 = np.asarray(w, np.float32).reshape(-1, d) @ X.astype(np.float32).T
    if b is not None:
        t32 = t32 + np.asarray(b, np.float32).reshape(-1, 1)
    with np.errstate(all="ignore"):
        lam = np.exp(t32.astype(np.float32)).astype(np.float64)
    lam = np.where(np.isnan(t32), np.nan, lam)
    return poisson_rule(lam[None], ObsUniforms(O, okeys, X.shape[0]))[0][0].astype(np.int32)


# ------------------------------------------------------------------------------- inputs
def generic_problem(d, rows, n, intercept, seed):
    """X, guide parameters (AutoDiagonalNormal) of a random case whose t stays within [-3, 4]: |x| <= 1, |loc| sums to 2.5 at most,
    draws within a few hundredths of loc."""
    rng = np.random.default_rng(seed)
    D = d + int(intercept)
    X = rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)
    loc = rng.uniform(-1, 1, size=D)
    loc = (loc * (2.5 / np.abs(loc).sum())).astype(np.float32)
    if intercept:
        loc[d] = np.float32(0.5)
    scale = np.full(D, 0.02 / D, np.float32)
    return X, {"auto_loc": loc, "auto_scale": scale}


# (d, rows, n, intercept): d on both sides of a K slice, rows and draws on both sides of a tile, each value with and without an
# intercept somewhere; the last covers several tiles both ways
TILE_EDGES = [(1, 129, 128, True), (31, 127, 129, False), (32, 128, 127, True), (33, 1, 128, False), (33, 129, 1, True), (1, 1, 1, False),
              (32, 127, 129, False), (31, 128, 127, True), (33, 257, 257, True)]


def edge_seed(d, rows, n, intercept):
    return 1000003 * d + 1009 * rows + 7 * n + int(intercept)


def oracle_draws(O, key_words, n, d, intercept, params, rows, posterior=True, subst=None):
    """(w (n, d) float32, b (n,) float32 or None, obs keys) of the multi form rebuilt on the CPU (predictive_ref.logreg_expect on the
    LogisticRegression of the same layout, AutoDiagonalNormal or the prior with `subst`), the latents rounded as the device does."""
    from d3p_amd.models import AutoDiagonalNormal, LogisticRegression

    from .predictive_ref import logreg_expect
    model = LogisticRegression(d, intercept=intercept)
    X = np.zeros((rows, d), np.float32)
    exp, okeys = logreg_expect(O, key_words, n, True, model, AutoDiagonalNormal(model) if posterior else None, params, X, subst)
    if posterior:
        lat = np.stack([(loc + (eps * sc.astype(np.float32)).astype(np.float32)).astype(np.float32) for loc, eps, sc in exp["_auto_latent"]])
        return lat[:, :d], (lat[:, d] if intercept else None), okeys
    w = np.stack([np.asarray(v, np.float32) for v in exp["w"]])
    b = np.stack([np.asarray(v, np.float32) for v in exp["intercept"]]).reshape(n) if intercept else None
    return w, b, okeys


EXACT_RATES = (2.0 ** -4, 1.0, 9.99, 10.01, 64.0, 1024.0, 8192.0)


def exact_rate_problem(rates=EXACT_RATES, pairs=3, copies=3, seed=5):
    """(X, w, t) with exactly representable linear predictors: row i carries rate i // copies.  w = [c_0 .. c_{R-1} | pairs of equal
    dyadic weights], c_i = round(log(rate_i) 2^16) / 2^16; a row selects its c_i with a 1 and multiplies each pair by (+x, -x), x in
    {0, 1/2, 1}: every product is a multiple of 2^-16 below 2^4 in magnitude and the pairs cancel, so the float32 sum is c_i in any
    order (20 bits), and dropping or doubling a column is seen."""
    rng = np.random.default_rng(seed)
    R = len(rates)
    c = np.round(np.log(np.asarray(rates)) * 2.0 ** 16) / 2.0 ** 16
    pw = rng.integers(1, 9, size=pairs) * rng.choice([-1, 1], size=pairs) / 64.0
    w = np.concatenate([c, np.repeat(pw, 2)]).astype(np.float32)
    X = np.zeros((R * copies, R + 2 * pairs), np.float32)
    for i in range(R * copies):
        X[i, i // copies] = 1.0
        x = rng.integers(0, 3, size=pairs) / 2.0
        X[i, R::2], X[i, R + 1::2] = x, -x
    t = np.repeat(c, copies)
    assert np.array_equal(w[:R].astype(np.float64), c) and np.array_equal(X.astype(np.float64) @ w.astype(np.float64), t)
    return X, w, t


# ------------------------------------------------------------------------------- distribution bounds
def poisson_moment_bounds(lam, n):
    """(bound on |mean - lam|, bound on |s^2 - lam|) at 5 standard errors: Var(mean) = lam / n; Var(s^2) = (mu4 - sigma^4 (n - 3) /
    (n - 1)) / n with mu4 = lam + 3 lam^2, at most (lam + 2 lam^2 + 2 lam^2 / (n - 1)) / n."""
    return 5 * np.sqrt(lam / n), 5 * np.sqrt((lam + 2 * lam ** 2 + 2 * lam ** 2 / (n - 1)) / n)


def normal_moment_bounds(n):
    """The same for a standard normal: Var(mean) = 1 / n, Var(s^2) = 2 / (n - 1)."""
    return 5 / np.sqrt(n), 5 * np.sqrt(2.0 / (n - 1))

"""Comparator of d3p_amd.criteria (WAIC) for tests/test_waic_host.py and tests/test_gpu_waic.py: float64 numpy on top of
tests/loglik_ref.py (regression families) and tests/mixture_density_ref.py (mixture model), which supply ll64, lppd64 and the
per-element error bound of ll.

    p_waic[r]    = sum_s (ll[s, r] - mean_s ll[s, r])^2 / (n - ddof)          pwaic64; a row with a -inf draw: +inf
    elpd_waic[r] = lppd[r] - p_waic[r]

Bound of p_waic per row, derived from the per-element bound of ll.  Let beta_r = max_s bound[s, r] (regression: LR.ll_bound; mixture:
max(ll_hi - ll, ll - ll_lo) of MR.intervals).  Perturbing every x_s = ll[s, r] by at most beta moves the mean by at most beta and
every centred value x_s - mean by at most 2 beta, so a square (x_s - mean)^2 moves by at most 4 beta |x_s - mean| + 4 beta^2 and

    bound_v[r] = (4 beta_r sum_s |x_s - mean| + 4 n beta_r^2) / (n - ddof) + 2^-22 v64[r].

The last term covers the kernel's float64 accumulation (n additions of relative error 2^-53 each: far below 2^-24 for any n that
fits a launch) and the one rounding to float32 (2^-24 relative), with a factor 4 of margin as the other comparators take it.
The elpd bound is lppd's bound + bound_v.  The bound is absolute: where the variance itself is tiny (the mixture's soft inputs at
k = 16, d = 256, n = 2: 2e-5) it is wider than the variance, and still a bound of 4e-5 on a quantity that is summed with lppd.

Calibration (tests/test_waic_host.py recomputes it): a float32 restatement of ll -- float32 product and LR.ll_of_t(dtype=float32);
MR.a32_restated and MR.ll32_restated -- fed to a float64 variance stays inside bound_v on every case with n >= 2 at both ddof:
largest error / bound 0.0097 over LR.sweep_cases(), 0.049 over MR.CASES x MR.KINDS.

Totals.  The device sums the (rows,) float32 pointwise arrays in float64 with torch; numpy's float64 sum of the same arrays may
order the additions differently, each of at most rows - 1 additions rounding by at most 2^-53 of a partial sum that is at most
sum |x|: `sum_bound` = rows 2^-52 sum |x|, for se through the same bound on its variance's terms.
"""
import numpy as np
import torch

from tests import loglik_ref as LR
from tests import mixture_density_ref as MR

ROUNDING = 2.0 ** -22


def pwaic64(ll, ddof):
    """(rows,) float64 from ll (n, rows): the variance over the draws with divisor n - ddof; +inf where a draw is -inf."""
    ll = np.asarray(ll, np.float64)
    n = ll.shape[0]
    assert n > ddof
    bad = np.isneginf(ll).any(axis=0)
    safe = np.where(bad[None, :], 0.0, ll)
    v = ((safe - safe.mean(axis=0)) ** 2).sum(axis=0) / (n - ddof)
    return np.where(bad, np.inf, v)


def bound_v(ll, beta, ddof, v=None):
    """(rows,) float64 (file docstring); rows with a -inf draw get 0 (they are compared by equality)."""
    ll = np.asarray(ll, np.float64)
    n = ll.shape[0]
    bad = np.isneginf(ll).any(axis=0)
    safe = np.where(bad[None, :], 0.0, ll)
    v = pwaic64(ll, ddof) if v is None else v
    spread = np.abs(safe - safe.mean(axis=0)).sum(axis=0)
    b = (4.0 * beta * spread + 4.0 * n * beta ** 2) / (n - ddof) + ROUNDING * np.where(bad, 0.0, v)
    return np.where(bad, 0.0, b)


def sum_bound(x):
    x = np.asarray(x, np.float64)
    return x.size * 2.0 ** -52 * np.abs(x).sum()


def totals64(elpd, pw):
    """numpy float64 totals of the device's own pointwise arrays: (elpd_waic, p_waic, se^2, bound of se^2)."""
    e, p = np.asarray(elpd, np.float64), np.asarray(pw, np.float64)
    rows = e.size
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = rows * (e - e.mean()) ** 2 / (rows - 1)
    return e.sum(), p.sum(), terms.sum(), sum_bound(terms)


def check_totals(res, what):
    """The WAICResult's totals against numpy float64 of its own pointwise arrays."""
    e, p = (res.pointwise[name].detach().cpu().numpy() for name in ("elpd_waic", "p_waic"))
    assert np.array_equal(e, (res.pointwise["lppd"] - res.pointwise["p_waic"]).detach().cpu().numpy(), equal_nan=True)
    for t in (res.elpd_waic, res.p_waic, res.waic, res.se):
        assert t.dtype == torch.float64 and t.dim() == 0 and t.device == res.pointwise["lppd"].device
    es, ps, var, var_bound = totals64(e, p)
    got_e, got_p, got_w, got_se = (float(t) for t in (res.elpd_waic, res.p_waic, res.waic, res.se))
    print(f"{what}: elpd_waic {got_e:.6f} (p_waic {got_p:.6f}, se {got_se:.6f}); |elpd - numpy| {abs(got_e - es):.3e} of {sum_bound(e):.3e}")
    assert abs(got_e - es) <= sum_bound(e) and abs(got_p - ps) <= sum_bound(p), what
    assert got_w == -2.0 * got_e, what
    if e.size == 1:
        assert np.isnan(got_se), what
    else:
        assert abs(got_se ** 2 - var) <= var_bound + 2.0 ** -51 * var, what   # (+ the square root's and the square's own roundings)
    assert res.n_rows == e.size


# ------------------------------------------------------------------------------------------------ regression families
_reg = {}


def regression_reference(family, n, rows, d, intercept, ddof):
    """Inputs, float64 reference and bounds of one sweep case; computed once and shared (read-only)."""
    key = (family, n, rows, d, intercept, ddof)
    if key not in _reg:
        X, y, W, b = LR.inputs(family, n, rows, d, intercept)
        sigma = LR.SIGMA[family]
        ll = LR.ll64(family, X, y, W, b, sigma)
        assert np.isfinite(ll).all()
        bound = LR.ll_bound(family, X, y, W, b, sigma, ll)
        lppd = LR.lppd64(ll)
        v = pwaic64(ll, ddof)
        bv = bound_v(ll, bound.max(axis=0), ddof, v)
        ref = {"X": X, "y": y, "W": W, "ll": ll, "lppd": lppd, "lppd_bound": LR.lppd_bound(ll, bound, lppd), "v": v, "bound_v": bv}
        if b is not None:
            ref["b"] = b
        ref["elpd"] = lppd - v
        ref["elpd_bound"] = ref["lppd_bound"] + bv
        for a in ref.values():
            a.setflags(write=False)
        _reg[key] = ref
    return _reg[key]


def regression_ll32(family, X, y, W, b):
    """ll with float32's error in it, as float64: the product in float32 (torch on the CPU) and the link through float32 torch."""
    t32 = torch.tensor(W) @ torch.tensor(X).T
    if b is not None:
        t32 = t32 + torch.tensor(b).reshape(-1, 1)
    return LR.ll_of_t(family, t32.numpy(), y, LR.SIGMA[family], torch.float32)


# ------------------------------------------------------------------------------------------------ mixture model
MIXTURE_CASES = [c for c in dict.fromkeys(MR.CASES) if c[3] >= 2]


def mixture_reference(kind, k, d, rows, n, ddof):
    """MR.reference's arrays plus {"beta", "v", "bound_v", "lppd_bound", "elpd", "elpd_bound"}."""
    ref = MR.reference(kind, k, d, rows, n)
    ll = ref["ll"]
    beta = np.maximum(ref["ll_hi"] - ll, ll - ref["ll_lo"]).max(axis=0)
    v = pwaic64(ll, ddof)
    bv = bound_v(ll, beta, ddof, v)
    lb = np.maximum(ref["lppd_hi"] - ref["lppd"], ref["lppd"] - ref["lppd_lo"])
    return dict(ref, beta=beta, v=v, bound_v=bv, lppd_bound=lb, elpd=ref["lppd"] - v, elpd_bound=lb + bv)


def mixture_ll32(ref):
    return MR.ll32_restated(MR.a32_restated(ref["obs"], ref["pis"], ref["mus"], ref["sigs"]))[0].astype(np.float64)


# ------------------------------------------------------------------------------------------------ comparison
def assert_within(dev, ref, bound, what):
    """+-inf by equality, everything else within the bound, NaN never; prints the worst error / bound ratio."""
    dev, ref, bound = np.asarray(dev, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert dev.shape == ref.shape, f"{what}: shape {dev.shape} != {ref.shape}"
    assert not np.isnan(dev).any(), f"{what}: NaN at {np.argwhere(np.isnan(dev))[0]}"
    assert not np.isnan(ref).any(), f"{what}: the comparator has a NaN"
    inf = np.isinf(ref)
    assert np.array_equal(dev[inf], ref[inf]) and np.isfinite(dev[~inf]).all(), f"{what}: the infinite entries differ"
    err = np.abs(dev[~inf] - ref[~inf])
    if err.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bound[~inf])
        print(f"{what}: max error {err.max():.3e}, largest error / bound {ratio.max():.4f}")
        assert np.all(err <= bound[~inf]), f"{what}: error {err[ratio.argmax()]:.3e} above the bound {bound[~inf][ratio.argmax()]:.3e}"
        return float(ratio.max())
    return 0.0


# ------------------------------------------------------------------------------------------------ Poisson overflow
def overflow_problem(all_draws):
    """The constructions of tests/test_gpu_loglik.py's two overflow tests, restated: d = 4, rows = 70, n = 5, no intercept.  One draw:
    w of draw 2 is scaled so that its nine largest t reach 95 and above, and the other rows of X are turned away from that w so that
    every other element stays moderate.  Every draw: the first 10 rows of X are set to 200 u / |u|^2, u the mean draw, so that t is
    about 200 under each draw.  Nothing lies near float32's overflow point 88.72, so no element can fall on the other side."""
    n, rows, d = 5, 70, 4
    X, y, W, b = LR.inputs("poisson", n, rows, d, False, seed=5)
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
    assert not ((t > 80.0) & (t < 89.0)).any()      # nothing near 88.72
    return n, rows, d, X, y, W, t

"""float64 reference of the VAE's log importance weights and of the column statistics (d3p_amd.vae_density), with the bounds the GPU
tests hold the device to.  Built on tests/predictive_ref.py's float64 network passes and their propagated float32 error bounds.

log importance weights (`log_weights_ref`)
------------------------------------------
Evaluated at the DEVICE's z (float32, taken as exact), with a = the float64 decoder output at z and (zl, zs) the float64 encoder
heads; predictive_ref's `vae_decode_bound` / `vae_encode_bound` give Eo, El, Es with |a_dev - a| <= Eo, |zl_dev - zl| <= El,
|zs_dev - zs| <= Es elementwise.  c = log(2 pi) / 2.

    log_px = sum_c x a - softplus(a)        d/da = x - sigmoid(a), |.| <= 1 for x in [0, 1]:   sum_c |x - sigmoid(a)| Eo_c <= sum_c Eo_c
                                            the float32 evaluation of a term (the product, the softplus, the difference):
                                            2^-22 (|x a| + softplus(a)) per term
    log_pz = sum_j -z^2 / 2 - c             no network input.  Two float32 roundings per term (the square, the difference; the halving
                                            is exact): 2^-24 z^2 / 2 + 2^-24 |z^2 / 2 + c| <= 2^-23 (z^2 / 2 + c) per term
    log_qz = sum_j -u^2 / 2 - zs - c,  u = (z - zl) / sigma, sigma = exp(zs)
                                            d/dzl = u / sigma and d/dzs = u^2 - 1; the float32 difference z - zl adds 2^-23 |z - zl| to
                                            the error of zl:    sum_j |u| / sigma (El_j + 2^-23 |z - zl|) + |u^2 - 1| Es_j
    each output is rounded to float32 once: 2^-24 (|value| + its bound)
    log_w  = log_px + log_pz - log_qz       bound = the log_px bound + the log_qz bound + one final rounding

The float64 sums of the float32 terms (at most 784 + 2 x 50 of them, relative error below 900 x 2^-53) are far below every term above
and are not counted.  Every element of every output must sit within its bound.

column statistics (`col_stats_ref`)
-----------------------------------
Brute force per column on the float32 matrix: math.fsum (exact sums, one rounding) and math.exp / math.log (glibc: below 1 ulp).  The
device adds n float64 values one by one (chunks of a quarter of the draws, merged pairwise) and calls OCML's exp and log, documented at
1 ulp each in float64.  With u = 2^-53 (1 ulp <= 2 u relative) and v - max exact in float64 (both float32):

    mean   the device's sum: (n - 1) u sum|v|; the divisions: u each      b_mean = n u sum|v| / n + 2 u |mean|
    var    a term (v - mean)^2 carries 3 u, the sum n u, on either side; the device's mean differs from the reference's by d <= b_mean:
           sum (v - m')^2 = sum (v - m)^2 + 2 (m - m') sum (v - m) + n d^2
                                                                          b_var = (2 (n + 3) u Q + 2 d sum|v - mean| + n d^2) / (n - 1) + 2 u var
    lse    r = exp(v - max): 2 u per side, the device's sum n u: R1 within (n + 5) u relative; log: 2 u |log R1| per side; the addition of
           max and the subtraction of log n: u each of the magnitudes
                                                                          b_lse = (n + 5) u + 4 u (|log R1| + log n + |max| + |lse|)
    ess    R1^2 / R2: 2 (n + 5) u + (n + 10) u + 2 u                      b_ess = (3 n + 24) u ess
"""
import math

import numpy as np

from tests import predictive_ref as P

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
U = 2.0 ** -53


def log_weights_ref(z, X, layers_dec, layers_enc, heads):
    """z: (n, B, Z) float32 (the device's), X: (B, D) float32.  Returns {name: (value, bound)} for log_w, log_px, log_pz, log_qz,
    each (n, B) float64."""
    n, B, Z = z.shape
    x = X.astype(np.float64)[None]
    zl, El, zs, Es = P.vae_encode_bound(X, layers_enc, heads)
    a, Eo = P.vae_decode_bound(z.reshape(n * B, Z), layers_dec)
    a, Eo = a.reshape(n, B, -1), Eo.reshape(n, B, -1)
    sp = P.softplus(a)
    px = (x * a - sp).sum(-1)
    b_px = (Eo + 2.0 ** -22 * (np.abs(x * a) + sp)).sum(-1)
    z64 = z.astype(np.float64)
    pz = (-0.5 * z64 * z64 - HALF_LOG_2PI).sum(-1)
    b_pz = (2.0 ** -23 * (0.5 * z64 * z64 + HALF_LOG_2PI)).sum(-1)
    sigma = np.exp(zs)[None]
    d = z64 - zl[None]
    u = d / sigma
    qz = (-0.5 * u * u - zs[None] - HALF_LOG_2PI).sum(-1)
    b_qz = (np.abs(u) / sigma * (El[None] + 2.0 ** -23 * np.abs(d)) + np.abs(u * u - 1) * Es[None]).sum(-1)
    lw = px + pz - qz
    b_lw = b_px + b_qz

    def rounded(v, b):
        return v, b + 2.0 ** -24 * (np.abs(v) + b)

    return {"log_w": rounded(lw, b_lw), "log_px": rounded(px, b_px), "log_pz": rounded(pz, b_pz), "log_qz": rounded(qz, b_qz)}


def assert_within(dev, ref, bound, what):
    """Every element within its bound; returns the largest error / bound ratio."""
    dev = np.asarray(dev, np.float64)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    assert np.all(np.isfinite(dev)), f"{what}: non-finite values"
    err = np.abs(dev - ref)
    ratio = err / bound
    k = int(np.argmax(ratio))
    print(f"{what}: largest error / bound = {ratio.ravel()[k]:.3g} (error {err.ravel()[k]:.3g}, bound {bound.ravel()[k]:.3g})")
    assert np.all(err <= bound), f"{what}: error {err.ravel()[k]} above its bound {bound.ravel()[k]} at {np.unravel_index(k, err.shape)}"
    return float(ratio.ravel()[k])


def col_stats_ref(m):
    """Brute force over the float32 matrix m (draws, cols): ({mean, var, lse, ess}: (cols,) float64, their bounds likewise).  Special
    columns: a NaN makes all four NaN; every draw -inf: mean = lse = -inf, var = ess = NaN."""
    m = np.asarray(m, np.float32)
    n, cols = m.shape
    out = {k: np.empty(cols) for k in ("mean", "var", "lse", "ess")}
    bnd = {k: np.zeros(cols) for k in out}
    for c in range(cols):
        v = [float(t) for t in m[:, c]]
        if any(math.isnan(t) for t in v):
            for k in out:
                out[k][c] = math.nan
            continue
        mx = max(v)
        if mx == -math.inf:
            out["mean"][c] = out["lse"][c] = -math.inf
            out["var"][c] = out["ess"][c] = math.nan
            continue
        mean = math.fsum(v) / n
        sabs = math.fsum(abs(t) for t in v)
        b_mean = n * U * sabs / n + 2 * U * abs(mean)
        Q = math.fsum((t - mean) ** 2 for t in v)
        var = Q / (n - 1) if n > 1 else math.nan
        b_var = ((2 * (n + 3) * U * Q + 2 * b_mean * math.fsum(abs(t - mean) for t in v) + n * b_mean ** 2) / (n - 1) + 2 * U * var) if n > 1 else 0.0
        r = [math.exp(t - mx) for t in v]
        R1, R2 = math.fsum(r), math.fsum(t * t for t in r)
        lse = mx + math.log(R1) - math.log(n)
        ess = R1 * R1 / R2
        out["mean"][c], out["var"][c], out["lse"][c], out["ess"][c] = mean, var, lse, ess
        bnd["mean"][c], bnd["var"][c] = b_mean, b_var
        bnd["lse"][c] = (n + 5) * U + 4 * U * (abs(math.log(R1)) + math.log(n) + abs(mx) + abs(lse))
        bnd["ess"][c] = (3 * n + 24) * U * ess
    return out, bnd


def assert_col_stats(dev, m, what):
    """dev: {mean, var, lse, ess} float64 (cols,) from the device for the float32 matrix m; returns the largest error / bound ratio
    (columns whose reference is not finite must match it exactly: NaN for NaN, -inf for -inf)."""
    ref, bnd = col_stats_ref(m)
    worst = 0.0
    for k in ("mean", "var", "lse", "ess"):
        d, r, b = np.asarray(dev[k], np.float64), ref[k], bnd[k]
        fin = np.isfinite(r)
        assert np.array_equal(np.isnan(d), np.isnan(r)), f"{what} {k}: NaN pattern differs"
        assert np.array_equal(d[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), f"{what} {k}: infinite values differ"
        if fin.any():
            err = np.abs(d[fin] - r[fin])
            ratio = np.where(err == 0, 0.0, err / np.maximum(b[fin], 1e-300))
            print(f"{what} {k}: largest error / bound = {ratio.max():.3g}")
            assert np.all(err <= b[fin]), f"{what} {k}: error {err.max()} above its bound"
            worst = max(worst, float(ratio.max()))
    return worst


def density_from_logw(logw):
    """The per-image quantities of held_out_density from a float32 (n, B) matrix: (values, bounds) of col_stats_ref under the names
    elbo, elbo_draw_var, log_px_is, ess."""
    ref, bnd = col_stats_ref(logw)
    names = {"mean": "elbo", "var": "elbo_draw_var", "lse": "log_px_is", "ess": "ess"}
    return {names[k]: v for k, v in ref.items()}, {names[k]: v for k, v in bnd.items()}

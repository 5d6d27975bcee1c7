"""Reference of d3p_kernel_sums and d3p_amd.mmd in plain numpy float64, and the bound d3p_mmd.hip's header derives.

t is formed in float32 exactly as the rule says; q by DIFFERENCES in float64, not by the Gram form; k_b = exp(-ln 2 gamma0 2^b q); sums
with math.fsum.  gram_f32 is the rule itself in float32 numpy (any order): what the bound has to hold for."""
import math

import numpy as np

U32, U64, LN2 = 2.0 ** -24, 2.0 ** -53, math.log(2.0)


def gamma(m, u=U32):
    return m * u / (1.0 - m * u)


def transform(x, shift, scale):
    """t = fl32(fl32(x - shift) * scale) of an (n, d) float32 or int32 table; a None skips its step."""
    t = x.astype(np.float32)
    if shift is not None:
        t = (t - shift.astype(np.float32)).astype(np.float32)
    if scale is not None:
        t = (t * scale.astype(np.float32)).astype(np.float32)
    return t


def kernel_sums(a, b, gamma0, n_b, shift=None, scale=None, exclude=False, roundings=40):
    """(out, bound): (B, na) float64 each, the sums of k_b over the admissible j and the header's bound on them, `roundings` float64
    additions on a row (d3p_kernel_sums_roundings)."""
    ta, tb = transform(a, shift, scale).astype(np.float64), transform(b, shift, scale).astype(np.float64)
    na, nb, d = ta.shape[0], tb.shape[0], ta.shape[1]
    g0 = float(np.float32(gamma0))
    dp = 32 * -(-d // 32)
    rb, absb = (tb * tb).sum(axis=1), np.abs(tb)
    out, bound = np.zeros((n_b, na)), np.zeros((n_b, na))
    np.seterr(over="ignore", invalid="ignore")     # (an uncentred table without a shift: the bound is infinite, and says so)
    for i in range(na):
        q = ((ta[i] - tb) ** 2).sum(axis=1)
        ok = np.arange(nb) != i if exclude else np.ones(nb, bool)
        norms = float((ta[i] * ta[i]).sum()) + rb
        dq = gamma(dp + 2) * norms + 2.0 * gamma(dp) * (absb @ np.abs(ta[i]))
        dq = dq + U32 * (q + dq) + (2 * dp + 4) * 2.0 ** -126
        err = np.expm1(LN2 * g0 * (dq + U32 * (q + dq))) * (1.0 + 2.0 * U32) + 2.0 * U32      # E_0
        for r in range(n_b):
            k = np.exp(-LN2 * g0 * 2.0 ** r * q)[ok]
            out[r, i] = math.fsum(k)
            each = err[ok] * k + 2.0 ** -125
            bound[r, i] = (1.0 + gamma(63)) * math.fsum(each) + (gamma(63) + gamma(roundings, U64)) * math.fsum(k + each)
            err = (2.0 * err + err * err) * (1.0 + U32) + U32                                 # E_(r+1) = (1 + E_r)^2 (1 + u) - 1
    return out, bound


def gram_f32(a, b, gamma0, n_b, shift=None, scale=None):
    """The rule in float32 numpy, sums in float64: (B, na)."""
    ta, tb = transform(a, shift, scale), transform(b, shift, scale)
    ra, rb = (ta * ta).sum(axis=1, dtype=np.float32), (tb * tb).sum(axis=1, dtype=np.float32)
    q = np.maximum(np.float32(0), (ra[:, None] + rb[None, :]) - np.float32(2) * (ta @ tb.T))
    k = np.exp2(-np.float32(gamma0) * q).astype(np.float32)
    rows = []
    for _ in range(n_b):
        rows.append(k.astype(np.float64).sum(axis=1))
        k = (k * k).astype(np.float32)
    return np.stack(rows)


def mmd(x, y, sigma2):
    """(mmd2, mmd2_unbiased, witness_x, witness_y) of float64 (n, d) points under k = exp(-|u - v|^2 / (2 sigma2)), by the definitions."""
    def gram(u, v):
        return np.exp(-((u[:, None, :] - v[None, :, :]) ** 2).sum(axis=2) / (2.0 * sigma2))
    kxx, kyy, kxy = gram(x, x), gram(y, y), gram(x, y)
    nx, ny = len(x), len(y)
    off = [(k.sum() - np.trace(k)) / (n * (n - 1)) if n > 1 else np.nan for k, n in ((kxx, nx), (kyy, ny))]
    return kxx.mean() + kyy.mean() - 2.0 * kxy.mean(), off[0] + off[1] - 2.0 * kxy.mean(), kxx.mean(axis=1) - kxy.mean(axis=1), kxy.mean(axis=0) - kyy.mean(axis=1)

"""numpy restatement of d3p_pair_stats_mixed (d3p_amd/csrc/d3p_pair_mixed.hip) and a plain float64 Gower distance beside it.

emulate() restates the stated arithmetic: the pack's float32 multiply u = fl32(x * scale) and its flags, the float32 chain qn <- qn +
|fl32(u_a - u_b)| over the numeric columns ascending, the integer count m of differing codes, and dist = fmaf(w_cat, m, qn) with ONE
rounding -- taken as the float32 rounding of the float64 value w_cat * m + qn, which is the fma's as long as that float64 value is exact.
data() builds such inputs: every x is a multiple of 2^-3 below 2^7 and every scale an odd multiple of 2^-17 below 1, so every u, every
difference and every qn is a multiple of 2^-20 below 2^20, while w_cat * m is a multiple of 2^-2 below 2^10: 40 bits, exact in float64.
(The products x * scale have up to 27 bits and the chain's sums pass 2^4: the float32 roundings of the pack and of the chain do occur.)

exact() is the plain float64 Gower distance sum_k |u_a - u_b| + w_cat * m on the SAME packed u (the pack's product is the bound's input,
not part of it: its rounding is relative to |x| * scale, not to the distance).  BOUND: with u32 = 2^-24 a numeric term passes the
subtraction's rounding, at most dn - 1 of the chain's additions (the first, onto +0, is exact) and the fma's, the categorical term the
fma's alone: at most 2 dn + 1 roundings, |dist - exact| <= gamma(2 dn + 1) * exact, gamma(k) = k u32 / (1 - k u32)."""
import math

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53


def gamma(k, u):
    return k * u / (1.0 - k * u)


def data(seed, n, kind, is_int):
    """A table (n, d) of the module docstring's exactness class; the categorical columns hold few levels, so that codes agree often."""
    rng = np.random.default_rng(seed)
    kind = np.asarray(kind)
    t = rng.integers(-64, 65, (n, len(kind))) if is_int else rng.integers(-512, 513, (n, len(kind))) / 8.0
    codes = np.array([0, 255, 1, 128, 7])[rng.integers(0, 5, (n, len(kind)))]
    return np.where(kind[None, :] == 1, codes, t).astype(np.int32 if is_int else np.float32)


def schema(seed, kind):
    """(scale float32 (d,), w_cat): odd multiples of 2^-17 below 1 on the numeric columns, one of them 0 (a constant column's)."""
    rng = np.random.default_rng(seed)
    scale = ((2 * rng.integers(0, 2 ** 16, len(kind)) + 1) * 2.0 ** -17).astype(np.float32)
    num = np.nonzero(np.asarray(kind) == 0)[0]
    if len(num) > 2:
        scale[num[1]] = 0.0
    return scale, 0.75


def pack(t, kind, scale):
    """(u float32 (n, dn), codes int64 (n, dc), flag bool (n,)) of a table: the pack launch."""
    kind = np.asarray(kind)
    v = t.astype(np.float32)
    with np.errstate(all="ignore"):
        u = v[:, kind == 0] * scale[kind == 0][None, :]                     # float32 x float32: one rounding
        c = v[:, kind == 1]
        ok = (c == np.trunc(c)) & (c >= 0) & (c <= 255)
        flag = ~np.isfinite(v[:, kind == 0]).all(axis=1) | ~np.isfinite(u).all(axis=1) | ~ok.all(axis=1)
        codes = np.where(ok, c, 0).astype(np.int64)
    return u, codes, flag


def _reduce(dist, fa, fb, excl):
    na, nb = dist.shape
    ok = np.ones((na, nb), bool)
    if excl:
        np.fill_diagonal(ok, False)
    out = {"dist": dist, "sum": np.zeros(na), "min": np.full(na, np.inf, dist.dtype), "argmin": np.full(na, -1, np.int64)}
    for i in range(na):
        if fa[i] or fb.any():
            out["sum"][i], out["min"][i] = np.nan, np.nan
        elif ok[i].any():
            row = np.where(ok[i], dist[i], np.inf)
            out["sum"][i] = math.fsum(float(x) for x in dist[i][ok[i]])
            out["argmin"][i] = int(np.argmin(row))                           # (the first index attaining the minimum)
            out["min"][i] = row[out["argmin"][i]]
    return out


def _parts(a, b, kind, scale):
    (ua, ca, fa), (ub, cb, fb) = pack(a, kind, scale), pack(b, kind, scale)
    return ua, ub, (ca[:, None, :] != cb[None, :, :]).sum(axis=2), fa, fb


def emulate(a, b, kind, scale, w_cat, excl=False):
    """The kernel's float32 distances restated: {"dist" (na, nb) float32, "sum" (math.fsum of them), "min", "argmin" (-1: none)}."""
    ua, ub, m, fa, fb = _parts(a, b, kind, scale)
    qn = np.zeros(m.shape, np.float32)
    with np.errstate(all="ignore"):
        for k in range(ua.shape[1]):
            qn = qn + np.abs(ua[:, None, k] - ub[None, :, k])                # float32 subtract, float32 add of its absolute value
        dist = (float(np.float32(w_cat)) * m + qn.astype(np.float64)).astype(np.float32)   # exact in float64: ONE rounding
    return _reduce(dist, fa, fb, excl)


def exact(a, b, kind, scale, w_cat, excl=False):
    """The float64 distance on the packed u (module docstring), reduced in float64."""
    ua, ub, m, fa, fb = _parts(a, b, kind, scale)
    with np.errstate(all="ignore"):
        l1 = np.abs(ua.astype(np.float64)[:, None, :] - ub.astype(np.float64)[None, :, :]).sum(axis=2)
    return _reduce(l1 + float(np.float32(w_cat)) * m, fa, fb, excl)

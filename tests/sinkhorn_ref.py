"""Reference of d3p_softmin_rows and d3p_amd.sinkhorn in plain numpy float64, and the bound d3p_sinkhorn.hip's header derives.

t is formed in float32 exactly as the rule says; q by DIFFERENCES in float64, not by the Gram form; L by a max-shifted log-sum-exp.
softmin_f32 is the rule itself in float32 numpy (any order): what the bound has to hold for.  sinkhorn is the dense log-domain iteration
of d3p_amd.sinkhorn.sinkhorn_divergence with the same schedule, built on softmin_rows."""
import math

import numpy as np

from tests.mmd_ref import LN2, U32, U64, gamma, transform


def softmin_rows(a, b, gam, h, shift=None, scale=None, prev=None, omega=1.0, logw=None, roundings=40):
    """(pot, bound): (na,) float64 each, the potential of the rule and the header's bound on it (omega times the bound on L in bits,
    plus the pot step's roundings), `roundings` float64 additions on a row (d3p_softmin_rows_roundings)."""
    ta, tb = transform(a, shift, scale).astype(np.float64), transform(b, shift, scale).astype(np.float64)
    na, nb, d = ta.shape[0], tb.shape[0], ta.shape[1]
    g0, h = float(np.float32(gam)), np.asarray(h, np.float32).astype(np.float64)
    dp = 32 * -(-d // 32)
    rb, absb, live = (tb * tb).sum(axis=1), np.abs(tb), h > -np.inf
    L, bound = np.full(na, -np.inf), np.zeros(na)
    np.seterr(over="ignore", invalid="ignore", divide="ignore")
    tb, rb, absb, h = tb[live], rb[live], absb[live], h[live]
    step = max(1, 2_000_000 // max(1, len(tb) * d))                 # rows of a at a time: the differences are (rows, nb, d)
    for lo in range(0, na if live.any() else 0, step):
        t = ta[lo:lo + step]
        q = ((t[:, None, :] - tb[None, :, :]) ** 2).sum(axis=2)
        v = h[None, :] - g0 * q
        top = v.max(axis=1, keepdims=True)
        Lr = top[:, 0] + np.log2(np.exp2(v - top).sum(axis=1))
        dq = gamma(dp + 2) * ((t * t).sum(axis=1)[:, None] + rb[None, :]) + 2.0 * gamma(dp) * (np.abs(t) @ absb.T)
        dq = dq + U32 * (q + dq) + (2 * dp + 4) * 2.0 ** -126
        dv = g0 * dq + U32 * (np.abs(h)[None, :] + g0 * (q + dq)) + 127.0 * U32 + math.log2(1.0 + 2.0 * U32)
        L[lo:lo + step] = Lr
        bound[lo:lo + step] = (np.log2(np.exp2(v - Lr[:, None] + dv).sum(axis=1)) + math.log2(1.0 + gamma(64) + gamma(roundings, U64))
                               + math.log2(1.0 + nb * 2.0 ** -126) + U64 * (4.0 + 2.0 * np.abs(Lr)))
    pot = -L
    if prev is not None:
        pot, bound = prev + omega * (pot - prev), omega * bound + U64 * (np.abs(L) + 2.0 * np.abs(prev))
    return pot, bound


def out_h(pot, logw):
    """The h the entry writes beside pot: one float64 addition, one conversion."""
    return (pot + logw.astype(np.float64)).astype(np.float32)


def softmin_f32(a, b, gam, h, shift=None, scale=None):
    """The rule in float32 numpy, the log-sum-exp in float64: pot = -L, (na,)."""
    ta, tb = transform(a, shift, scale), transform(b, shift, scale)
    ra, rb = (ta * ta).sum(axis=1, dtype=np.float32), (tb * tb).sum(axis=1, dtype=np.float32)
    q = np.maximum(np.float32(0), (ra[:, None] + rb[None, :]) - np.float32(2) * (ta @ tb.T))
    v = (np.asarray(h, np.float32)[None, :] - np.float32(gam) * q).astype(np.float64)
    top = v.max(axis=1)
    return -(top + np.log2(np.exp2(v - top[:, None]).sum(axis=1)))


def schedule(x, y, shift, scale, epsilon, scaling):
    """The rungs above epsilon: the squared diameter bound of the transformed tables times scaling^(2 k)."""
    t = np.concatenate([transform(x, shift, scale), transform(y, shift, scale)]).astype(np.float64)
    rungs, e = [], float(((t.max(axis=0) - t.min(axis=0)) ** 2).sum())
    while e > epsilon:
        rungs.append(e)
        e *= scaling * scaling
    return rungs


def sinkhorn(x, y, epsilon, wx, wy, shift=None, scale=None, rungs=(), n_iter=10, debias=True, roundings=40):
    """(divergence, ot_xy, f_x, g_y, worst, walks): the averaged symmetric iteration from potentials of 0 -- a step at each rung, n_iter
    at epsilon, one final step with omega = 1 --; worst is the largest (bound of a walk in bits, plus the u |h| of the float32 h it
    read) x its epsilon ln 2, walks the number of steps on the path."""
    w = [wx / wx.sum(), wy / wy.sum()]
    np.seterr(divide="ignore")
    sides = [(x, y, 0), (y, x, 1)] + ([(x, x, 0), (y, y, 1)] if debias else [])
    logw = [np.log2(w[s[2]]).astype(np.float32) for s in sides]
    pot, reads, worst = [np.zeros(len(s[0])) for s in sides], (1, 0, 2, 3), 0.0

    def step(eps, omega, averaged=True):
        nonlocal worst
        h = [out_h(p, lw) for p, lw in zip(pot, logw)]
        new = []
        for k, s in enumerate(sides):
            hk = h[reads[k]]
            p, bound = softmin_rows(s[0], s[1], 1.0 / (2.0 * eps * LN2), hk, shift, scale, pot[k] if averaged else None, omega, None, roundings)
            worst = max(worst, float((bound.max() + U32 * np.abs(hk[hk > -np.inf]).max()) * eps * LN2))
            new.append(p)
        return new
    for k, eps in enumerate(rungs):
        pot = [p * (eps / (rungs[k + 1] if k + 1 < len(rungs) else epsilon)) for p in step(eps, 0.5)]
    for _ in range(n_iter):
        pot = step(epsilon, 0.5)
    pot = step(epsilon, 1.0, averaged=False)
    c = epsilon * LN2
    ot = c * (w[0] @ pot[0] + w[1] @ pot[1])
    div = c * (w[0] @ (pot[0] - pot[2]) + w[1] @ (pot[1] - pot[3])) if debias else ot
    return div, ot, pot[0] * c, pot[1] * c, worst, len(rungs) + n_iter + 1

"""Comparator of the pair statistics and the fidelity report (d3p_amd/fidelity.py, d3p_amd/csrc/d3p_pair_stats.hip; DESIGN.md section
4w): a numpy float64 restatement with math.fsum sums and exact minima, a float32 emulation of the kernel's distance rule by the chain of
tests/energy_ref.py, the derived error bound, and the report restated on given per-row statistics.  Nothing here reaches a device.

    exact(a, b, exclude_diagonal=False)    -> {"sum": (na,) float64 (fsum), "min": (na,) float64, "argmin": (na,) int64, "dist": (na, nb)}
    emulate(a, b, exclude_diagonal=False)  -> {"sum": float64 (fsum of the float32 distances), "min": float32, "argmin": int64}: the
                                              kernel's rule, the first-index tie rule on q
    bound(ex, nb, d)                       -> {"sum", "min"}: (na,) float64, the largest |device - exact| the rule admits
    energy(sxy, sxx, syy, nx, ny)          -> (d2, d2_unbiased, exy, exx, eyy) in float64 from per-row sums
    report(train, synthetic, holdout, probs, stats=emulate) -> dict of the FidelityReport's numbers
"""
import math

import numpy as np

from tests.energy_ref import U32, U64, _fsum, _half_ulp32, _q32

NONE = -1


def _as2(t):
    t = np.asarray(t)
    return t[:, None] if t.ndim == 1 else t


def _admissible(na, nb, exclude_diagonal):
    ok = np.ones((na, nb), bool)
    if exclude_diagonal:
        assert na == nb
        ok[np.arange(na), np.arange(na)] = False
    return ok


def _bad_rows(a, b):
    """The rows whose outputs are NaN, NaN, none: a non-finite element in the row of a, or anywhere in b."""
    fa = ~np.isfinite(a.astype(np.float64)).all(axis=1)
    return fa | (not np.isfinite(b.astype(np.float64)).all())


def _q64(a, b):
    q = np.zeros((a.shape[0], b.shape[0]), np.float64)
    for c in range(a.shape[1]):
        t = a[:, c].astype(np.float64)[:, None] - b[:, c].astype(np.float64)[None, :]
        q += t * t
    return q


def _reduce(q, dist, ok, bad, min_dtype):
    na = q.shape[0]
    out = {"sum": np.zeros(na, np.float64), "min": np.full(na, np.inf, min_dtype), "argmin": np.full(na, NONE, np.int64)}
    for i in range(na):
        if bad[i]:
            out["sum"][i], out["min"][i] = np.nan, np.nan
            continue
        js = np.nonzero(ok[i])[0]
        if js.size == 0:
            continue
        out["sum"][i] = _fsum(dist[i, js])
        k = js[np.argmin(q[i, js])]          # (numpy's argmin: the first of equal q)
        out["min"][i], out["argmin"][i] = dist[i, k], k
    return out


def exact(a, b, exclude_diagonal=False):
    a, b = _as2(a), _as2(b)
    with np.errstate(all="ignore"):
        q = _q64(a, b)
        dist = np.sqrt(q)
    out = _reduce(q, dist, _admissible(a.shape[0], b.shape[0], exclude_diagonal), _bad_rows(a, b), np.float64)
    out["dist"] = dist
    return out


def emulate(a, b, exclude_diagonal=False):
    a, b = _as2(a), _as2(b)
    with np.errstate(all="ignore"):
        q = _q32(a[:, None, :], b[None, :, :])
        dist = np.sqrt(q).astype(np.float32)
    return _reduce(q, dist.astype(np.float64), _admissible(a.shape[0], b.shape[0], exclude_diagonal), _bad_rows(a, b), np.float32)


def rho(d):
    """The relative error of one distance: (d / 2 + 2) 2^-24 (1 + 2^-10)."""
    return (d / 2.0 + 2.0) * U32 * (1.0 + 2.0 ** -10)


def bound(ex, nb, d):
    """|device - exact| per row.  Every summand is non-negative, so the errors are relative: a distance carries rho(d);
    the float64 sum of nb terms in any order, with the widening and the order's 16 extra additions (slots, segments, butterfly), at most
    (nb + 16) 2^-53.  The minimum of perturbed distances lies within rho of the smallest exact one; its float32 root is rounded once
    more: half an ulp."""
    r = rho(d)
    s, m = np.abs(ex["sum"]), np.abs(ex["min"])
    with np.errstate(all="ignore"):
        return {"sum": (r + (nb + 16.0) * U64) * s, "min": r * m + _half_ulp32(m + r * m)}


def energy(sxy, sxx, syy, nx, ny):
    txy, txx, tyy = _fsum(sxy), _fsum(sxx), _fsum(syy)
    exy, exx, eyy = txy / (nx * ny), txx / (nx * nx), tyy / (ny * ny)
    with np.errstate(all="ignore"):
        ux = np.float64(txx) / np.float64(nx * (nx - 1))
        uy = np.float64(tyy) / np.float64(ny * (ny - 1))
    return 2.0 * exy - exx - eyy, 2.0 * exy - ux - uy, exy, exx, eyy


def report(train, synthetic, holdout=None, probs=(0.05, 0.5, 0.95), stats=emulate):
    """The numbers of fidelity.fidelity_report from per-row statistics of `stats` (emulate: the kernel's float32 minima, which the
    comparisons are made on)."""
    T, S = _as2(train), _as2(synthetic)
    st, ss, tt, ts = stats(S, T), stats(S, S, True), stats(T, T, True), stats(T, S)
    dcr = st["min"]
    out = {"energy_train": energy(st["sum"], ss["sum"], tt["sum"], S.shape[0], T.shape[0]),
           "dcr_quantiles": tuple(float(np.float32(np.quantile(dcr[np.isfinite(dcr)].astype(np.float64), p, method="linear"))) for p in probs),
           "n_exact_copies": int((dcr == 0).sum()),
           "aa_truth": float((ts["min"] > tt["min"]).mean()), "aa_synth": float((dcr > ss["min"]).mean())}
    out["aa"] = 0.5 * (out["aa_truth"] + out["aa_synth"])
    if holdout is not None:
        H = _as2(holdout)
        sh, hh, hs = stats(S, H), stats(H, H, True), stats(H, S)
        out["energy_holdout"] = energy(sh["sum"], ss["sum"], hh["sum"], S.shape[0], H.shape[0])
        out["aa_holdout"] = 0.5 * (float((hs["min"] > hh["min"]).mean()) + float((sh["min"] > ss["min"]).mean()))
        out["privacy_loss"] = out["aa_holdout"] - out["aa"]
        out["closer_to_train"] = float(((dcr < sh["min"]) + 0.5 * (dcr == sh["min"])).mean())
    return out


def closed_form_d1(x, y):
    """The energy distance of two integer samples at d = 1 in exact integer arithmetic: (num, den) of d2 = 2 Sxy / (nx ny) - Sxx / nx^2 -
    Syy / ny^2 over the common denominator nx^2 ny^2."""
    x, y = [int(v) for v in np.asarray(x).ravel()], [int(v) for v in np.asarray(y).ravel()]
    sxy = sum(abs(u - v) for u in x for v in y)
    sxx = sum(abs(u - v) for u in x for v in x)
    syy = sum(abs(u - v) for u in y for v in y)
    nx, ny = len(x), len(y)
    return 2 * sxy * nx * ny - sxx * ny * ny - syy * nx * nx, nx * nx * ny * ny, (sxy, sxx, syy)


assert math.isclose(rho(2), 3.0 * U32 * (1.0 + 2.0 ** -10))

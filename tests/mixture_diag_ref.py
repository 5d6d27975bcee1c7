"""Comparator of d3p_amd.mixture_diagnostics for tests/test_mixture_diag_host.py and tests/test_gpu_mixture_diag.py: a float64 numpy
restatement of the densities of DESIGN.md section 4k, element by element with math.lgamma, and of the draw-sums entry's summation
order.

    log_p_pis(k) = lgamma(k);  log_p_mus;  log_p_sigs;  log_q_pis (xlogy: 0 where alpha_j == 1, whatever pis_j);  log_q_mus
    log_joint = totals + log_p_pis + log_p_mus + log_p_sigs;     log_ratio = totals + log_p_pis + log_p_mus - log_q_pis - log_q_mus
    *_mag: the sum of the magnitudes of a density's terms, for the rounding bounds T 2^-53 sum |terms|
    tree_totals(ll): the entry's order restated (include/d3p_hip.h): per tile of 64 rows the balanced binary tree with zeros past the
                     end, tiles of a strip one by one from 0.0, strips one by one from strip 0's -- the entry's BITS from its own matrix

The totals from a given matrix, their reordering bound, the statistics over the ratios and the Pareto k are tests/guide_diag_ref.py's.
"""
import math

import numpy as np

from tests import guide_diag_ref as G

HALF_LOG_2PI = G.HALF_LOG_2PI
U53 = G.U53
TILE, MAX_STRIPS = 64, 2048


def strips_of(rows):
    """(strips, per): the strip function of d3p_gmm_loglik_draw_sums, of rows alone."""
    tiles = -(-rows // TILE)
    per = -(-tiles // MAX_STRIPS) if tiles else 0
    return (-(-tiles // per), per) if tiles else (0, 0)


def tree_totals(ll):
    """(n,) float64: the entry's summation order on a given (n, rows) float32 matrix."""
    ll = np.asarray(ll)
    n, rows = ll.shape
    strips, per = strips_of(rows)
    tiles = -(-rows // TILE)
    v = np.zeros((n, tiles * TILE), np.float64)
    v[:, :rows] = ll.astype(np.float64)
    v = v.reshape(n, tiles, TILE)
    with np.errstate(invalid="ignore"):
        while v.shape[2] > 1:
            v = v[:, :, 0::2] + v[:, :, 1::2]
        v = v[:, :, 0]
        out = None
        for t in range(strips):
            acc = np.zeros(n, np.float64)
            for i in range(t * per, min((t + 1) * per, tiles)):
                acc = acc + v[:, i]
            out = acc if out is None else out + acc
    return out if out is not None else np.zeros(n, np.float64)


def _xlogy(a, p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a == 0.0, 0.0, a * np.log(p))


def log_p_pis(k):
    return math.lgamma(k)


def log_p_mus(mus, tau):
    mus = np.asarray(mus, np.float64).reshape(len(mus), -1)
    return -(mus * mus / (2.0 * tau * tau)).sum(axis=1) - mus.shape[1] * (math.log(tau) + HALF_LOG_2PI)


def log_p_mus_mag(mus, tau):
    mus = np.asarray(mus, np.float64).reshape(len(mus), -1)
    return (mus * mus / (2.0 * tau * tau)).sum(axis=1) + mus.shape[1] * (abs(math.log(tau)) + HALF_LOG_2PI)


def log_p_sigs(sigs):
    s = np.asarray(sigs, np.float64).reshape(len(sigs), -1)
    return (-2.0 * np.log(s) - 1.0 / s).sum(axis=1)


def log_p_sigs_mag(sigs):
    s = np.asarray(sigs, np.float64).reshape(len(sigs), -1)
    return (2.0 * np.abs(np.log(s)) + 1.0 / s).sum(axis=1)


def alpha_of(alpha_log):
    return np.exp(np.asarray(alpha_log, np.float32).astype(np.float64))


def log_q_pis(pis, alpha):
    pis = np.asarray(pis, np.float64)
    const = math.lgamma(float(alpha.sum())) - sum(math.lgamma(float(a)) for a in alpha)
    return const + _xlogy(alpha[None, :] - 1.0, pis).sum(axis=1)


def log_q_pis_mag(pis, alpha):
    pis = np.asarray(pis, np.float64)
    const = abs(math.lgamma(float(alpha.sum()))) + sum(abs(math.lgamma(float(a))) for a in alpha)
    return const + np.abs(_xlogy(alpha[None, :] - 1.0, pis)).sum(axis=1)


def log_q_mus(mus, loc):
    mus = np.asarray(mus, np.float64).reshape(len(mus), -1)
    dev = mus - np.asarray(loc, np.float32).astype(np.float64).reshape(1, -1)
    return -(dev * dev / 2.0).sum(axis=1) - mus.shape[1] * HALF_LOG_2PI


def log_q_mus_mag(mus, loc):
    mus = np.asarray(mus, np.float64).reshape(len(mus), -1)
    dev = mus - np.asarray(loc, np.float32).astype(np.float64).reshape(1, -1)
    return (dev * dev / 2.0).sum(axis=1) + mus.shape[1] * HALF_LOG_2PI


def log_joint(totals, k, mus, sigs, tau):
    return totals + log_p_pis(k) + log_p_mus(mus, tau) + log_p_sigs(sigs)


def log_ratio(totals, k, pis, mus, alpha_log, mus_loc, tau):
    return totals + log_p_pis(k) + log_p_mus(mus, tau) - log_q_pis(pis, alpha_of(alpha_log)) - log_q_mus(mus, mus_loc)


def density_bound(k, d, pis, mus, sigs, alpha_log, mus_loc, tau, with_sigs):
    """Float64 rounding of the O(k d) density sums for two evaluations in different orders: a density of T terms, each formed with up
    to four roundings and lgamma / log / exp within an ulp or two (8 roundings allowed), errs by at most (T + 8) 2^-53 sum |terms| per
    evaluation; twice that for two.  Terms: mus k d + 1, sigs 2 k d, q(pis) k + 2 (+ alpha = exp(alpha_log), one more ulp inside its
    terms), q(mus) k d + 1."""
    kd = k * d
    b = (kd + 9) * log_p_mus_mag(mus, tau) + 8 * abs(math.lgamma(k))
    if with_sigs:
        b = b + (2 * kd + 8) * log_p_sigs_mag(sigs)
    else:
        alpha = alpha_of(alpha_log)
        b = b + (k + 10) * log_q_pis_mag(pis, alpha) + (kd + 9) * log_q_mus_mag(mus, mus_loc)
        # alpha = exp(alpha_log) may itself differ by an ulp (2^-52 relative) between two evaluations, and lgamma(1) = lgamma(2) = 0
        # leaves no magnitude to scale by: absolute slack alpha_j ulp (|log pis_j| + |digamma(alpha_j)|) + (k + 1) A ulp |digamma(A)|
        # with A = sum alpha and |digamma(a)| <= 1 / a + |log a| + 1 for a > 0
        dig = lambda a: 1.0 / a + np.abs(np.log(a)) + 1.0   # noqa: E731
        with np.errstate(divide="ignore"):
            lp = np.where(np.asarray(pis, np.float64) > 0, np.abs(np.log(np.asarray(pis, np.float64))), 0.0)
        A = float(alpha.sum())
        b = b + 2.0 * ((alpha[None, :] * (lp + dig(alpha)[None, :])).sum(axis=1) + (k + 1) * A * dig(A))
    return 2.0 * U53 * b

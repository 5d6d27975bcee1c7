"""numpy / float64 restatements of d3p_amd.sliced for its tests: the projection with its header's bound, W_p on the n_a n_b level grid."""
import math

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53


def project(x, theta, shift, chunk):
    """(p, bound): the float64 projections of the float32 t = fl32(x - shift) and the header's bound per element."""
    t = x.astype(np.float32)
    if shift is not None:
        t = t - shift.astype(np.float32)[None, :]          # one float32 subtraction
    t64, th64 = t.astype(np.float64), theta.astype(np.float64)
    dp = -(-x.shape[1] // chunk) * chunk
    gamma = dp * U32 / (1.0 - dp * U32)
    return t64 @ th64, gamma * (np.abs(t64) @ np.abs(th64)) + dp * 2.0 ** -126


def wasserstein(a, b, p):
    """(W_p^p, sum |term| / (n_a n_b)) of two sorted samples: Python-integer overlaps on the level grid, float64 terms, math.fsum."""
    na, nb = len(a), len(b)
    i = j = level = 0
    terms = []
    while level < na * nb:
        nxt = min((i + 1) * nb, (j + 1) * na)
        delta = abs(float(a[i]) - float(b[j]))
        terms.append(float(nxt - level) * (delta * delta if p == 2 else delta))
        level = nxt
        i += level == (i + 1) * nb
        j += level == (j + 1) * na
    return (math.fsum(terms) / (na * nb),) * 2   # (every term is >= 0)


def wasserstein_brute(a, b, p):
    na, nb = len(a), len(b)   # every level of the grid, one by one (small n only)
    return math.fsum(abs(float(a[k // nb]) - float(b[k // na])) ** p for k in range(na * nb)) / (na * nb)


def w2_bound(lib, na, nb, sum_abs):
    """gamma_k sum |term| / (n_a n_b) with the entry's count of roundings plus the 3 of a term (which the reference's terms carry too)."""
    k = lib.d3p_column_w2_distance_roundings(na, nb) + 3
    return (k * U64 / (1.0 - k * U64) + 3.0 * U64) * sum_abs

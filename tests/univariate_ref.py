"""Plain numpy / float64 restatements of d3p_amd.univariate for its tests: the order keys, the sorted columns, the doubled midranks, the
integer KS numerator and the Wasserstein-1 sum with its bound.  Tables are handled as their uint32 words."""
import math

import numpy as np

U = 2.0 ** -53


def keys(words, is_int):
    """The order key of stored words (uint32): float32 with -0 as +0, int32 with the sign bit flipped."""
    u = words.astype(np.uint32)
    if is_int:
        return u ^ np.uint32(0x80000000)
    u = np.where((u << np.uint32(1)) == 0, np.uint32(0), u)
    return np.where(u >> np.uint32(31) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def words_of(k, is_int):
    k = k.astype(np.uint32)
    if is_int:
        return k ^ np.uint32(0x80000000)
    return np.where(k >> np.uint32(31) != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)


def values(k, is_int):
    w = words_of(k, is_int)
    return w.view(np.int32).astype(np.float64) if is_int else w.view(np.float32).astype(np.float64)


def is_nan(words):
    return (words.astype(np.uint32) << np.uint32(1)) > np.uint32(0xff000000)


def sort_columns(x_words, is_int):
    """(n, d) words -> (d, n) words, every column in ascending key order."""
    return words_of(np.sort(keys(x_words, is_int).T, axis=1), is_int)


def ranks2(x_words, is_int):
    """(n, d) int64: lo + hi + 1 by np.searchsorted on the sorted keys; 0 in a float32 column that holds a NaN."""
    k = keys(x_words, is_int)
    out = np.zeros(k.shape, np.int64)
    for c in range(k.shape[1]):
        if not is_int and is_nan(x_words[:, c]).any():
            continue
        s = np.sort(k[:, c])
        out[:, c] = np.searchsorted(s, k[:, c], "left") + np.searchsorted(s, k[:, c], "right") + 1
    return out


def cdf_column(a_words, b_words, is_int):
    """(ks_num, the key of ks_at, w1 by fsum, sum |term|) of one column pair, without the flag rules."""
    ka, kb = np.sort(keys(a_words, is_int)), np.sort(keys(b_words, is_int))
    na, nb = len(ka), len(kb)
    pooled = np.unique(np.concatenate([ka, kb]))
    i = np.searchsorted(ka, pooled, "right").astype(np.int64)
    j = np.searchsorted(kb, pooled, "right").astype(np.int64)
    num = np.abs(i * nb - j * na)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (num[:-1].astype(np.float64) / (float(na) * float(nb))) * np.diff(values(pooled, is_int))
    return int(num.max()), int(pooled[np.argmax(num)]), math.fsum(terms), math.fsum(np.abs(terms))


def w1_bound(lib, na, nb, sum_abs):
    """gamma_k sum |term| from the entry's count of roundings, plus the 4 u per term of the float64 terms above."""
    k = lib.d3p_column_cdf_distance_roundings(na, nb)
    return (k * U / (1.0 - k * U) + 4.0 * U) * sum_abs

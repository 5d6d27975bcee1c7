"""A numpy restatement of the rule of d3p_marginals (d3p_amd/csrc/d3p_marginals.hip) and of the float64 summaries of
d3p_amd.marginals: the codes by ``searchsorted(side="left")`` with NaN taken first, the counts by ``np.add.at``, the lexicographic pair
order, total variation distances and Cramer's V.  A plain module (no test in it)."""
import numpy as np


def pair_index(i, j, d):
    """The lexicographic index of the pair i < j among the columns 0 .. d - 1."""
    assert 0 <= i < j < d
    return i * (2 * d - i - 1) // 2 + (j - i - 1)


def pairs(d):
    """(P, 2): the pairs i < j in the order of pair_index."""
    return np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int64).reshape(-1, 2)


def codes(x, edges, nbins, B):
    """The (n, d) codes of the table x: edges (d, >= max(nbins) - 1) float32, of which column c uses its first nbins[c] - 1."""
    x = np.asarray(x)
    x = x[:, None] if x.ndim == 1 else x
    v = x.astype(np.float32)
    out = np.empty(v.shape, dtype=np.int64)
    for c in range(v.shape[1]):
        e = np.asarray(edges[c], dtype=np.float32)[:int(nbins[c]) - 1]
        nan = np.isnan(v[:, c])
        out[:, c] = np.where(nan, B, np.searchsorted(e, np.where(nan, np.float32(0), v[:, c]), side="left"))
    return out


def counts(x, edges, nbins, B):
    """(one_way (d, K), two_way (P, K, K)) as int64."""
    cd = codes(x, edges, nbins, B)
    n, d = cd.shape
    K = B + 1
    one = np.zeros((d, K), dtype=np.int64)
    for c in range(d):
        np.add.at(one[c], cd[:, c], 1)
    pr = pairs(d)
    two = np.zeros((len(pr), K, K), dtype=np.int64)
    for p, (i, j) in enumerate(pr):
        assert p == pair_index(i, j, d)
        np.add.at(two[p], (cd[:, i], cd[:, j]), 1)
    return one, two


def counts_product(x, edges, nbins, B):
    """The same counts from ONE product of the n x d K indicator matrix with itself (float64, exact below 2^53): what the tests of large
    or wide tables use, where a call of np.add.at per pair takes too long.  tests/test_marginals_host.py holds it equal to counts."""
    cd = codes(x, edges, nbins, B)
    n, d = cd.shape
    K = B + 1
    ind = np.zeros((n, d * K), dtype=np.float64)
    ind[np.arange(n)[:, None], np.arange(d)[None, :] * K + cd] = 1.0
    g = np.rint(ind.T @ ind).astype(np.int64).reshape(d, K, d, K)
    pr = pairs(d)
    one = np.stack([np.diag(g[c, :, c, :]) for c in range(d)])
    two = g[pr[:, 0], :, pr[:, 1], :] if len(pr) else np.zeros((0, K, K), dtype=np.int64)
    return one, two


def tvd(ca, na, cb, nb):
    """1/2 sum |p - q| over the last axis, float64."""
    return 0.5 * np.abs(np.asarray(ca, np.float64) / na - np.asarray(cb, np.float64) / nb).sum(axis=-1)


def cramers_v(tab, n):
    """Cramer's V of one (K, K) count table over n rows; 0 with fewer than two non-empty rows or columns."""
    o = np.asarray(tab, np.float64)
    r, c = o.sum(axis=1), o.sum(axis=0)
    k = min(int((r > 0).sum()), int((c > 0).sum())) - 1
    if k < 1:
        return 0.0
    ex = np.outer(r, c) / n
    pos = ex > 0
    chi2 = (((o - ex) ** 2)[pos] / ex[pos]).sum()
    return min(1.0, float(np.sqrt(chi2 / (n * k))))


def summaries(one_a, two_a, na, one_b, two_b, nb):
    """The float64 summaries of two tables' counts, as d3p_amd.marginals.marginal_fidelity reports them."""
    K = one_a.shape[1]
    P = two_a.shape[0]
    t1 = tvd(one_a, na, one_b, nb)
    t2 = tvd(two_a.reshape(P, K * K), na, two_b.reshape(P, K * K), nb) if P else np.zeros(0)
    va = np.array([cramers_v(t, na) for t in two_a], dtype=np.float64)
    vb = np.array([cramers_v(t, nb) for t in two_b], dtype=np.float64)
    diff = np.abs(va - vb)
    return {"tvd_one_way": t1, "tvd_two_way": t2, "tvd_one_way_mean": float(t1.mean()), "tvd_two_way_mean": float(t2.mean()) if P else float("nan"),
            "cramers_v_a": va, "cramers_v_b": vb, "assoc_diff_mean": float(diff.mean()) if P else float("nan"),
            "assoc_diff_max": float(diff.max()) if P else float("nan"), "missing_a": one_a[:, K - 1] / na, "missing_b": one_b[:, K - 1] / nb}


def quantile_edges(col, bins):
    """The quantile rule of bin_edges for one column: distinct order statistics at ranks ceil(k m / bins) - 1 of the finite values,
    without the maximum."""
    v = np.sort(np.asarray(col, np.float64)[np.isfinite(np.asarray(col, np.float64))])
    m = len(v)
    if m == 0:
        return []
    return sorted({float(v[max(-(-k * m // bins) - 1, 0)]) for k in range(1, bins)} - {float(v[-1])})

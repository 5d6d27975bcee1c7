"""numpy restatements of what d3p_amd/csrc/d3p_classify.hip computes: the bin map of d3p_binary_curve, its two histograms, the pair
counts and the fixed-point sums; the confusion counts of d3p_predict_confusion from the stored matrices; and, as a comparator only, the
exact Mann-Whitney AUC of a score vector (midranks via argsort).  Everything is an integer, so every comparison is by value."""
import numpy as np

BINS = 0x7E001
HALF = 0x3F000
FIXED = 2.0 ** 36


def bin_of(p):
    """bin(p) = c(p) for p < 0.5f, 2 * 0x3F000 - c(1.0f - p) otherwise, c(x) = float_as_uint(x) >> 12; -0.0f as 0.  p: float32 in [0, 1]."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1) + np.float32(0.0)     # -0.0f + 0.0f = +0.0f
    low = p.view(np.uint32).astype(np.int64) >> 12
    mirror = np.float32(1.0) - p                                               # float32; exact for p in [0.5, 1]
    high = 2 * HALF - (mirror.view(np.uint32).astype(np.int64) >> 12)
    return np.where(p < np.float32(0.5), low, high)


def valid(p, y):
    p, y = np.asarray(p, np.float32).reshape(-1), np.asarray(y).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (p >= 0) & (p <= 1) & ((y == 0) | (y == 1))


def curve(p, y, B):
    """(hist (2, BINS) int64, calib (3, B) int64, summary [n_invalid, P, N, conc, same, ks numerator] as Python ints) of the valid rows."""
    p, y = np.asarray(p, np.float32).reshape(-1), np.asarray(y).reshape(-1).astype(np.int64)
    ok = valid(p, y)
    n_invalid = int((~ok).sum())
    p, y = p[ok], y[ok]
    hist = np.zeros((2, BINS), np.int64)
    np.add.at(hist, (y, bin_of(p)), 1)
    b = np.minimum(B - 1, ((p + np.float32(0.0)) * np.float32(B)).astype(np.int64))   # the product in float32
    calib = np.zeros((3, B), np.int64)
    np.add.at(calib[0], b, 1)
    np.add.at(calib[1], b, y)
    np.add.at(calib[2], b, (p.astype(np.float64) * FIXED).astype(np.uint64).astype(np.int64))
    return hist, calib, [n_invalid] + pair_counts(hist)


def pair_counts(hist):
    """[P, N, sum_b pos_b #{neg in bins below b}, sum_b pos_b neg_b, max_k |b_k P - a_k N|] as Python ints (arbitrary precision); a_k /
    b_k: the positives / negatives of the bins 0..k."""
    neg, pos = hist[0].astype(object), hist[1].astype(object)
    b, a = np.cumsum(neg), np.cumsum(pos)
    below = np.concatenate([[0], b[:-1]])
    P, N = int(pos.sum()), int(neg.sum())
    return [P, N, int((pos * below).sum()), int((pos * neg).sum()), int(np.abs(b * P - a * N).max())]


def auc_bounds(summary):
    """(auc_lo, auc, auc_hi) in float64 from [n_invalid, P, N, conc, same]; NaN where P N == 0."""
    _, P, N, conc, same = summary[:5]
    pn = float(P) * float(N)
    if not pn:
        return (float("nan"),) * 3
    return conc / pn, (conc + same / 2) / pn, (conc + same) / pn


def exact_auc(p, y):
    """The Mann-Whitney AUC: (sum of the positives' midranks - P (P + 1) / 2) / (P N), ties at half weight."""
    p, y = np.asarray(p, np.float64).reshape(-1), np.asarray(y).reshape(-1).astype(np.int64)
    order = np.argsort(p, kind="stable")
    s = p[order]
    start = np.concatenate([[True], s[1:] != s[:-1]])
    first = np.flatnonzero(start)
    last = np.concatenate([first[1:], [s.size]])                 # one past each group's end
    mid = (first + 1 + last) / 2.0                                # mean of the ranks first + 1 .. last
    ranks = np.empty(s.size, np.float64)
    ranks[order] = np.repeat(mid, last - first)
    P = int((y == 1).sum())
    N = y.size - P
    if P == 0 or N == 0:
        return float("nan")
    return (ranks[y == 1].sum() - P * (P + 1) / 2.0) / (float(P) * float(N))


def calibration_errors(calib, rows):
    """(ece, mce) by d3p_amd.classification._calibration_errors' steps."""
    ece, mce = 0.0, 0.0
    for b in range(calib.shape[1]):
        count, pos, total = (int(v) for v in calib[:, b])
        if count:
            gap = abs(pos / count - (total / FIXED) / count)
            ece, mce = ece + (count / rows) * gap, max(mce, gap)
    return ece, mce


def ks_statistic(hist, P, N):
    """max |tpr - fpr| over the bin edges, counted from the TOP bin down (the ROC's direction): the value summary[5] / (P N) has."""
    if not (P and N):
        return float("nan")
    cn, cp = np.cumsum(hist[0][::-1]).astype(object), np.cumsum(hist[1][::-1]).astype(object)
    return int(np.abs(cp * N - cn * P).max()) / (float(P) * float(N))


def confusion(mu, v, y, tau):
    """(10, n) int64 from the stored matrices mu (n, rows) float32 and v (n, rows) int32, labels y (rows,) and up to four thresholds."""
    mu, v, y = np.asarray(mu, np.float32), np.asarray(v), np.asarray(y, np.float32).reshape(-1)
    out = np.zeros((10, mu.shape[0]), np.int64)
    out[0] = (v.astype(np.float32) == y[None]).sum(1)
    out[1] = np.isnan(mu).sum(1)
    with np.errstate(invalid="ignore"):
        for j, t in enumerate(tau):
            ge = mu >= np.float32(t)
            out[2 + 2 * j] = (ge & (y[None] == 1)).sum(1)
            out[3 + 2 * j] = (ge & (y[None] == 0)).sum(1)
    return out

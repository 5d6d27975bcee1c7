"""Comparator of d3p_psis_loo / d3p_amd.criteria.loo for tests/test_loo_host.py and tests/test_gpu_loo.py: a float64 numpy restatement
of PSIS-LOO for ONE column of a draws x rows log-likelihood matrix, written from Vehtari, Gelman & Gabry (2017, section 2.1 and its
appendix), Vehtari et al. (2024, "Pareto smoothed importance sampling") and Zhang & Stephens (2009).

    x[s]  = -ll[s] - max_s(-ll[s])                               log importance ratios, the largest 0
    lppd  = logsumexp_s ll - log n
    M     = ceil(min(n / 5, 3 sqrt n))                           relative efficiency 1
    cut   = max((M+1)-th largest x, log DBL_MIN);  tail = {s : x[s] > cut}, T <= M draws, ascending by (value, draw index)
    e_j   = exp(x_j) - exp(cut);  m = 30 + floor(sqrt T);  b_i = 1 / e_T + (1 - sqrt(m / (i - 0.5))) / (3 e_q),  q = floor(T/4 + 0.5)
    k_i   = mean_j log1p(-b_i e_j);  L_i = T (log(-b_i / k_i) - k_i - 1);  w_i = 1 / sum_j exp(L_j - L_i), below 10 eps dropped
    b     = sum w_i b_i;  k = mean_j log1p(-b e_j);  sigma = -k / b;  k <- (T k + 5) / (T + 10)
    T <= 4, k or sigma not finite, sigma <= 0: the raw x stand, k = +inf; else with p_j = (j - 0.5) / T
    x_j   = min(0, log(exp(cut) + sigma expm1(-k log1p(-p_j)) / k))   (-sigma log1p(-p_j) where |k| < eps)
    elpd  = logsumexp_s (x[s] + ll[s]) - logsumexp_s x[s]

Special values: a NaN makes all three NaN; a +inf makes elpd and k NaN and lppd +inf; a -inf makes elpd -inf and k +inf, lppd finite
unless every draw is -inf.

`psis_column(col)` is the reference (numpy's own sums and means).  `psis_column(col, kernel_order=True, rng=...)` restates the same
steps in the summation orders of k_psis_loo (d3p_amd/csrc/d3p_psis.hip: 8 strided partials per column combined in order; sequential
sums over the tail per candidate and over the candidates; 64 strided partials merged by an xor butterfly for the last sums over the
tail) and, with a generator, moves every exp / log / log1p / expm1 result by a random whole number of ulps in [-2, 2]: the model of a
device libm.  Equal tail values are interchangeable in every sum, so the kernel keeps no draw index; the restatement does likewise.

Bound of the device's float32 outputs against the reference: |got - v| <= 2^-24 |v| + the float64 term, which is calibrated, not
guessed (`calibrate()`; tests/test_loo_host.py re-runs it on a part of the sweep): the largest deviation of the perturbed kernel-order
restatement from the reference over `sweep_columns()` -- columns of the GPU test's direct-entry matrices, 3 perturbation seeds -- times
4.  elpd and lppd are measured relative to max(|v|, 1).  k is measured relative to the column's conditioning
cond = max(1, exp(x_1) / e_1) = 1 / (1 - exp(cut - x_1)): e_j = exp(x_j) - exp(cut) carries 2 ulps of each exp, at most 2^-51 exp(x_j) /
e_j of itself, largest at j = 1, the tail draw next to the cut, and k is a mean of log1p of ratios of the e_j.

    recorded:  elpd 1.6e-14, lppd 4.5e-15 (relative to max(|v|, 1));  k 662 x 2^-52 x cond (near-tied, n = 225; random columns: 132)
    F64_ELPD = F64_LPPD = 4 x 1.6e-14 = 6.4e-14;   F64_K_PER_COND = 4 x 662 x 2^-52 = 5.9e-13
    (in absolute terms the largest deviations of k were 1.7e-13 on the random and 1.2e-6 on the near-tied columns)

How tight that leaves the check of k, as bound / (2^-24 |k|) over all columns of the sweep's matrices: random columns median 1.001, 99th
percentile 4.9, largest 463 (one column whose x_1 lies 1e-6 above the cut); near-tied columns, where the whole tail lies a few float32
ulps above the cut (cond 4e6 .. 1.3e8), median 18, largest 1.0e4.  On those the check of k is as loose as the fit is ill-conditioned.
"""
import math
import sys

import numpy as np

LOG_DBL_MIN = math.log(sys.float_info.min)
assert LOG_DBL_MIN == -708.3964185322641
EPS = sys.float_info.epsilon

F64_ELPD = 6.4e-14
F64_LPPD = 6.4e-14
F64_K_PER_COND = 5.9e-13
ROUND32 = 2.0 ** -24

DIRECT_N = (1, 2, 5, 6, 20, 21, 25, 26, 63, 64, 65, 128, 129, 225, 226, 1000, 4097)
DIRECT_ROWS = (1, 63, 64, 65, 127, 128, 129, 257)


def tail_len(n):
    """M = ceil(min(n / 5, 3 sqrt n))."""
    return int(math.ceil(min(n / 5.0, 3.0 * math.sqrt(n))))


class _Fn:
    """exp, log, log1p, expm1: numpy's, or numpy's moved by a random whole number of ulps in [-2, 2]."""

    def __init__(self, rng=None):
        self.rng = rng

    def _move(self, v):
        if self.rng is None:
            return v
        v = np.asarray(v, np.float64)
        step = self.rng.integers(-2, 3, size=v.shape).astype(np.float64)
        with np.errstate(invalid="ignore"):
            moved = v + step * np.spacing(np.abs(v))
        return np.where(np.isfinite(v), moved, v)

    def exp(self, v):
        with np.errstate(over="ignore", invalid="ignore"):
            return self._move(np.exp(v))

    def log(self, v):
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._move(np.log(v))

    def log1p(self, v):
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._move(np.log1p(v))

    def expm1(self, v):
        with np.errstate(over="ignore", invalid="ignore"):
            return self._move(np.expm1(v))


def _seq(v):
    """Sum in index order."""
    v = np.asarray(v, np.float64)
    return np.add.accumulate(v)[-1] if v.size else np.float64(0.0)


def _strided(v, lanes):
    """lanes partial sums in index order, lane l over v[l::lanes]."""
    return np.array([_seq(v[l::lanes]) for l in range(lanes)], np.float64)


def _butterfly(p, op=np.add):
    """The xor butterfly 32, 16, .., 1 over 64 lanes; every lane ends with the same value."""
    p = np.asarray(p, np.float64).copy()
    idx = np.arange(64)
    off = 32
    while off >= 1:
        p = op(p, p[idx ^ off])
        off >>= 1
    return p[0]


def _logsumexp(v):
    v = np.asarray(v, np.float64)
    top = v.max()
    if not np.isfinite(top):
        return top
    return top + np.log(np.exp(v - top).sum())


def psis_column(col, kernel_order=False, rng=None):
    """{"elpd", "lppd", "k", "T", "tail", "cond"} of one column (file docstring); "tail" is the boolean membership over the draws,
    "cond" the conditioning max(1, exp(x_1) / e_1) of the fit (1 where there is none)."""
    ll32 = np.asarray(col)
    ll = ll32.astype(np.float64)
    n = ll.size
    none = np.zeros(n, bool)
    if np.isnan(ll).any():
        return {"elpd": np.nan, "lppd": np.nan, "k": np.nan, "T": 0, "tail": none, "cond": 1.0}
    if np.isposinf(ll).any():
        return {"elpd": np.nan, "lppd": np.inf, "k": np.nan, "T": 0, "tail": none, "cond": 1.0}
    f = _Fn(rng)
    top = ll.max()
    if top == -np.inf:
        lppd = -np.inf
    elif kernel_order:
        part = np.array([_seq(f.exp(ll[l::8] - top)) if ll[l::8].size else 0.0 for l in range(8)])
        lppd = top + f.log(_seq(part)) - f.log(float(n))
    else:
        lppd = top + np.log(np.exp(ll - top).sum()) - np.log(float(n))
    if np.isneginf(ll).any():
        return {"elpd": -np.inf, "lppd": float(lppd), "k": np.inf, "T": 0, "tail": none, "cond": 1.0}
    x = -ll - np.max(-ll)
    mn = ll.min()
    M = tail_len(n)
    cut = max(np.sort(x)[::-1][min(M, n - 1)], LOG_DBL_MIN)
    tail = x > cut
    idx = np.nonzero(tail)[0]
    idx = idx[np.lexsort((idx, x[idx]))]
    T = idx.size
    assert T <= M
    xt, llt = x[idx], ll[idx]
    ecut = f.exp(cut)
    k_out, xs, cond = np.inf, xt, 1.0
    if T > 4:
        with np.errstate(all="ignore"):
            e = f.exp(xt) - ecut
            cond = max(1.0, float(np.exp(xt[0])) / e[0]) if e[0] > 0.0 else np.inf
            m = 30 + int(math.floor(math.sqrt(T)))
            q = int(math.floor(T / 4.0 + 0.5))
            i = np.arange(1, m + 1, dtype=np.float64)
            b_i = 1.0 / e[-1] + (1.0 - np.sqrt(m / (i - 0.5))) / (3.0 * e[q - 1])
            lp = f.log1p(-b_i[:, None] * e[None, :])
            if kernel_order:
                k_i = np.add.accumulate(lp, axis=1)[:, -1] / T
            else:
                k_i = lp.mean(axis=1)
            L = T * (f.log(-b_i / k_i) - k_i - 1.0)
            ex = f.exp(L[None, :] - L[:, None])
            w = 1.0 / (np.add.accumulate(ex, axis=1)[:, -1] if kernel_order else ex.sum(axis=1))
            w = np.where(w < 10.0 * EPS, 0.0, w)
            if kernel_order:
                w = w / _seq(w)
                b = _seq(w * b_i)
                k = _butterfly(_strided(f.log1p(-b * e), 64)) / T
            else:
                w = w / w.sum()
                b = (w * b_i).sum()
                k = np.log1p(-b * e).mean()
            sigma = -k / b
            kreg = (T * k + 5.0) / (T + 10.0)
            if np.isfinite(k) and np.isfinite(sigma) and sigma > 0.0:
                k_out = float(kreg)
                p = (np.arange(1, T + 1, dtype=np.float64) - 0.5) / T
                l1 = f.log1p(-p)
                qv = -sigma * l1 if abs(kreg) < EPS else sigma * f.expm1(-kreg * l1) / kreg
                xs = np.minimum(0.0, f.log(ecut + qv))
    if kernel_order:
        rest = ~tail
        xr, lr = x[rest], ll[rest]
        pos = np.nonzero(rest)[0]
        dnt = nnt = np.float64(0.0)
        d_part, n_part = [], []
        for l in range(8):
            sel = pos % 8 == l
            d_part.append(_seq(f.exp(xr[sel])))
            n_part.append(_seq(f.exp((xr[sel] + lr[sel]) - mn)))
        dnt, nnt = _seq(d_part), _seq(n_part)
        v = xs + llt
        den = dnt + _butterfly(_strided(f.exp(xs), 64))
        lmax = v.max() if T else -np.inf
        high = max(lmax, mn)
        num = nnt * f.exp(mn - high) + _butterfly(_strided(f.exp(v - high), 64))
        elpd = high + f.log(num) - f.log(den)
    else:
        xx = x.copy()
        xx[idx] = xs
        elpd = _logsumexp(xx + ll) - _logsumexp(xx)
    return {"elpd": float(elpd), "lppd": float(lppd), "k": k_out, "T": int(T), "tail": tail, "cond": cond}


def psis_matrix(ll):
    """(elpd, lppd, k, T, cond) float64 / int arrays over the columns of ll (n, rows)."""
    out = [psis_column(ll[:, r]) for r in range(ll.shape[1])]
    return (np.array([o["elpd"] for o in out]), np.array([o["lppd"] for o in out]), np.array([o["k"] for o in out]),
            np.array([o["T"] for o in out]), np.array([o["cond"] for o in out]))


def bounds(elpd, lppd, k, cond):
    """Per-value bounds of the device's float32 outputs against the float64 reference (file docstring); non-finite values get 0 and
    are compared by equality."""
    def one(v, term):
        v = np.asarray(v, np.float64)
        with np.errstate(invalid="ignore"):
            b = ROUND32 * np.abs(v) + term
        return np.where(np.isfinite(v), b, 0.0)
    with np.errstate(invalid="ignore"):
        return (one(elpd, F64_ELPD * np.maximum(np.abs(elpd), 1.0)), one(lppd, F64_LPPD * np.maximum(np.abs(lppd), 1.0)),
                one(k, F64_K_PER_COND * np.asarray(cond, np.float64)))


def within(got, ref, bound):
    """Elementwise: equal where the reference is not finite, else inside the bound."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(invalid="ignore"):
        return np.where(fin, np.abs(got - ref) <= bound, same)


# ------------------------------------------------------------------------------------------------ the direct-entry sweep
def random_matrix(n, rows, seed):
    """float32 (n, rows): columns of log-likelihoods as a regression gives them, each column with its own spread, some heavy-tailed."""
    r = np.random.default_rng([seed, n, rows])
    scale = 10.0 ** r.uniform(-2.0, 0.7, rows)
    centre = r.normal(-2.0, 2.0, rows)
    z = r.normal(size=(n, rows))
    heavy = r.random(rows) < 0.3
    z = np.where(heavy[None, :], z * np.exp(0.8 * r.normal(size=(n, rows))), z)
    return (centre[None, :] - scale[None, :] * z * z).astype(np.float32)


def near_tied_matrix(n, rows, seed):
    """float32 (n, rows): every column takes its draws from a few adjacent float32 values (exact ties and one-ulp gaps at the cut)."""
    r = np.random.default_rng([seed, n, rows, 7])
    base = r.normal(-3.0, 1.0, rows).astype(np.float32)
    span = r.integers(2, 12, rows)
    steps = r.integers(0, span[None, :], size=(n, rows))
    out = np.empty((n, rows), np.float32)
    for c in range(rows):
        ladder = np.empty(span[c], np.float32)
        v = base[c]
        for j in range(span[c]):
            ladder[j] = v
            v = np.nextafter(v, np.float32(-np.inf))
        out[:, c] = ladder[steps[:, c]]
    return out


def low_cut_column(n=64):
    """8 draws within a few nats of the smallest ll, the others more than 708.4 above it: the (M+1)-th largest x lies below
    log DBL_MIN (n >= 40, so that M >= 8)."""
    r = np.random.default_rng(4)
    col = (-5.0 + r.random(n)).astype(np.float32)
    col[:8] = (-720.0 + 3.0 * r.random(8)).astype(np.float32)
    return col


FIXED_NAMES = ("ties", "equal", "one_neg_inf", "all_neg_inf", "one_nan", "one_pos_inf", "low_cut", "plain")


def fixed_columns():
    """float32 (100, 8), the columns named by FIXED_NAMES: 10 distinct values x 10; all draws equal; one -inf draw; every draw -inf; one
    NaN (beside a -inf); one +inf; a cut below log DBL_MIN; an ordinary column."""
    n = 100
    plain = (-1.0 - np.random.default_rng(9).normal(size=n) ** 2).astype(np.float32)
    cols = {name: plain.copy() for name in FIXED_NAMES}
    cols["ties"] = (np.repeat(np.arange(10, dtype=np.float32), 10) * -0.5)[np.random.default_rng(3).permutation(n)]
    cols["equal"] = np.full(n, -1.25, np.float32)
    cols["one_neg_inf"][17] = -np.inf
    cols["all_neg_inf"] = np.full(n, -np.inf, np.float32)
    cols["one_nan"][40] = np.nan
    cols["one_nan"][41] = -np.inf
    cols["one_pos_inf"][99] = np.inf
    cols["low_cut"] = low_cut_column(n)
    return np.stack([cols[name] for name in FIXED_NAMES], axis=1)


def direct_cases():
    """(n, rows) of the direct-entry sweep: every n with two row counts, every row count with two n."""
    cases = []
    for i, n in enumerate(DIRECT_N):
        for rows in (DIRECT_ROWS[i % len(DIRECT_ROWS)], DIRECT_ROWS[(3 * i + 5) % len(DIRECT_ROWS)]):
            if (n, rows) not in cases:
                cases.append((n, rows))
    return cases


def sweep_columns(max_columns=6):
    """Yield (kind, n, column) over the sweep's matrices, at most max_columns columns of each."""
    for n, rows in direct_cases():
        for kind, make in (("random", random_matrix), ("near_tied", near_tied_matrix)):
            mat = make(n, rows, 1)
            for c in range(min(rows, max_columns)):
                yield kind, n, mat[:, c]


def calibrate(columns, seeds=(0,)):
    """Largest deviation of the perturbed kernel-order restatement from the reference: {"elpd", "lppd", "k"} -> {kind: value}, elpd and
    lppd relative to max(|v|, 1), k in units of 2^-52 cond; tail membership and k = +inf must agree exactly."""
    worst = {name: {} for name in ("elpd", "lppd", "k")}
    for kind, n, col in columns:
        ref = psis_column(col)
        for seed in seeds:
            got = psis_column(col, kernel_order=True, rng=np.random.default_rng([seed, n]))
            assert got["T"] == ref["T"] and np.array_equal(got["tail"], ref["tail"])
            assert np.isinf(got["k"]) == np.isinf(ref["k"]), (kind, n)
            for name in ("elpd", "lppd"):
                dev = abs(got[name] - ref[name]) / max(abs(ref[name]), 1.0)
                worst[name][kind] = max(worst[name].get(kind, 0.0), dev)
            if np.isfinite(ref["k"]):
                worst["k"][kind] = max(worst["k"].get(kind, 0.0), abs(got["k"] - ref["k"]) / (ref["cond"] * 2.0 ** -52))
    return worst

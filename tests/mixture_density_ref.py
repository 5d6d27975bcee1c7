"""CPU comparator of d3p_amd.mixture_density for tests/test_mixture_density_host.py and tests/test_gpu_mixture_density.py, built on
tests/mixture_ref.py (a64 and its condition scale, assign_inputs, logsumexp with max-subtraction), following DESIGN.md section 4g.

Per draw s, `a64[s, r, j]` is the float64 value of a from the float32 inputs and `scale[s, r, j]` the sum of the magnitudes of its
terms (mixture_ref.a64).  The device's float32 a is held within
    b[s, r, j] = BOUND_ULPS 2^-24 scale[s, r, j].
BOUND_ULPS is calibrated afresh for k_gmm_density's operation order, which `a32_restated` restates in numpy float32: rinv = 1 / sigs
once per draw; per term t = x - mu, z = t rinv, q = q + z z over c in index order; C_j = (log pis_j - H_j) - fl(d) log(2 pi) / 2 with
H_j the float32 sum of log sigs_jc in index order; a_j = -0.5 q_j + C_j -- every operation rounded on its own.  Over the GPU tests'
inputs (CASES: both input kinds at every shape of mixture_ref.SHAPES with n in 1, 2, 5, the row edges and the draw edges) the
largest error seen is A_ERR_SEEN_ULPS = 11.86 in units of 2^-24 scale (hard inputs at k = 16, d = 256: a serial float32 sum of 256
terms); BOUND_ULPS = 4 x that = 47.44, the project's margin (mixture_ref: it covers logf and the reciprocal differing in the last ulp
between libm and the device).

The downstream quantities get no invented tolerance.  They are judged by intervals in float64 with max-subtraction:
    ll   in [lse_j(a - b), lse_j(a + b)]
    lppd in [lse_s(ll_lo) - log n, lse_s(ll_hi) - log n]
    a draw's responsibility of j in [e^(a_j - b_j) / (e^(a_j - b_j) + sum_{i != j} e^(a_i + b_i)),
                                     e^(a_j + b_j) / (e^(a_j + b_j) + sum_{i != j} e^(a_i - b_i))]
    resp between the means of those ends over the draws
each widened by a rounding slack for the reduction's own float32 steps (expf, logf, the reciprocal of the sum, the running maximum's
rescaling, the final rounding to float32):
    ll, lppd:  SLACK_ULPS 2^-24 (1 + |value|)         resp:  SLACK_ULPS 2^-24   (a responsibility is at most 1)
The slack is calibrated the same way: the kernel's reduction restated in numpy (`ll32_restated`, `lppd32_restated`,
`resp32_restated`, with the waves' split of the draws and their fixed-order merge) against the float64 reduction of the SAME float32
a, so that it measures the reduction alone.  Largest error seen SLACK_ERR_SEEN_ULPS = 1.71 of those units (soft inputs at k = 3, d = 2); SLACK_ULPS
= 4 x that = 6.84.  The ends of ll that go into lppd's interval carry ll's slack.

test_mixture_density_host.py::test_bound_and_slack_calibration recomputes both figures and asserts them.
"""
import numpy as np

from d3p_amd import mixture_density as MD
from . import mixture_ref as R

T, DT = MD.ROW_TILE, MD.DRAW_TILE
HALF_LOG_2PI = R.HALF_LOG_2PI

A_ERR_SEEN_ULPS = 11.86
BOUND_ULPS = 47.44
SLACK_ERR_SEEN_ULPS = 1.71
SLACK_ULPS = 6.84

NS = (1, 2, 5)
# (k, d, rows, n): every shape of mixture_ref.SHAPES at n in 1, 2, 5; the row tile's edges; the draw split's edges (4 waves: 3, 5, 9;
# the two largest shapes split the draws over 2 waves: 1, 3, 5)
SHAPE_CASES = [(k, d, rows, n) for (k, d, rows) in R.SHAPES for n in NS]
ROW_EDGE_CASES = [(3, 2, rows, 2) for rows in (T - 1, T, T + 1, 2 * T + 1)]
DRAW_EDGE_CASES = [(3, 5, 3, n) for n in (DT - 1, DT + 1, 2 * DT + 1)] + [(16, 256, 5, 3), (32, 128, 5, 3)]
CASES = SHAPE_CASES + ROW_EDGE_CASES + DRAW_EDGE_CASES
KINDS = ("hard", "soft")


def draw_waves(k, d):
    """How many waves of a workgroup split the draws (d3p_gmm_density.hip: 4 where four latent copies fit in LDS beside the row
    tile, else 2): a function of (k, d) alone."""
    tile = (T * (d | 1) + 1) & ~1
    per_wave = 2 * k * d + ((k + 1) & ~1)
    return DT if 4 * (tile + DT * per_wave) <= 163840 else 2


# ------------------------------------------------------------------------------------------------ inputs
def _jitter(mus, sigs, pis, n, r, rel):
    """n draws around one parameter set: float32 (pis (n, k), mus (n, k, d), sigs (n, k, d))."""
    k, d = mus.shape
    p = pis[None] * r.uniform(0.9, 1.1, (n, k))
    p /= p.sum(axis=1, keepdims=True)
    m = mus[None] + rel * sigs[None] * r.normal(size=(n, k, d))
    s = sigs[None] * (1.0 + rel * r.uniform(-1.0, 1.0, (n, k, d)))
    return p.astype(np.float32), m.astype(np.float32), s.astype(np.float32)


def hard_inputs(k, d, rows, n):
    """mixture_ref.assign_inputs (well-separated clusters, near one-hot) replicated over n draws with per-draw jitter."""
    obs, mus, sigs, pis = R.assign_inputs(k, d, rows)
    r = np.random.default_rng(7000 + 100 * k + d + rows + n)
    return (obs,) + _jitter(mus.astype(np.float64), sigs.astype(np.float64), pis.astype(np.float64), n, r, 0.05)


def soft_inputs(k, d, rows, n):
    """Overlapping components: means within about one scale / sqrt(d) of each other, scales in [0.8, 1.25] (one scale per
    dimension, shared by the components up to the per-draw jitter, so that the components stay comparable at d = 256 too); rows drawn
    from the mixture.  Returns float32 (obs (rows, d), pis (n, k), mus (n, k, d), sigs (n, k, d))."""
    r = np.random.default_rng(9000 + 100 * k + d + rows + n)
    sc = r.uniform(0.85, 1.2, d)
    sigs = np.broadcast_to(sc[None], (k, d)).copy()
    mus = 0.7 * sc[None] * r.normal(size=(k, d)) / np.sqrt(d)
    pis = r.uniform(0.5, 1.5, k)
    pis /= pis.sum()
    z = r.integers(0, k, rows)
    obs = (mus[z] + sigs[z] * r.normal(size=(rows, d))).astype(np.float32)
    return (obs,) + _jitter(mus, sigs, pis, n, r, 0.03 / np.sqrt(d))


def inputs(kind, k, d, rows, n):
    return hard_inputs(k, d, rows, n) if kind == "hard" else soft_inputs(k, d, rows, n)


# ------------------------------------------------------------------------------------------------ a: float64 and the restatement
def a64_draws(obs, pis, mus, sigs):
    """(a (n, rows, k) float64, its condition scale) -- mixture_ref.a64 per draw."""
    both = [R.a64(obs, mus[s], sigs[s], pis[s]) for s in range(pis.shape[0])]
    return np.stack([x[0] for x in both]), np.stack([x[1] for x in both])


def a32_restated(obs, pis, mus, sigs):
    """k_gmm_density's operation order in numpy float32 (file docstring): (n, rows, k)."""
    x, p, m, s = (np.asarray(v, np.float32) for v in (obs, pis, mus, sigs))
    n, k, d = m.shape
    rinv = np.float32(1.0) / s
    H = np.zeros((n, k), np.float32)
    lg = np.log(s)
    for c in range(d):
        H = H + lg[:, :, c]
    with np.errstate(divide="ignore"):
        C = (np.log(p) - H) - np.float32(d) * np.float32(HALF_LOG_2PI)
    q = np.zeros((n, x.shape[0], k), np.float32)
    for c in range(d):
        t = x[None, :, None, c] - m[:, None, :, c]
        z = t * rinv[:, None, :, c]
        q = q + z * z
    a = np.float32(-0.5) * q + C[:, None, :]
    assert a.dtype == np.float32
    return a


def bound(scale):
    return BOUND_ULPS * 2.0 ** -24 * scale


def lse(a, axis):
    """logsumexp in float64 with max-subtraction along `axis` (removed); all -inf gives -inf."""
    a = np.asarray(a, np.float64)
    m = a.max(axis=axis, keepdims=True)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        out = safe + np.log(np.exp(a - safe).sum(axis=axis, keepdims=True))
    return np.squeeze(out, axis=axis)


def softmax64(a):
    a = np.asarray(a, np.float64)
    return np.exp(a - lse(a, -1)[..., None])


def slack(value):
    return SLACK_ULPS * 2.0 ** -24 * (1.0 + np.abs(value))


RESP_SLACK = SLACK_ULPS * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the reduction restated
def ll32_restated(a32):
    """(ll (n, rows) float32, p (n, rows, k) float32): m = max_j a_j, e_j = expf(a_j - m), the sum in index order, ll = m + logf(sum),
    p_j = e_j * (1 / sum)."""
    a32 = np.asarray(a32, np.float32)
    m = a32.max(axis=2)
    e = np.exp(a32 - m[..., None])
    sm = np.zeros_like(m)
    for j in range(a32.shape[2]):
        sm = sm + e[..., j]
    ll = m + np.log(sm)
    p = e * (np.float32(1.0) / sm)[..., None]
    assert ll.dtype == np.float32 and p.dtype == np.float32
    return ll, p


def lppd32_restated(ll32, W):
    """Wave w keeps a running (max float32, sum float64) over its draws w, w + W, ... with one float32 exp per draw; wave 0 merges
    the others in order in float64; the result is rounded to float32 once (finite inputs)."""
    n, rows = ll32.shape
    parts = []
    for w in range(W):
        m = np.full(rows, -np.inf, np.float32)
        s = np.zeros(rows, np.float64)
        for i in range(w, n, W):
            x = ll32[i]
            up = x > m
            with np.errstate(invalid="ignore"):
                s_up = s * np.exp((m - x).astype(np.float32)).astype(np.float64) + 1.0
                s_in = s + np.exp((x - m).astype(np.float32)).astype(np.float64)
            s = np.where(up, s_up, s_in)
            m = np.where(up, x, m)
        parts.append((m, s))
    m, s = parts[0]
    for m1, s1 in parts[1:]:
        mm = np.maximum(m, m1)
        with np.errstate(invalid="ignore"):
            a0 = np.where(m == -np.inf, s, s * np.exp(m.astype(np.float64) - mm))
            a1 = np.where(m1 == -np.inf, s1, s1 * np.exp(m1.astype(np.float64) - mm))
        m, s = mm, a0 + a1
    return ((m.astype(np.float64) + np.log(s)) - np.log(float(n))).astype(np.float32)


def resp32_restated(p32, W):
    n = p32.shape[0]
    tot = np.zeros(p32.shape[1:], np.float64)
    for w in range(W):
        acc = np.zeros(p32.shape[1:], np.float64)
        for i in range(w, n, W):
            acc = acc + p32[i].astype(np.float64)
        tot = tot + acc
    return (tot / float(n)).astype(np.float32)


def errors_of_case(kind, k, d, rows, n):
    """(largest |a32 - a64| in units of 2^-24 scale, largest error of the restated reduction in the slack's units)."""
    obs, pis, mus, sigs = inputs(kind, k, d, rows, n)
    a, scale = a64_draws(obs, pis, mus, sigs)
    a32 = a32_restated(obs, pis, mus, sigs)
    err_a = float(np.max(np.abs(a32.astype(np.float64) - a) / (2.0 ** -24 * scale)))
    ll32, p32 = ll32_restated(a32)
    W = draw_waves(k, d)
    a32d = a32.astype(np.float64)
    ll_x = lse(a32d, 2)
    e_ll = np.max(np.abs(ll32 - ll_x) / (2.0 ** -24 * (1.0 + np.abs(ll_x))))
    lp_x = lse(ll32.astype(np.float64), 0) - np.log(float(n))
    e_lp = np.max(np.abs(lppd32_restated(ll32, W) - lp_x) / (2.0 ** -24 * (1.0 + np.abs(lp_x))))
    e_rs = np.max(np.abs(resp32_restated(p32, W) - softmax64(a32d).mean(axis=0)) / 2.0 ** -24)
    return err_a, float(max(e_ll, e_lp, e_rs))


# ------------------------------------------------------------------------------------------------ intervals
_cache = {}


def reference(kind, k, d, rows, n):
    """The inputs and the float64 reference with its intervals for one case; computed once and shared (read-only)."""
    key_ = (kind, k, d, rows, n)
    if key_ not in _cache:
        obs, pis, mus, sigs = inputs(kind, k, d, rows, n)
        ref = intervals(obs, pis, mus, sigs)
        ref.update(obs=obs, pis=pis, mus=mus, sigs=sigs)
        for v in ref.values():
            v.setflags(write=False)
        _cache[key_] = ref
    return _cache[key_]


def intervals(obs, pis, mus, sigs):
    """{"a", "b", "ll", "ll_lo", "ll_hi", "lppd", "lppd_lo", "lppd_hi", "resp", "resp_lo", "resp_hi"} in float64 (file docstring)."""
    a, scale = a64_draws(obs, pis, mus, sigs)
    b = bound(scale)
    n, _, k = a.shape
    lo, hi = a - b, a + b
    ll = lse(a, 2)
    ll_lo, ll_hi = lse(lo, 2), lse(hi, 2)
    ll_lo, ll_hi = ll_lo - slack(ll_lo), ll_hi + slack(ll_hi)
    logn = np.log(float(n))
    lppd = lse(ll, 0) - logn
    lppd_lo, lppd_hi = lse(ll_lo, 0) - logn, lse(ll_hi, 0) - logn
    lppd_lo, lppd_hi = lppd_lo - slack(lppd_lo), lppd_hi + slack(lppd_hi)
    r_lo, r_hi = np.empty_like(a), np.empty_like(a)
    for j in range(k):
        rest = np.arange(k) != j
        if rest.any():
            r_lo[..., j] = np.exp(lo[..., j] - np.logaddexp(lo[..., j], lse(hi[..., rest], 2)))
            r_hi[..., j] = np.exp(hi[..., j] - np.logaddexp(hi[..., j], lse(lo[..., rest], 2)))
        else:
            r_lo[..., j] = r_hi[..., j] = 1.0
    return {"a": a, "b": b, "ll": ll, "ll_lo": ll_lo, "ll_hi": ll_hi, "lppd": lppd, "lppd_lo": lppd_lo, "lppd_hi": lppd_hi,
            "resp": softmax64(a).mean(axis=0), "resp_lo": r_lo.mean(axis=0) - RESP_SLACK, "resp_hi": r_hi.mean(axis=0) + RESP_SLACK}


def inside(x, lo, hi, what):
    x = np.asarray(x, np.float64)
    bad = ~((x >= lo) & (x <= hi))
    width = np.maximum(hi - lo, 1e-300)
    pos = np.max(np.abs(x - 0.5 * (lo + hi)) / (0.5 * width))
    print(f"{what}: farthest from the interval's centre {pos:.3f} half-widths")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside, first at {np.argwhere(bad)[0]}: {x[bad][0]!r} not in [{lo[bad][0]!r}, {hi[bad][0]!r}]"

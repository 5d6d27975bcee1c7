"""Float64 restatements of the stage, optimiser and mixture log-prob entries of d3p_amd/csrc/d3p_stages.hip, written from the
reference's text (d3p/svi.py, d3p/optimizers.py, d3p/gmm.py, numpyro.optim.Adam, jax.random.randint), not from the kernels.

Every function takes float32 arrays (scalars are rounded to float32 first, as the C entries receive them), works in float64 and returns
the value together with the condition number its bound is stated in: the sum of the magnitudes of the terms that were added.  Where
the reference's own float32 arithmetic leaves the format (a sum of squares or a square beyond float32) the restatement does too, so
that an overflow row is the reference's 0 / -inf / +inf and not a float64 value no float32 program can produce.

The case lists of tests/test_gpu_stages.py live here as well: tests/test_stages_host.py pins their lengths and the conditions the GPU
assertions rely on (margins of the accept / reject decisions, which rows overflow) on the CPU.

All bounds are in units of U = 2^-24, the largest relative error of one rounded float32 operation.
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126                       # the smallest normal float32: what a flushed or underflowed term can be off by
F32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103   # the smallest magnitude that rounds to +inf in float32 (round to nearest even)
HALF_LOG_2PI = 0.91893853320467274178
# powf's relative error.  The ROCm tree these tests were written against ships no document stating the device math library's ulp
# bounds, so this is the 1e-5 relative that tests/test_gpu_dpsvi.py asserts for the general-order norm.
POWF_REL = 1e-5


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


def _s(v):
    """A scalar as the C entry receives it: rounded to float32, then exact in float64."""
    return float(np.float32(v))


def _as_f32_range(a):
    """Values a float32 computation would have rounded to +-inf become +-inf."""
    a = np.asarray(a, np.float64)
    return np.where(np.abs(a) >= F32_OVERFLOW, np.copysign(np.inf, a), a)


# ------------------------------------------------------------------------------------------------------------ the restatements
def clip_rows(g, c):
    """d3p/svi.py:119-122 per row: g / max(1, ||row|| / c), jnp.maximum's NaN propagation (numpy.maximum has it too).  -> (value, |value|)"""
    c = _s(c)
    if c == 0.0:
        raise ValueError("The clipping threshold must be greater than 0.")
    g64 = _f64(g)
    with np.errstate(all="ignore"):
        ss = _as_f32_range((g64 * g64).sum(axis=1))
        factor = 1.0 / np.maximum(1.0, np.sqrt(ss) / c)
        out = g64 * factor[:, None]
    return out, np.abs(out)


def full_norm(v, ord=2):
    """numpy.linalg.norm of the flat vector (d3p/svi.py:68-87; an empty tree gives 0).  -> (value, |value|)"""
    v64 = _f64(v).reshape(-1)
    if v64.size == 0:
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        val = float(np.linalg.norm(v64, ord=ord))
    return val, abs(val)


def combine(g, loss=None):
    """d3p/svi.py:327-348: the column means and the mean loss.  -> (avg, sum|g| / B, loss, sum|loss| / B)"""
    g64 = _f64(g)
    B = g64.shape[0]
    avg, cond = g64.sum(axis=0) / B, np.abs(g64).sum(axis=0) / B
    if loss is None:
        return avg, cond, None, None
    l64 = _f64(loss)
    return avg, cond, float(l64.sum() / B), float(np.abs(l64).sum() / B)


def perturb_apply(avg, noise, dp_scale, c, n, obs_scale, factor):
    """d3p/svi.py:365-375, :487-488: (avg + noise * dp_scale * c / n) * obs_scale * factor.  -> (value, cond)"""
    a, z = _f64(avg), _f64(noise)
    scale = _s(dp_scale) * (_s(c) / _s(n))
    of = _s(obs_scale) * _s(factor)
    return (a + z * scale) * of, (np.abs(a) + np.abs(z * scale)) * abs(of)


def adam(x, m, v, g, i, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """numpyro.optim.Adam = jax.example_libraries.optimizers.adam: m = (1 - b1) g + b1 m, v = (1 - b2) g^2 + b2 v,
    x -= lr mhat / (sqrt(vhat) + eps) with mhat = m / (1 - b1^(i+1)), vhat likewise; g^2 leaves float32 where the reference's does.
    -> dict(x, m, v, upd = |lr mhat / (sqrt(vhat) + eps)|, cond_m, cond_v, upd_cond = the update with cond_m in the place of |m|:
    what an error of m stated in units of its terms, which may cancel, does to x)"""
    lr, b1, b2, eps = _s(lr), _s(b1), _s(b2), _s(eps)
    x, m, v, g = _f64(x), _f64(m), _f64(v), _f64(g)
    with np.errstate(all="ignore"):
        gg = _as_f32_range(g * g)
        m1 = (1.0 - b1) * g + b1 * m
        v1 = (1.0 - b2) * gg + b2 * v
        mhat = m1 / (1.0 - b1 ** (i + 1))
        vhat = v1 / (1.0 - b2 ** (i + 1))
        upd = lr * mhat / (np.sqrt(vhat) + eps)
        cond_m = (1.0 - b1) * np.abs(g) + b1 * np.abs(m)
        return dict(x=x - upd, m=m1, v=v1, upd=np.abs(upd), cond_m=cond_m, cond_v=(1.0 - b2) * gg + b2 * np.abs(v),
                    upd_cond=lr * (cond_m / (1.0 - b1 ** (i + 1))) / (np.sqrt(vhat) + eps))


def adam_power_amplification(i, b1, b2):
    """How a relative error of b^(i+1) reaches the update: through 1 - b1^(i+1) in full, through 1 - b2^(i+1) under the square root."""
    b1, b2 = _s(b1), _s(b2)
    p1, p2 = b1 ** (i + 1), b2 ** (i + 1)
    return p1 / (1.0 - p1) + 0.5 * p2 / (1.0 - p2)


def sgd(x, g, lr):
    """numpyro.optim.SGD: x - lr g.  -> (value, |x| + |lr g|)"""
    x, g, lr = _f64(x), _f64(g), _s(lr)
    return x - lr * g, np.abs(x) + np.abs(lr * g)


def adadp(x, lr, x_stepped, x_prev, g, i, tol=1.0, stability_check=True):
    """d3p/optimizers.py:29-112 on the flat vector: max(1, x) without the absolute value, the literal 0.9 / 1.1 clamps (as float32).
    -> dict(x, lr, x_stepped, x_prev, err (odd steps, else None), reject, cond = |x| + |lr g|)"""
    x, xs, xp, g = _f64(x), _f64(x_stepped), _f64(x_prev), _f64(g)
    lr, tol = _s(lr), _s(tol)
    new_x = x - 0.5 * lr * g
    cond = np.abs(x) + np.abs(lr * g)
    if i % 2 == 0:
        return dict(x=new_x, lr=lr, x_stepped=x - lr * g, x_prev=x, err=None, reject=False, cond=cond)
    with np.errstate(all="ignore"):
        e = (xs - new_x) / np.maximum(1.0, xs)
        err = float(np.sqrt(np.sum(e * e)))
        ratio = math.inf if err == 0.0 else tol / err
        new_lr = lr * min(max(math.sqrt(ratio), _s(0.9)), _s(1.1))
    reject = bool(stability_check and err > tol)
    return dict(x=xp.copy() if reject else new_x, lr=new_lr, x_stepped=xs, x_prev=xp, err=err, reject=reject, cond=cond)


def logsumexp_rows(a):
    """jax.scipy.special.logsumexp over the last axis: a NaN anywhere gives NaN, every term -inf gives -inf."""
    a = np.asarray(a, np.float64)
    out = np.empty(a.shape[0])
    for r, row in enumerate(a):
        if np.isnan(row).any():
            out[r] = np.nan
            continue
        mx = row.max()
        out[r] = mx if np.isinf(mx) else mx + math.log(np.exp(row - mx).sum())
    return out


def gmm_log_prob(x, locs, scales, pis):
    """d3p/gmm.py:71-86: logsumexp_k(log pi_k + sum_j log N(x_j; loc_kj, scale_kj)).  A component's per-coordinate terms are taken in
    float64 unless the reference's float32 term is not finite (z * z beyond float32, an infinite or NaN coordinate): then the term is
    that float32 value.  -> (value, |value|)"""
    x32, l32, s32 = f32(x), f32(locs), f32(scales)
    with np.errstate(all="ignore"):
        z32 = (x32[:, None, :] - l32[None]) / s32[None]
        t32 = np.float32(-0.5) * z32 * z32 - np.log(s32)[None] - np.float32(HALF_LOG_2PI)
        z64 = (_f64(x32)[:, None, :] - _f64(l32)[None]) / _f64(s32)[None]
        t64 = -0.5 * z64 * z64 - np.log(_f64(s32))[None] - HALF_LOG_2PI
        t = np.where(np.isfinite(t32), t64, t32.astype(np.float64))
        comp = t.sum(axis=2) + np.log(_f64(f32(pis)))[None]
    val = logsumexp_rows(comp)
    return val, np.abs(val)


def tf_randint(words_hi, words_lo, lo, hi):
    """jax.random.randint's combination of the two word streams of split(key) for int32 (jax/_src/random.py, jax <= 0.4.10) in Python
    integers; the two places where the uint32 arithmetic wraps are written out."""
    M = 1 << 32
    span = 1 if hi <= lo else (hi - lo) % M                 # maxval - minval, converted to uint32
    mult = (1 << 16) % span
    mult = ((mult * mult) % M) % span                       # wrap 1: the uint32 product of (2^16 % span) with itself
    out = np.empty(len(words_hi), np.int64)
    for j, (h, l) in enumerate(zip(words_hi, words_lo)):
        off = (((int(h) % span) * mult) % M + int(l) % span) % M   # wrap 2: the uint32 product and sum
        val = (lo % M + off % span) % M                            # minval + (offset % span) in 32 bits
        out[j] = val - M if val >= (1 << 31) else val
    return out.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ the case lists
def _paired(first, second):
    """Every value of `first` with two values of `second` (the pairing of psis_ref.direct_cases): no full product."""
    cases = []
    for i, a in enumerate(first):
        for b in (second[i % len(second)], second[(i + 2) % len(second)]):
            cases.append((a, b))
    return cases


CLIP_B = (1, 3, 4, 5, 257)                # 4 rows per workgroup
CLIP_P = (1, 63, 64, 65, 129, 4097)       # 64 lanes stride a row
CLIP_KINDS = ("below", "above", "at_c", "zero", "overflow", "nan", "inf")
CLIP_C = (1.0, 0.37, 2.5)


def clip_cases():
    return _paired(CLIP_P, CLIP_B)          # (P, B)


def clip_kind(case_index, row):
    return CLIP_KINDS[(row + case_index) % len(CLIP_KINDS)]


def clip_input(case_index):
    """(g float32 (B, P), c): row r is of kind clip_kind(case_index, r), so that the seven kinds rotate through every row position."""
    P, B = clip_cases()[case_index]
    c = CLIP_C[case_index % len(CLIP_C)]
    rng = np.random.default_rng([101, case_index])
    g = np.empty((B, P), np.float64)
    for r in range(B):
        kind = clip_kind(case_index, r)
        v = rng.standard_normal(P)
        v[np.abs(v) < 1e-3] = 1e-3
        unit = v / np.sqrt((v * v).sum())
        if kind == "below":
            row = unit * c * 0.01
        elif kind == "above":
            row = unit * c * 100.0
        elif kind == "at_c":
            row = unit * c
        elif kind == "zero":
            row = np.zeros(P)
        elif kind == "overflow":
            row = np.sign(v) * 1e20
        else:
            row = unit * c * 3.0
            row[(r * 7 + case_index) % P] = np.nan if kind == "nan" else np.inf
        g[r] = row
    return f32(g), c


NORM_N = (1, 255, 256, 257, 513, 65537)   # one 256-thread workgroup strides the vector
NORM_ORDS = (0, 1, 2, 3, 0.5, -1.5, math.inf, -math.inf)
NORM_CONTENTS = ("mixed", "zeros", "equal", "nan", "pos_inf", "neg_inf")


def norm_cases():
    return [(n, content) for n in NORM_N for content in NORM_CONTENTS]


def norm_inputs(n, content):
    """The vectors of one case: one, except for `nan` (a NaN at 0, 255, 256 and n - 1 in turn, where the vector has that index)."""
    rng = np.random.default_rng([202, n])
    base = rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)      # mixed magnitudes spanning 2^+-20
    base[base == 0] = 1.0
    if content == "mixed":
        return [f32(base)]
    if content == "zeros":
        v = base.copy()
        v[::3] = 0.0
        return [f32(v)]
    if content == "equal":
        return [f32(np.full(n, -0.7))]
    if content == "nan":
        out = []
        for at in sorted({0, 255, 256, n - 1}):
            if at < n:
                v = base.copy()
                v[at] = np.nan
                out.append(f32(v))
        return out
    v = base.copy()
    v[(n * 5) // 7] = np.inf if content == "pos_inf" else -np.inf
    return [f32(v)]


def norm_bound(n, ord):
    """The relative bound of one order in units of U: a thread's chain of ceil(n / 256) adds or fmas, eight adds of the LDS tree, the
    root; counts (ord 0) and selections (ord +-inf) are exact; a general order pays powf twice, per term and on the sum."""
    if ord == 0 or math.isinf(ord):
        return 0.0
    count = (-(-n // 256) + 12) * U
    return count if ord in (1, 2) else count + 2.0 * POWF_REL


COMBINE_B = (1, 7, 8, 9, 255, 256, 257)   # eight row groups per workgroup; the loss goes through 256 threads
COMBINE_P = (1, 31, 32, 33, 65, 1030)     # 32 columns per workgroup


def combine_cases():
    return _paired(COMBINE_B, COMBINE_P)    # (B, P)


def combine_input(B, P):
    """(g, loss): ordinary columns; every fourth column (B >= 2) cancels to about 2^-12 of the sum of its magnitudes."""
    rng = np.random.default_rng([303, B, P])
    g = rng.standard_normal((B, P)) + 0.5
    if B >= 2:
        for col in range(0, P, 4):
            t = np.abs(rng.standard_normal(B // 2)) + 0.5
            g[0:2 * (B // 2):2, col] = t
            g[1:2 * (B // 2):2, col] = -t * (1.0 - 2.0 ** -11)
            if B % 2:
                g[B - 1, col] = 0.0
    return f32(g), f32(rng.standard_normal(B) * 3.0 + 10.0)


PERTURB_SITES = ([0, 1, 15, 16, 17, 0, 2049], [1])   # one thread = one ChaCha block = 16 elements of a site
APPLY_N = (1, 255, 256, 257, 65537)

ADAM_P = (0, 1, 255, 256, 257, 65537)
ADAM_STEPS = (0, 1, 9, 999, 10 ** 6)
ADAM_HYPER = ((1e-3, 0.9, 0.999, 1e-8), (1e-2, 0.8, 0.99, 1e-6))      # numpyro's defaults and one other (lr, b1, b2, eps)
ADAM_SPECIAL_G = (0.0, 1e-30, 1e19, 1e20)


def adam_cases():
    return [(P, i) for P in ADAM_P for i in ADAM_STEPS]


def adam_input(P, i, random_moments):
    """(x, m, v, g, special): g holds ADAM_SPECIAL_G at its first entries, rotated by the step's position in ADAM_STEPS so that P = 1
    meets a different one at every step; special[j] names the entry's special value or is -1."""
    rng = np.random.default_rng([404, P, i, int(random_moments)])
    x = rng.standard_normal(P)
    g = rng.standard_normal(P) * 0.3
    m = rng.standard_normal(P) * 0.1 if random_moments else np.zeros(P)
    v = rng.random(P) * 0.05 + 1e-4 if random_moments else np.zeros(P)
    special = np.full(P, -1)
    rot = ADAM_STEPS.index(i)
    for j in range(min(P, len(ADAM_SPECIAL_G))):
        special[j] = (j + rot) % len(ADAM_SPECIAL_G)
        g[j] = ADAM_SPECIAL_G[special[j]]
    return f32(x), f32(m), f32(v), f32(g), special


def adam_pow_eps(i):
    """The relative error of b^(i+1) as the float32 program holds it.  Step 0: b itself, exact.  Step 10^6: the power has vanished.
    Step 1: b * b needs 48 bits, so even a correctly rounded float32 power is off by up to U, and so is the float32 reference's (2 U
    allows the device's powf one ulp instead of half).  Steps 9 and 999: powf's bound."""
    return {0: 0.0, 1: 2.0 * U, 10 ** 6: 0.0}.get(i, POWF_REL)


ADADP_P = (1, 257, 16383, 16384, 16385, 262145)   # k_adadp_err strides by 64 x 256; k_adadp_apply is capped at 1024 workgroups
ADADP_SCENARIOS = ("accept", "reject", "no_check", "zero_grad")
ADADP_LR0 = 0.05
ADADP_LR0_F32 = float(np.float32(ADADP_LR0))


def adadp_cases():
    return [(P, s) for P in ADADP_P for s in ADADP_SCENARIOS]


def adadp_input(P, scenario):
    """(x0, g_even, g_odd, tol, stability_check).  tol is set from the float64 error estimate of the odd step: 1.1 err (accepted,
    lr x sqrt(1.1)), 0.9 err (rejected with the check, kept without; lr x sqrt(0.9)); zero gradients give err = 0 and lr x 1.1."""
    rng = np.random.default_rng([505, P])
    x0 = f32(rng.standard_normal(P) * 2.0)
    if scenario == "zero_grad":
        return x0, f32(np.zeros(P)), f32(np.zeros(P)), 1.0, True
    g0, g1 = f32(rng.standard_normal(P) * 0.5), f32(rng.standard_normal(P) * 0.5)
    even = adadp(x0, ADADP_LR0, f32(np.zeros(P)), x0, g0, 0)
    odd = adadp(f32(even["x"]), even["lr"], f32(even["x_stepped"]), f32(even["x_prev"]), g1, 1, tol=1.0)
    tol = float(np.float32(odd["err"] * (1.1 if scenario == "accept" else 0.9)))
    return x0, g0, g1, tol, scenario != "no_check"


def adadp_lr_bound(P):
    return (-(-P // 16384) + 64 + 16) * U


GMM_K = (1, 4, 5, 16, 17, 63, 64)         # the kernel is instantiated for at most 4, 16 and 64 components
GMM_D = (1, 63, 64, 65, 129)              # 64 lanes stride the event dimension
GMM_B = (1, 3, 4, 5, 257)                 # 4 rows per workgroup
GMM_HOSTILE = ("pos_inf", "big", "nan")
GMM_RTOL, GMM_ATOL = 2e-5, 1e-4           # tests/test_gpu_gmm.py's


def gmm_cases():
    """(K, d, B): every K with two (d, B) pairs."""
    cases = []
    for i, K in enumerate(GMM_K):
        for d, B in ((GMM_D[i % 5], GMM_B[(3 * i + 5) % 5]), (GMM_D[(i + 2) % 5], GMM_B[(i + 1) % 5])):
            cases.append((K, d, B))
    return cases


def gmm_input(K, d, B):
    """(x, locs, scales, pis): ordinary rows; one pi = 0 among positive ones and a last component about 10^3 d log-units away (K >= 2)."""
    rng = np.random.default_rng([606, K, d, B])
    locs = rng.standard_normal((K, d)) * 3.0
    scales = 0.2 + rng.random((K, d))
    pis = rng.dirichlet(np.ones(K))
    if K >= 2:
        locs[K - 1] += 50.0
    if K >= 3:
        pis[K // 2] = 0.0
        pis /= pis.sum()
    return f32(rng.standard_normal((B, d)) * 3.0), f32(locs), f32(scales), f32(pis)


def gmm_hostile_positions(B):
    """First, inside a 4-row workgroup, last."""
    mid = (B // 2) | 2 if B > 5 else B // 2
    return sorted({0, mid, B - 1})


def gmm_hostile(x, rotation):
    """x with the hostile rows put in: position j of gmm_hostile_positions takes kind GMM_HOSTILE[(j + rotation) % 3].
    -> (x, {row: kind})"""
    x = x.copy()
    placed = {}
    for j, row in enumerate(gmm_hostile_positions(x.shape[0])):
        kind = GMM_HOSTILE[(j + rotation) % 3]
        if kind == "pos_inf":
            x[row, (row + rotation) % x.shape[1]] = np.inf
        elif kind == "big":
            x[row, :] = 1e30
        else:
            x[row, (row + 2 * rotation) % x.shape[1]] = np.nan
        placed[row] = kind
    return x, placed


RANDINT_N = (1, 257)
RANDINT_RANGES = ((0, 100000), (-7, 2 ** 31 - 1), (-2 ** 31, 2 ** 31 - 1), (0, 65537), (5, 5))
